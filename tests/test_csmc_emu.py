"""Conditional SMC on the device (tests/csmc_cases.py) on the emulator build of the kernel sources.  Skipped when a GPU
is visible: tests/test_csmc_gpu.py then runs the same checks, with more chains."""
import pytest

import csmc_cases as cc

pytestmark = pytest.mark.skipif(
    __import__("conftest").HAS_GPU, reason="GPU visible: covered by test_csmc_gpu.py")


def test_pinned_to_the_reference(golden):
    cc.check_pinned(golden)


@pytest.mark.parametrize("case", sorted(cc.CASES))
def test_steps_and_paths_equal_the_restated_contract(golden, case):
    cc.check_restated(golden, case)


def test_philox_mode_is_the_documented_streams(golden):
    cc.check_philox_streams(golden)


@pytest.mark.parametrize("backward", [False, True], ids=["genealogy", "backward"])
def test_conditional_updates_leave_the_smoothing_law_invariant(golden, backward):
    cc.check_invariance(golden, C=128, backward=backward)


def test_lifecycle(golden):
    cc.check_lifecycle(golden)


def test_refusals(golden):
    cc.check_refusals(golden)
