"""Hybrid rejection backward sampling on the device (tests/smoothing_reject_cases.py) on the emulator build of the
kernel sources.  Skipped when a GPU is visible: tests/test_smoothing_reject_gpu.py then runs the same checks, with more
trajectories (and the comparison with the reference's own sampler, which needs them)."""
import pytest

import smoothing_reject_cases as rc

pytestmark = pytest.mark.skipif(
    __import__("conftest").HAS_GPU, reason="GPU visible: covered by test_smoothing_reject_gpu.py")


@pytest.mark.parametrize("case", sorted(rc.SHAPES_EMU))
def test_rows_equal_the_restated_contract(golden, case):
    rc.check_restated(golden, case, emu=True)


def test_degenerate_and_looser_bounds(golden):
    rc.check_degenerate_bounds(golden)


def test_philox_mode_is_the_documented_streams(golden):
    rc.check_philox_streams(golden)


def test_law_is_the_ffbs_law(golden):
    rc.check_law(golden, M=512)


def test_refusals(golden):
    rc.check_refusals(golden)


def test_sampling_leaves_the_filter_alone(golden):
    rc.check_non_interference(golden, N=1500)
