"""Backward sampling on the device (tests/smoothing_cases.py) on the emulator build of the kernel sources.  Skipped
when a GPU is visible: tests/test_smoothing_gpu.py then runs the same checks, with more trajectories."""
import pytest

import smoothing_cases as sc

pytestmark = pytest.mark.skipif(
    __import__("conftest").HAS_GPU, reason="GPU visible: covered by test_smoothing_gpu.py")


def test_pinned_to_the_reference(golden):
    sc.check_pinned(golden)


@pytest.mark.parametrize("case", sorted(sc.SHAPES_EMU))
def test_rows_equal_the_restated_reference(golden, case):
    sc.check_restated(golden, case, emu=True)


def test_philox_mode_is_the_documented_streams(golden):
    sc.check_philox_streams(golden)


def test_law_of_the_exact_sampler(golden):
    sc.check_law(golden, M=512)


def test_refusals(golden):
    sc.check_refusals(golden)


def test_sampling_leaves_the_filter_alone(golden):
    sc.check_non_interference(golden, N=1500)
