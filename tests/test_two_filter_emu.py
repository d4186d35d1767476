"""Two-filter smoothing on the device (tests/two_filter_cases.py) on the emulator build of the kernel sources.  Skipped
when a GPU is visible: tests/test_two_filter_gpu.py then runs the same checks at the sizes that need one, and the
comparison in law (80 calls of 4096 pairs)."""
import pytest

import two_filter_cases as tc

pytestmark = pytest.mark.skipif(
    __import__("conftest").HAS_GPU, reason="GPU visible: covered by test_two_filter_gpu.py")


@pytest.mark.parametrize("case", tc.EMU_CASES)
def test_on2_equals_the_restated_double_sum(golden, case):
    tc.check_restated(golden, case, emu=True)


def test_source_slices_are_a_geometry_not_a_result(golden, monkeypatch):
    tc.check_slices(golden, monkeypatch)


@pytest.mark.parametrize("case,P", [("lg_1500x700", None), ("gordon_1501x1501", None), ("lg_1500x700", 5000)])
def test_on_pairs_equal_the_restated_contract(golden, case, P):
    tc.check_pairs(golden, case, P, emu=True)


def test_philox_mode_is_the_documented_stream(golden):
    tc.check_philox(golden)


def test_pinned_to_the_reference(golden):
    tc.check_pinned(golden)


def test_same_call_twice_reads_only_and_pickles(golden):
    tc.check_behaviour(golden)


def test_numpy_route_agrees_with_the_device_route(golden):
    tc.check_numpy_route(golden, emu=True)


def test_refusals(golden, monkeypatch):
    tc.check_refusals(golden, monkeypatch)


def test_sqmc_filters_take_the_numpy_route(golden):
    tc.check_sqmc_takes_the_numpy_route(golden)
