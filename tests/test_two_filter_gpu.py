"""Two-filter smoothing on the device (tests/two_filter_cases.py) on an MI355X, at the sizes that need one: ragged
particle counts on both sides, N_f != N_i, several source slices, every univariate transition family, an island of a
multi-island filter, and the comparison in law of the O(N) estimator with the O(N^2) one."""
import pytest

import two_filter_cases as tc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", tc.GPU_CASES)
def test_on2_equals_the_restated_double_sum(golden, case):
    tc.check_restated(golden, case)


def test_source_slices_are_a_geometry_not_a_result(golden, monkeypatch):
    tc.check_slices(golden, monkeypatch)


@pytest.mark.parametrize("case,P", [("lg_4099x1500", None), ("gordon_1501x1501", None), ("lg_4099x1500", 5000)])
def test_on_pairs_equal_the_restated_contract(golden, case, P):
    tc.check_pairs(golden, case, P)


def test_philox_mode_is_the_documented_stream(golden):
    tc.check_philox(golden)


def test_pinned_to_the_reference(golden):
    tc.check_pinned(golden)


def test_on_agrees_with_on2_in_law(golden):
    tc.check_law(golden)


def test_same_call_twice_reads_only_and_pickles(golden):
    tc.check_behaviour(golden)


def test_numpy_route_agrees_with_the_device_route(golden):
    tc.check_numpy_route(golden)


def test_refusals(golden, monkeypatch):
    tc.check_refusals(golden, monkeypatch)


def test_sqmc_filters_take_the_numpy_route(golden):
    tc.check_sqmc_takes_the_numpy_route(golden)
