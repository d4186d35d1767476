"""On-line smoothing collectors on the device (tests/online_smoothing_cases.py) on an MI355X: naive and O(N^2)
recursions step by step against their restatement in NumPy on filters that cover both step forms, the one-launch
filter, a time-dependent transition and both scale slots; Paris indices against the restated contract in the three
rejection launches; the reference's own estimates; Paris in law; determinism, pickling, non-interference, the host
route and the refusals."""
import pytest

import online_smoothing_cases as oc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", oc.GPU_CASES)
def test_naive_and_on2_equal_the_restated_recursions(golden, case):
    oc.check_restated(golden, case)


def test_no_history_is_needed_and_one_may_be_kept(golden):
    oc.check_restated(golden, "guided_700", store_history=True)


def test_source_slices_are_a_geometry_not_a_result(golden, monkeypatch):
    oc.check_slices(golden, monkeypatch)


def test_geometry_thresholds_of_the_all_pairs_launch(golden, monkeypatch):
    oc.check_geometry_thresholds(golden, monkeypatch)


@pytest.mark.parametrize("case,shape", [(c, s) for c in sorted(oc.PARIS_SHAPES) for s in oc.PARIS_SHAPES[c]])
def test_paris_indices_equal_the_restated_contract(golden, case, shape):
    oc.check_paris_indices(golden, case, *shape)


def test_paris_philox_mode_is_the_documented_streams(golden):
    oc.check_paris_philox(golden)


def test_pinned_to_the_reference(golden):
    oc.check_pinned(golden)


def test_paris_is_the_on2_smoother_in_law(golden):
    oc.check_paris_law(golden)


def test_same_run_twice_and_pickled_mid_run(golden):
    oc.check_deterministic_and_pickle(golden)


def test_the_update_only_reads_the_filter(golden):
    oc.check_reads_only(golden)


def test_host_route_agrees_with_the_device_route(golden):
    oc.check_host_route_agrees(golden)


def test_refusals(golden):
    oc.check_refusals(golden)
