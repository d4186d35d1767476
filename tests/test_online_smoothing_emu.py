"""On-line smoothing collectors on the device (tests/online_smoothing_cases.py) on the emulator build of the kernel
sources.  Skipped when a GPU is visible: tests/test_online_smoothing_gpu.py then runs the same checks at the sizes
that need one (N = 4099 would be 4099^2 pairs, twice, per step and collector here) and the comparison of Paris with the
O(N^2) smoother in law (16 runs of 30 steps, one workgroup per index in the exact launch)."""
import pytest

import online_smoothing_cases as oc

pytestmark = pytest.mark.skipif(
    __import__("conftest").HAS_GPU, reason="GPU visible: covered by test_online_smoothing_gpu.py")


@pytest.mark.parametrize("case", oc.EMU_CASES)
def test_naive_and_on2_equal_the_restated_recursions(golden, case):
    oc.check_restated(golden, case, emu=True)


def test_no_history_is_needed_and_one_may_be_kept(golden):
    oc.check_restated(golden, "guided_700", emu=True, store_history=True)


def test_source_slices_are_a_geometry_not_a_result(golden, monkeypatch):
    oc.check_slices(golden, monkeypatch)


@pytest.mark.parametrize("case,shape", [(c, s) for c in sorted(oc.PARIS_SHAPES_EMU) for s in oc.PARIS_SHAPES_EMU[c]])
def test_paris_indices_equal_the_restated_contract(golden, case, shape):
    oc.check_paris_indices(golden, case, *shape)


def test_paris_philox_mode_is_the_documented_streams(golden):
    oc.check_paris_philox(golden, case="guided_700", Nparis=1, T=3)


def test_pinned_to_the_reference(golden):
    oc.check_pinned(golden)


def test_same_run_twice_and_pickled_mid_run(golden):
    oc.check_deterministic_and_pickle(golden)


def test_the_update_only_reads_the_filter(golden):
    oc.check_reads_only(golden)


def test_host_route_agrees_with_the_device_route(golden):
    oc.check_host_route_agrees(golden)


def test_refusals(golden):
    oc.check_refusals(golden)
