"""The log-weight stores a resampling step leaves out (tests/lazy_lw_cases.py) on the emulator build of the kernel
sources.  Skipped when a GPU is visible: tests/test_lazy_lw_gpu.py then runs the same checks, at full length."""
import pytest

import lazy_lw_cases as lc

pytestmark = pytest.mark.skipif(
    __import__("conftest").HAS_GPU, reason="GPU visible: covered by test_lazy_lw_gpu.py")

T_SHORT = 16        # (the emulator runs a step of these sizes in 0.1-0.3 s: every boundary of 16 steps, not of 40)


@pytest.mark.parametrize("case", sorted(lc.CASES))
def test_lazy_equals_eager_equals_stepwise(golden, case):
    lc.check_coverage(golden, case)
    lc.check_three_runs(golden, case)


@pytest.mark.parametrize("case", ["toy_2048", "theta_1501"])
def test_every_call_boundary(golden, case):
    lc.check_coverage(golden, case, T=T_SHORT)
    lc.check_boundaries(golden, case, T=T_SHORT)


def test_ineligible_filters_always_store(golden):
    lc.check_ineligible(golden, T=12)


def test_state_transport_between_calls(golden):
    lc.check_state_transport(golden, "gordon_3000", ks=(7,))
