"""The log-weight stores a resampling step leaves out (tests/lazy_lw_cases.py) on an MI355X: a run in one
smc_filter_step call against the same run with every store made (SMC_EAGER_LW=1) and one step per call, the call
boundary at every step, the filters that never leave a store out, pickling and cloning between two calls."""
import pytest

import lazy_lw_cases as lc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", sorted(lc.CASES))
def test_lazy_equals_eager_equals_stepwise(golden, case):
    lc.check_three_runs(golden, case)


@pytest.mark.parametrize("case", sorted(lc.CASES))
def test_every_call_boundary(golden, case):
    lc.check_boundaries(golden, case)


@pytest.mark.parametrize("case", sorted(lc.CASES))
def test_interior_steps_hold_every_transition(golden, case):
    lc.check_coverage(golden, case)


def test_ineligible_filters_always_store(golden):
    lc.check_ineligible(golden)


@pytest.mark.parametrize("case", ["toy_2048", "cox_3x2048", "theta_1501"])
def test_state_transport_between_calls(golden, case):
    lc.check_state_transport(golden, case)
