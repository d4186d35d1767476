"""Hybrid rejection backward sampling on the device (tests/smoothing_reject_cases.py) on an MI355X: every row against
the contract restated in NumPy at sizes that reach the three launches, degenerate and looser bounds, the Philox streams
as documented, the law against the exact marginals and against the reference's own sampler, refusals, and a filter that
steps on after sampling."""
import pytest

import smoothing_reject_cases as rc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", sorted(rc.SHAPES))
def test_rows_equal_the_restated_contract(golden, case):
    rc.check_restated(golden, case)


def test_degenerate_and_looser_bounds(golden):
    rc.check_degenerate_bounds(golden)


def test_philox_mode_is_the_documented_streams(golden):
    rc.check_philox_streams(golden)


def test_law_is_the_ffbs_law(golden):
    rc.check_law(golden, M=4096)


def test_pinned_to_the_reference_in_law(golden):
    rc.check_pinned_in_law(golden)


def test_refusals(golden):
    rc.check_refusals(golden)


def test_sampling_leaves_the_filter_alone(golden):
    rc.check_non_interference(golden)
