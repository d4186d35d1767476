"""Backward sampling on the device (tests/smoothing_cases.py) on an MI355X: the reference's own FFBS run reproduced
index for index, both samplers against the reference's expression in NumPy at sizes that reach every code path, the
Philox streams as documented, the law of the exact sampler, refusals, and a filter that steps on after sampling."""
import pytest

import smoothing_cases as sc

pytestmark = pytest.mark.gpu


def test_pinned_to_the_reference(golden):
    sc.check_pinned(golden)


@pytest.mark.parametrize("case", sorted(sc.SHAPES))
def test_rows_equal_the_restated_reference(golden, case):
    sc.check_restated(golden, case)


def test_philox_mode_is_the_documented_streams(golden):
    sc.check_philox_streams(golden)


def test_law_of_the_exact_sampler(golden):
    sc.check_law(golden, M=4096)


def test_refusals(golden):
    sc.check_refusals(golden)


def test_sampling_leaves_the_filter_alone(golden):
    sc.check_non_interference(golden)
