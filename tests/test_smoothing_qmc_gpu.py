"""QMC backward sampling on the device (tests/smoothing_qmc_cases.py) on the MI355X."""
import pytest

import smoothing_qmc_cases as qc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", sorted(qc.CASES))
def test_rows_equal_the_restated_reference_in_both_geometries(golden, case):
    qc.check_restated(golden, case)


def test_h_orders_are_the_sorted_order_of_every_step(golden):
    qc.check_h_orders(golden)


def test_ends_of_the_unit_interval(golden):
    qc.check_edges(golden)


def test_qmc_property_mean_within_one_iid_standard_error(golden):
    qc.check_qmc_property(golden, M=1024)


def test_refusals(golden):
    qc.check_refusals(golden)


def test_sampling_leaves_the_filter_alone(golden):
    qc.check_non_interference(golden)
