"""Conditional SMC on the device (tests/csmc_cases.py) on an MI355X: the reference's own CSMC run reproduced entry for
entry, every step against the contract restated in NumPy at the sizes that reach every code path, the new trajectories of
all islands against the genealogy and against the existing backward sampler, the Philox streams as documented, invariance
of the smoothing law under repeated conditional updates, the life cycle of a conditional filter, and refusals."""
import pytest

import csmc_cases as cc

pytestmark = pytest.mark.gpu


def test_pinned_to_the_reference(golden):
    cc.check_pinned(golden)


@pytest.mark.parametrize("case", sorted(cc.CASES))
def test_steps_and_paths_equal_the_restated_contract(golden, case):
    cc.check_restated(golden, case)


def test_philox_mode_is_the_documented_streams(golden):
    cc.check_philox_streams(golden)


@pytest.mark.parametrize("backward", [False, True], ids=["genealogy", "backward"])
def test_conditional_updates_leave_the_smoothing_law_invariant(golden, backward):
    cc.check_invariance(golden, C=512, backward=backward)


def test_lifecycle(golden):
    cc.check_lifecycle(golden)


def test_refusals(golden):
    cc.check_refusals(golden)
