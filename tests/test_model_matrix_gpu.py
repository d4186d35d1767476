"""Gordon et al., ThetaLogistic, StochVolLeverage and DiscreteCox on every step form, against the oracle
(tests/model_matrix_cases.py), on an MI355X: the one-workgroup filter, the flat step, the two-level step wide, tile
and ragged, with k_reduce2 in front, the spacings kernels, islands, the strict step, fused SQMC -- each (model, cell)
a teacher-forced audit of every particle at every step -- and the observations that leave one particle, or none."""
import pytest

import model_matrix_cases as mm

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cell", sorted(mm.CELLS))
@pytest.mark.parametrize("model", mm.MODELS)
def test_cell_against_oracle(golden, model, cell):
    mm.check_cell(golden, model, cell)


@pytest.mark.parametrize("model", mm.MODELS)
def test_evidence_across_a_skipped_resampling(golden, model):
    mm.check_skipped_resampling(golden, model)


@pytest.mark.parametrize("N", sorted(mm.STRICT_SIZES))
@pytest.mark.parametrize("model", mm.MODELS)
def test_strict_step_is_the_sequential_cdf(golden, model, N):
    mm.check_strict(golden, model, N)


@pytest.mark.parametrize("gather", [False, True], ids=["recompute", "gather"])
@pytest.mark.parametrize("model", mm.MODELS)
def test_fused_sqmc_against_oracle(golden, model, gather):
    mm.check_sqmc(golden, model, gather)


@pytest.mark.parametrize("model", mm.MODELS)
def test_flat_sqmc_equals_operator_path(golden, model):
    mm.check_sqmc_flat(golden, model)


@pytest.mark.parametrize("cell", mm.DEGENERATE_CELLS)
@pytest.mark.parametrize("model,bad", mm.ONE_SURVIVOR)
def test_one_survivor(golden, model, bad, cell):
    mm.check_one_survivor(golden, model, bad, cell)


# An observation no particle survives is a user's bad data point: the reference goes on with NaN summaries.  Last in
# this file.
@pytest.mark.parametrize("cell", mm.DEGENERATE_CELLS)
@pytest.mark.parametrize("model,bad", mm.DEAD)
def test_dead_population(golden, model, bad, cell):
    mm.check_dead_population(golden, model, bad, cell)
