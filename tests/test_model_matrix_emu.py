"""Gordon et al., ThetaLogistic, StochVolLeverage and DiscreteCox on every step form, against the oracle
(tests/model_matrix_cases.py), on the emulator build of the kernel sources.  Skipped when a GPU is visible:
tests/test_model_matrix_gpu.py then runs the same cells."""
import pytest

import model_matrix_cases as mm

pytestmark = pytest.mark.skipif(
    __import__("conftest").HAS_GPU, reason="GPU visible: covered by test_model_matrix_gpu.py")


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


@pytest.mark.parametrize("cell", mm.DEGENERATE_CELLS)
@pytest.mark.parametrize("model,bad", mm.DEAD)
def test_dead_population(golden, model, bad, cell):
    mm.check_dead_population(golden, model, bad, cell)
