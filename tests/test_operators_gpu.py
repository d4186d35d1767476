"""The operator path against NumPy (tests/operator_cases.py) on an MI355X: DeviceArray arithmetic, the distributions
classes on device arrays, X[A], X @ M, column / stack_columns and Weights -- every op code, operand form and refusal,
at the same sizes as tests/test_operators_emu.py (each op is one launch over at most 16 k elements)."""
import pytest

import operator_cases as oc

pytestmark = pytest.mark.gpu


def test_every_op_code_is_covered():
    oc.check_op_table()


@pytest.mark.parametrize("n", oc.SIZES_1D)
def test_elementwise_exact_ops_every_route(n):
    oc.check_elementwise_exact(n)


@pytest.mark.parametrize("shape", oc.SHAPES_2D)
def test_elementwise_operand_forms(shape):
    oc.check_elementwise_forms(shape)


def test_libm_functions_within_the_measured_bounds():
    oc.check_libm()


def test_pow_routes_and_undefined_ufuncs():
    oc.check_pow_routes()


def test_elementwise_c_entry():
    oc.check_elementwise_c_level()


@pytest.mark.parametrize("N", (1, 2, 255, 257))
def test_normal_all_operand_kinds(N):
    oc.check_normal(N)


@pytest.mark.parametrize("N", (1, 257))
def test_normal_philox_stream(N):
    oc.check_normal_philox(N)


@pytest.mark.parametrize("N", (1, 257))
def test_poisson_operand_kinds(N):
    oc.check_poisson(N)


@pytest.mark.parametrize("d", (1, 2, 3, 33, 64))
@pytest.mark.parametrize("N", (1, 257))
def test_mvnormal_operand_kinds(d, N):
    oc.check_mvnormal(d, N)


def test_mvnormal_dimension_65_is_refused():
    oc.check_mvnormal_refused()


def test_indep_prod_host_and_device():
    oc.check_indep_prod()


@pytest.mark.parametrize("d", (1, 5, 64))
@pytest.mark.parametrize("k", (1, 5, 64))
@pytest.mark.parametrize("N", (1, 257))
def test_rows_matmul_within_the_derived_bound(N, d, k):
    oc.check_matmul(N, d, k)


def test_rows_matmul_edges():
    oc.check_matmul_edges()


@pytest.mark.parametrize("shape", ((1, 1), (257, 3), (256, 64)))
def test_columns_and_stack(shape):
    oc.check_columns(shape)


@pytest.mark.parametrize("d", (1, 5))
@pytest.mark.parametrize("M", (1, 257))
def test_gather_index_kinds_and_sources(M, d):
    oc.check_gather(M, d)


def test_host_index_follows_numpy():
    oc.check_host_index()


def test_refusals():
    oc.check_refusals()
