"""QMC backward sampling (tests/smoothing_qmc_cases.py), CPU only: the NumPy restatement against the reference's own run
(tests/golden/ffbs_qmc_lg.npz), and the host route of ParticleHistory against the restatement."""
import smoothing_qmc_cases as qc


def test_restatement_gives_the_reference_paths_on_the_fixture(golden):
    qc.check_fixture(golden)


def test_host_route_equals_the_restatement(golden):
    qc.check_host_route(golden)
