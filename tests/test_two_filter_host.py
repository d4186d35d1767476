"""Two-filter smoothing on histories kept on the host (tests/two_filter_cases.py): operator-path filters and the host
``ParticleHistory`` take the NumPy route.  Runs with or without a GPU."""
import two_filter_cases as tc


def test_operator_path_filters_take_the_numpy_route(golden):
    tc.check_operator_path_filters(golden)
