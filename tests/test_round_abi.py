"""The defaults msfm_round_default_options documents (the layouts of the structs of msfm_round_adjust: tests/test_abi.py)."""
from metricsfm_amd import capi


def test_round_defaults_are_the_references():
    o = capi.round_options()
    for b in (o.partial, o.full):
        assert (b.max_num_iterations, b.huber_delta, b.function_tolerance, b.gradient_tolerance, b.parameter_tolerance) == (100, 1.0, 1e-6, 1e-10, 1e-8)
    assert (o.weight_partial, o.weight_full, o.th_mse_outliers, o.keep_problem) == (2.0, 1.0, 1.0, 0)
    o = capi.round_options(keep_problem=1, partial=dict(max_num_iterations=7))
    assert (o.partial.max_num_iterations, o.full.max_num_iterations, o.keep_problem) == (7, 100, 1)
