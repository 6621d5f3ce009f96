"""The defaults msfm_localize_pose_default_options fills (basic_structs.h:186, :177; the 200 samples of
absolute_pose_via_epnp.cc; the sweep of msfm_epnpf_default_options); the layout of msfm_localize_pose_options: tests/test_abi.py."""
from metricsfm_amd import _abi as A
from metricsfm_amd import capi


def test_localize_pose_defaults_are_the_reference_values():
    o = capi.localize_pose_options()
    assert (o.th_mse_localization, o.th_min_2d3d_corres, o.max_iter, o.seed, o.first_row, o.max_tries) == (5.0, 20, 200, 0x4D53464D50, 0, 16)
    d = capi.epnpf_options()
    assert all(getattr(o.sweep, f) == getattr(d, f) for f, _ in A.EpnpfOptions._fields_)
    o = capi.localize_pose_options(max_tries=1, sweep=dict(f_ratio_step=0.05))
    assert o.max_tries == 1 and o.sweep.f_ratio_step == 0.05 and o.sweep.f_ratio_min == 0.5
