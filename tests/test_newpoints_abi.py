"""The defaults msfm_new_points_default_options fills (basic_structs.h:187, :190, :191; the 500 of sfm_incremental.cc:781);
the layouts of the two structs of msfm_new_points: tests/test_abi.py."""
from metricsfm_amd import capi


def test_new_points_defaults_are_the_reference_values():
    o = capi.new_points_options()
    assert (o.th_mse_reprojection, o.th_angle_small, o.th_angle_large, o.th_matches_large) == (3.0, 3.0 / 180.0 * 3.1415, 5.0 / 180.0 * 3.1415, 500)
    assert capi.new_points_options(th_matches_large=7).th_matches_large == 7
