"""The defaults msfm_seed_default_options fills (basic_structs.h:174, :187, :190; the sample counts and seeds of the two
relpose calls); the layouts of the two structs of msfm_seed_hypotheses: tests/test_abi.py."""
from metricsfm_amd import capi


def test_seed_defaults_are_the_reference_values():
    o = capi.seed_options()
    assert (o.th_mse_reprojection, o.th_angle_small, o.th_seedpair_structures) == (3.0, 3.0 / 180.0 * 3.1415, 20)
    assert (o.ransac_times_5pt, o.ransac_times_8pt, o.seed_5pt, o.seed_8pt) == (100, 200, 0x4D53464D45, 0x4D53464D38)
    assert capi.seed_options(th_seedpair_structures=7).th_seedpair_structures == 7
