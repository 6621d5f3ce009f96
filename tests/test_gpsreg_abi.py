"""The default values of the "SLAM + GPS registration" section of include/msfm.h (the struct layouts: tests/test_abi.py)."""
from metricsfm_amd import capi


def test_defaults_are_the_references():
    o = capi.gpsreg_options()
    assert (o.th_outlier, o.min_views, o.window, o.clip_deg) == (3.0, 3, 20, 80.0)
    assert capi.gpsreg_options(window=5).window == 5
