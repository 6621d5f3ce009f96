"""The default values of the "Which image pairs to match" section of include/msfm.h and the refusals that need no device
(the struct layouts: tests/test_abi.py)."""
import ctypes as C
import subprocess

from metricsfm_amd import _abi as A
from metricsfm_amd import capi


def test_defaults_are_the_references():
    o = capi.pair_select_options()
    assert (o.th_init_matches, o.th_inliers, o.max_hypotheses) == (30, 20, 0)
    f, d = o.fransac, capi.fransac_options()
    assert (f.threshold, f.confidence, f.max_iterations, f.min_points, f.min_inliers, f.seed) == (3.0, 0.99, 2000, 30, 30, d.seed)
    o = capi.pair_select_options(th_inliers=5, max_iterations=100)
    assert o.th_inliers == 5 and o.fransac.max_iterations == 100


def test_null_handles_are_refused_without_a_device():
    L = capi.lib()
    h = C.c_void_p()
    one = C.c_int32(1)
    assert L.msfm_wordset_create(None, 2, C.byref(one), None, None, 10, None, 0, C.byref(h)) == A.MSFM_E_INVAL
    assert L.msfm_pair_select(None, 0, 1, None, C.byref(h)) == A.MSFM_E_INVAL
    assert L.msfm_wordset_size(None, None, None, None, None, None) == A.MSFM_E_INVAL
    assert L.msfm_wordset_fetch(None, None, None, None, None, None, None) == A.MSFM_E_INVAL
    assert L.msfm_pair_set_size(None, None, None, None, None) == A.MSFM_E_INVAL
    assert L.msfm_pair_set_fetch(None, None, None, None, None, None, None, None, None) == A.MSFM_E_INVAL
    L.msfm_wordset_destroy(None)
    L.msfm_pair_set_destroy(None)
    L.msfm_pair_select_default_options(None)


def test_argument_checks_under_the_host_sanitizers(tmp_path):
    """metricsfm_amd/csrc/pairsel_args.h - the checks msfm_wordset_create / msfm_pair_select refuse with - in the stand-alone
    tests/pairselect_host_check.cc, built -DPAIRSELECT_ARGS_ONLY with AddressSanitizer and UBSan: no library, no device."""
    from tests import pairselect_data as D
    exe = tmp_path / "pairselect_args_check"
    subprocess.check_call(D.host_check_command(exe, args_only=True))
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "pairselect_host_check ok" in run.stdout, run.stdout + run.stderr
