"""The vocabulary-training exports without a device: null handles are refused, the prototypes are the ones written here, the
defaults are the reference's, and the argument checks of voctrain_args.h run in a stand-alone program under the host sanitizers."""
import ctypes as C
import inspect
import os
import subprocess

from metricsfm_amd import _abi as A
from metricsfm_amd import capi
from tests import voctrain_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_null_handles_are_refused():
    L = capi.lib()
    out = C.c_void_p()
    assert L.msfm_descset_voctree_train(None, 10, 6, 11, 1, 0, C.byref(out)) == A.MSFM_E_INVAL
    assert L.msfm_voctree_train_stats(*([None] * 13)) == A.MSFM_E_INVAL
    assert L.msfm_voctree_fetch(None, None, None, None, None, None, None) == A.MSFM_E_INVAL
    assert not out.value


def test_prototypes_and_defaults():
    """The options are plain arguments and the statistics come from a getter, so include/msfm.h gains no struct; the binding's
    defaults are the reference's (fbow's Params{k, L, nthreads, maxIters = 11}; database.cc:658, :673), which the host check
    below asserts of voctrain_defaults, the library's statement of them."""
    i, vp, P = C.c_int, C.c_void_p, C.POINTER
    ip, i64p = A.c_int_p, P(C.c_int64)
    assert capi.PROTOTYPES["msfm_descset_voctree_train"] == (i, [vp, i, i, i, i, C.c_uint64, P(vp)])
    assert capi.PROTOTYPES["msfm_voctree_train_stats"] == (i, [vp, ip, i64p, ip, i64p, ip, ip, ip, ip, ip, ip, ip, ip])
    assert capi.PROTOTYPES["msfm_voctree_fetch"] == (i, [vp, P(C.c_uint16), A.c_float_p, P(C.c_uint32), A.c_float_p, P(C.c_uint16), P(C.c_uint32)])
    assert inspect.signature(capi.DescSet.train_voctree).parameters["k"].default == 10
    assert [p.default for p in list(inspect.signature(capi.DescSet.train_voctree).parameters.values())[1:]] == [10, 6, 11, 1, 0]
    assert not hasattr(A, "VoctrainOptions") and "msfm_voctrain" not in open(os.path.join(ROOT, "include", "msfm.h")).read()


def test_argument_checks_under_the_host_sanitizers(tmp_path):
    exe = tmp_path / "voctrain_host_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "voctrain_host_check.cc"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "voctrain_host_check ok" in out.stdout
    # the library's draw and the restatement's are the same function
    words = out.stdout.split()
    assert [int(words[-2]), int(words[-1])] == [V.draw(0, 0, 0, 0), V.draw(7, 3, 11, 2)]
