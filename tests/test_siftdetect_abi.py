"""The detector's exports without a device: the prototypes the binding reads from include/msfm.h are the ones written here by
hand, the library has the symbols, null handles are refused, and the host numbers of metricsfm_amd/csrc/sift_args.h are the ones
the restatement makes."""
import ctypes as C
import os
import subprocess

import numpy as np

from metricsfm_amd import _abi as A
from metricsfm_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_prototypes_read_from_the_header():
    vp, i, f = C.c_void_p, C.c_int, C.c_float
    fp, ip, i64p = A.c_float_p, A.c_int_p, C.POINTER(C.c_int64)
    want = {
        "msfm_scalespace_detect": (i, [vp, f, f, i, fp, ip, i64p]),
        "msfm_descset_extract": (i, [vp, i, vp, f, f, i, i, i64p]),
    }
    L = capi.lib()
    for name, (restype, argtypes) in want.items():
        assert capi.PROTOTYPES[name] == (restype, argtypes), name
        assert name in capi.SYMBOLS and hasattr(L, name), name
        assert getattr(L, name).restype is restype and list(getattr(L, name).argtypes) == argtypes, name


def test_null_handles_are_refused():
    L = capi.lib()
    frames, n, st = np.zeros((4, 4), np.float32), C.c_int32(-3), np.full(len(A.SIFT_DETECT_STATS), -1, np.int64)
    assert L.msfm_scalespace_detect(None, 0.0, 10.0, 4, A.ptr(frames, A.c_float_p), C.byref(n), A.ptr(st, C.POINTER(C.c_int64))) == A.MSFM_E_INVAL
    assert L.msfm_descset_extract(None, 0, None, 0.0, 10.0, 4, 0, A.ptr(st, C.POINTER(C.c_int64))) == A.MSFM_E_INVAL
    assert n.value == -3 and (st == -1).all() and not frames.any()


def test_host_numbers_and_checks(tmp_path):
    """sift_args.h compiled as plain C++: the threshold checks, the edge bound, sigmaw and a frame's sigma as include/msfm.h words
    them, and the sizes of the two records that cross PCIe."""
    src = tmp_path / "t.cpp"
    src.write_text('#include "sift_args.h"\n#include <cmath>\nint main() {\n'
                   '  if (!sift_check_detect(0.f, 10.f, 65535).empty() || !sift_check_detect(0.f, 0.f, 0).empty()) return 1;\n'
                   '  if (sift_check_detect(-1.f, 10.f, 1).empty() || sift_check_detect(NAN, 10.f, 1).empty() || sift_check_detect(0.f, INFINITY, 1).empty()) return 2;\n'
                   '  if (sift_check_detect(0.f, -0.5f, 1).empty() || sift_check_detect(0.f, 10.f, -1).empty() || sift_check_detect(0.f, 10.f, 65536).empty()) return 3;\n'
                   '  if (sift_edge_bound(10.f) != 12.1f) return 4;\n'
                   '  if (sift_sigmaw(3, 0.f) != (float)(1.5 * 1.6 * std::pow(2.0, 1.0 / 3))) return 5;\n'
                   '  if (sift_frame_sigma(5, 2, 1.25f) != (float)(1.6 * std::pow(2.0, 1.0 / 5) * std::pow(2.0, 2 + 1.25 / 5))) return 6;\n'
                   '  if (sizeof(SiftRawKp) != 32 || sizeof(SiftOrientIn) != 20 || SIFT_DETECT_STATS != 18 || SIFT_ST_D2H != 17) return 7;\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "t"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "metricsfm_amd", "csrc"), str(src), "-o", str(exe)])
    assert subprocess.run([str(exe)]).returncode == 0
