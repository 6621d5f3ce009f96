"""The stereo-rectification exports without a device: the prototypes the binding reads from include/msfm.h are the ones written here
by hand, the library has the symbols, null handles are refused, and the tables of _abi.py say what the header's text says."""
import ctypes as C
import os
import re

import numpy as np

from metricsfm_amd import _abi as A
from metricsfm_amd import _header, capi, dense

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_text():
    with open(_header.HEADER) as fh:
        return fh.read()


def test_prototypes_read_from_the_header():
    vp, vpp, i, dp = C.c_void_p, C.POINTER(C.c_void_p), C.c_int, A.c_double_p
    ip, i64p, u8p = A.c_int_p, C.POINTER(C.c_int64), A.c_u8_p
    want = {
        "msfm_stereo_rectify": (i, [dp, dp, dp, dp, dp, dp, i, i, dp, dp, dp, dp, dp, ip]),
        "msfm_rectifier_create": (i, [vp, i, i, vpp]),
        "msfm_rectifier_rectify": (i, [vp, u8p, i, u8p, i, dp, dp, dp, dp, dp, dp, i, dp, dp, dp, dp, i64p]),
        "msfm_rectifier_fetch": (i, [vp, i, vp]),
        "msfm_rectifier_size": (i, [vp, ip, ip, i64p]),
        "msfm_rectifier_destroy": (None, [vp]),
        "msfm_sgm_execute_rectified": (i, [vp, vp, i64p]),
    }
    L = capi.lib()
    for name, (restype, argtypes) in want.items():
        assert capi.PROTOTYPES[name] == (restype, argtypes), name
        assert name in capi.SYMBOLS and hasattr(L, name), name
        assert getattr(L, name).restype is restype and list(getattr(L, name).argtypes) == argtypes, name
    assert hasattr(capi.Context, "rectifier") and capi.Rectifier._destroy == "msfm_rectifier_destroy"
    assert hasattr(capi.StereoSGM, "execute_rectified") and callable(capi.stereo_rectify)
    for name in ("epipolar_rectification", "sgm_dense_posed", "write_pose_file"):
        assert callable(getattr(dense, name)), name


def test_tables_say_what_the_header_says():
    text = header_text()
    assert "#define MSFM_RECTIFY_STATS %d" % len(A.RECTIFY_STATS) in text
    assert A.RECTIFY_STATS == A.SGM_STATS                      # "as MSFM_SGM_STATS"
    assert len(_header.struct_names(text)) == 25               # every new entry point takes plain arguments
    assert [k for k, _, _ in A.RECTIFY_FETCH] == list(range(6))
    # "kind 0 / 1 rectified left / right (uint8); 2 / 3 mapx / mapy of the left image, 4 / 5 of the right (float)"
    para = " ".join(re.search(r"msfm_rectifier_fetch waits and copies.*?\(float\)", text, flags=re.S).group(0).replace("*", " ").split())
    m = re.search(r"kind 0 / 1 rectified left / right \((\w+)\); 2 / 3 mapx / mapy of the left image, 4 / 5 of the right \((\w+)\)", para)
    assert m, para
    c_size = dict(uint8=1, float=4)
    sizes = [np.dtype(d).itemsize for _, _, d in A.RECTIFY_FETCH]
    assert sizes == [c_size[m.group(1)]] * 2 + [c_size[m.group(2)]] * 4
    assert [n for _, n, _ in A.RECTIFY_FETCH] == ["left", "right", "mapx_left", "mapy_left", "mapx_right", "mapy_right"]
    # the parameter block: the header's text, the library's constant and the binding's agree
    with open(os.path.join(ROOT, "metricsfm_amd", "csrc", "rectify_args.h")) as fh:
        args = fh.read()
    assert int(re.search(r"#define\s+RECT_PARAM_BYTES\s+(\d+)", args).group(1)) == A.RECTIFY_PARAM_BYTES == 2 * 13 * 8
    assert "= %d bytes)" % A.RECTIFY_PARAM_BYTES in text and "(%d + 2 w h)" % A.RECTIFY_PARAM_BYTES in text
    assert int(re.search(r"#define\s+RECT_FETCH_KINDS\s+(\d+)", args).group(1)) == len(A.RECTIFY_FETCH)


def test_null_handles_are_refused():
    L = capi.lib()
    INV = A.MSFM_E_INVAL
    st, img, out = np.full(len(A.RECTIFY_STATS), -1, np.int64), np.zeros((4, 64), np.uint8), np.full((4, 64), 7, np.uint8)
    K, R, t = np.eye(3), np.eye(3), np.array([-1.0, 0, 0])
    d = [A.ptr(a, A.c_double_p) for a in (K, R, np.zeros(3), K, R, t)]
    u8 = A.ptr(img, A.c_u8_p)
    w = C.c_int32(-3)
    assert L.msfm_rectifier_create(None, 64, 4, None) == INV
    assert L.msfm_rectifier_rectify(None, u8, 64, u8, 64, *d, 0, None, None, None, None, A.ptr(st, C.POINTER(C.c_int64))) == INV
    assert L.msfm_rectifier_fetch(None, 0, out.ctypes.data_as(C.c_void_p)) == INV
    assert L.msfm_rectifier_size(None, C.byref(w), None, None) == INV
    assert L.msfm_sgm_execute_rectified(None, None, A.ptr(st, C.POINTER(C.c_int64))) == INV
    L.msfm_rectifier_destroy(None)
    assert (st == -1).all() and (out == 7).all() and w.value == -3
