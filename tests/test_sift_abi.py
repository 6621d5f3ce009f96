"""The scale-space and describe exports without a device: the prototypes the binding reads from include/msfm.h are the ones
written here by hand, the library has the symbols, and null handles are refused."""
import ctypes as C

from metricsfm_amd import _abi as A
from metricsfm_amd import capi


def test_prototypes_read_from_the_header():
    vp, i, P = C.c_void_p, C.c_int, C.POINTER
    fp, ip, up, i64p = A.c_float_p, A.c_int_p, A.c_u8_p, C.POINTER(C.c_int64)
    want = {
        "msfm_scalespace_create": (i, [vp, up, i, i, i, i, i, P(vp)]),
        "msfm_scalespace_fetch": (i, [vp, i, i, i, fp]),
        "msfm_scalespace_size": (i, [vp, i, ip, ip, i64p]),
        "msfm_scalespace_destroy": (None, [vp]),
        "msfm_descset_describe": (i, [vp, i, vp, fp, i, i, i64p]),
        "msfm_descset_fetch": (i, [vp, i, fp, fp]),
    }
    L = capi.lib()
    for name, (restype, argtypes) in want.items():
        assert capi.PROTOTYPES[name] == (restype, argtypes), name
        assert name in capi.SYMBOLS and hasattr(L, name), name
        assert getattr(L, name).restype is restype and list(getattr(L, name).argtypes) == argtypes, name


def test_null_handles_are_refused():
    L = capi.lib()
    out = C.c_void_p()
    assert L.msfm_scalespace_create(None, None, 8, 8, 8, 1, 1, C.byref(out)) == A.MSFM_E_INVAL
    assert L.msfm_scalespace_fetch(None, 0, 0, 0, None) == A.MSFM_E_INVAL
    assert L.msfm_scalespace_size(None, 0, None, None, None) == A.MSFM_E_INVAL
    assert L.msfm_descset_describe(None, 0, None, None, 0, 0, None) == A.MSFM_E_INVAL
    assert L.msfm_descset_fetch(None, 0, None, None) == A.MSFM_E_INVAL
    L.msfm_scalespace_destroy(None)
    assert not out.value
