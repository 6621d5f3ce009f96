"""The dense-stereo exports without a device: the prototypes the binding reads from include/msfm.h are the ones written here by hand,
the library has the symbols, null handles are refused, the host side of metricsfm_amd/csrc/sgm_args.h does what the header says,
and dense.read_pose_file reads a file written here."""
import ctypes as C
import os
import subprocess

import numpy as np

from metricsfm_amd import _abi as A
from metricsfm_amd import _header, capi, dense
from tests import sgm_data as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_prototypes_read_from_the_header():
    vp, vpp, i, f, d = C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_float, C.c_double
    ip, i64p, u8p = A.c_int_p, C.POINTER(C.c_int64), A.c_u8_p
    want = {
        "msfm_sgm_create": (i, [vp, i, i, i, i, i, f, vpp]),
        "msfm_sgm_execute": (i, [vp, u8p, i, u8p, i, i64p]),
        "msfm_sgm_fetch": (i, [vp, i, i, vp]),
        "msfm_sgm_depth": (i, [vp, d, d, u8p]),
        "msfm_sgm_size": (i, [vp, ip, ip, ip, i64p]),
        "msfm_sgm_destroy": (None, [vp]),
    }
    L = capi.lib()
    for name, (restype, argtypes) in want.items():
        assert capi.PROTOTYPES[name] == (restype, argtypes), name
        assert name in capi.SYMBOLS and hasattr(L, name), name
        assert getattr(L, name).restype is restype and list(getattr(L, name).argtypes) == argtypes, name
    assert hasattr(capi.Context, "stereo_sgm") and capi.StereoSGM._destroy == "msfm_sgm_destroy"


def test_stats_length_and_struct_count():
    with open(_header.HEADER) as fh:
        text = fh.read()
    assert "#define MSFM_SGM_STATS %d" % len(A.SGM_STATS) in text
    assert len(_header.struct_names(text)) == 25   # every new entry point takes plain arguments
    assert [k for k, _, _ in A.SGM_FETCH] == list(range(8))
    assert (A.SGM_LANE_DISP, A.SGM_PATH_THREADS, A.SGM_WTA_TILE) == X.launch_constants()


def test_null_handles_are_refused():
    L = capi.lib()
    st, img, out = np.full(len(A.SGM_STATS), -1, np.int64), np.zeros((4, 64), np.uint8), np.full((4, 64), 7, np.uint8)
    w = C.c_int32(-3)
    assert L.msfm_sgm_create(None, 64, 4, 64, 10, 120, 0.96, None) == A.MSFM_E_INVAL
    assert L.msfm_sgm_execute(None, A.ptr(img, A.c_u8_p), 64, A.ptr(img, A.c_u8_p), 64, A.ptr(st, C.POINTER(C.c_int64))) == A.MSFM_E_INVAL
    assert L.msfm_sgm_fetch(None, 7, 0, out.ctypes.data_as(C.c_void_p)) == A.MSFM_E_INVAL
    assert L.msfm_sgm_depth(None, 1.0, 1.0, A.ptr(out, A.c_u8_p)) == A.MSFM_E_INVAL
    assert L.msfm_sgm_size(None, C.byref(w), None, None, None) == A.MSFM_E_INVAL
    L.msfm_sgm_destroy(None)
    assert (st == -1).all() and (out == 7).all() and w.value == -3


def test_host_rules_and_checks(tmp_path):
    """sgm_args.h compiled as plain C++: the refusals of create and execute as include/msfm.h lists them, the median network
    against a sort on every 0/1 pattern (a network that sorts those sorts everything) and on random values, the winner's rule,
    the depth table."""
    src = tmp_path / "t.cpp"
    src.write_text('#include "sgm_args.h"\n#include <algorithm>\n#include <cstdlib>\nint main() {\n'
                   '  if (!sgm_check_create(64, 1, 64, 10, 120, 0.96f).empty() || !sgm_check_create(16384, 16384, 128, 0, 0, 0.f).empty()) return 1;\n'
                   '  if (!sgm_check_create(128, 5, 128, 224, 224, 1.f).empty()) return 1;\n'
                   '  if (sgm_check_create(64, 5, 96, 10, 120, 0.96f).empty() || sgm_check_create(127, 5, 128, 10, 120, 0.96f).empty()) return 2;\n'
                   '  if (sgm_check_create(16385, 5, 64, 10, 120, 0.96f).empty() || sgm_check_create(64, 0, 64, 10, 120, 0.96f).empty()) return 2;\n'
                   '  if (sgm_check_create(64, 16385, 64, 10, 120, 0.96f).empty()) return 2;\n'
                   '  if (sgm_check_create(64, 5, 64, 10, 225, 0.96f).empty() || sgm_check_create(64, 5, 64, 121, 120, 0.96f).empty()) return 3;\n'
                   '  if (sgm_check_create(64, 5, 64, -1, 120, 0.96f).empty() || sgm_check_create(64, 5, 64, -2, -1, 0.96f).empty()) return 3;\n'
                   '  if (sgm_check_create(64, 5, 64, 10, 120, NAN).empty() || sgm_check_create(64, 5, 64, 10, 120, 1.5f).empty()) return 4;\n'
                   '  if (sgm_check_create(64, 5, 64, 10, 120, -0.1f).empty() || sgm_check_create(64, 5, 64, 10, 120, INFINITY).empty()) return 4;\n'
                   '  int z = 0;\n'
                   '  if (!sgm_check_execute(&z, 64, &z, 70, 64).empty() || sgm_check_execute(nullptr, 64, &z, 64, 64).empty()) return 5;\n'
                   '  if (sgm_check_execute(&z, 64, nullptr, 64, 64).empty() || sgm_check_execute(&z, 63, &z, 64, 64).empty()) return 5;\n'
                   '  if (sgm_check_execute(&z, 64, &z, 63, 64).empty()) return 5;\n'
                   '  for (int bits = 0; bits < 512; bits++) {\n'
                   '    int p[9], n = 0;\n'
                   '    for (int i = 0; i < 9; i++) { p[i] = (bits >> i) & 1; n += p[i]; }\n'
                   '    if (sgm_median9(p) != (n >= 5)) return 6;\n'
                   '  }\n'
                   '  srand(5);\n'
                   '  for (int t = 0; t < 2000; t++) {\n'
                   '    int p[9], s[9];\n'
                   '    for (int i = 0; i < 9; i++) p[i] = s[i] = rand() % 130;\n'
                   '    std::sort(s, s + 9);\n'
                   '    if (sgm_median9(p) != s[4]) return 7;\n'
                   '  }\n'
                   '  uint32_t k0 = 0xffffffffu, k1 = 0xffffffffu;\n'
                   '  const uint32_t keys[5] = {(9u << 16) | 0, (7u << 16) | 1, (30u << 16) | 2, (7u << 16) | 3, (8u << 16) | 4};\n'
                   '  for (int i = 0; i < 5; i++) sgm_two_smallest(keys[i], k0, k1);\n'
                   '  if (k0 != ((7u << 16) | 1) || k1 != ((7u << 16) | 3)) return 8;\n'
                   '  if (sgm_decide(k0, k1, 0.96f) != 0 || sgm_decide(k0, k1, 1.0f) != 1 || sgm_decide(k0, (7u << 16) | 2, 0.5f) != 1) return 9;\n'
                   '  if (sgm_decide((5u << 16) | 9, 0xffffffffu, 0.96f) != 9 || sgm_decide((5u << 16) | 9, 0xffffffffu, 0.f) != 0) return 9;\n'
                   '  uint8_t tab[128];\n'
                   '  sgm_depth_table(0.05, 300.0, tab);\n'
                   '  if (tab[0] != 0 || tab[11] != 0 || tab[12] != (uint8_t)(((200.0 * 0.05) * 300.0) / 12.0) || tab[127] != 23) return 10;\n'
                   '  sgm_depth_table(-0.05, 300.0, tab);\n'
                   '  for (int d = 0; d < 128; d++) if (tab[d]) return 11;\n'
                   '  if (sgm_fetch_item(2, 128) != 128 || sgm_fetch_item(0, 64) != 4 || sgm_fetch_item(6, 64) != 2 || sgm_fetch_item(7, 64) != 1) return 12;\n'
                   '  if (sgm_fetch_item(8, 64) || sgm_fetch_item(-1, 64) || SGM_STATS != 3) return 12;\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "t"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "metricsfm_amd", "csrc"), str(src), "-o", str(exe)])
    assert subprocess.run([str(exe)]).returncode == 0


def test_read_pose_file(tmp_path):
    rng = np.random.default_rng(3)
    n = 3
    Ks, ts, Rs, dist = rng.uniform(1, 900, (n, 3, 3)), rng.normal(0, 5, (n, 3)), rng.normal(0, 1, (n, 3, 3)), rng.normal(0, 0.1, (n, 5))
    path = tmp_path / "sfm_sure.txt"
    with open(path, "w") as fh:
        for i in range(8):
            fh.write("header line %d with 1 2 3 numbers\n" % i)
        for i in range(n):
            fh.write("img_%02d.jpg %d %d\n" % (i, 640 + i, 480 - i))
            fh.write(" ".join(repr(float(v)) for v in Ks[i].ravel()) + "\n")
            fh.write(" ".join(repr(float(v)) for v in dist[i]) + "\n")
            fh.write(" ".join(repr(float(v)) for v in ts[i]) + "\n")
            fh.write(" ".join(repr(float(v)) for v in Rs[i].ravel()) + "\n")
        fh.write("\n")
    got = dense.read_pose_file(str(path))
    assert got["names"] == ["img_00.jpg", "img_01.jpg", "img_02.jpg"]
    assert got["sizes"].tolist() == [[640, 480], [641, 479], [642, 478]]
    for key, want in (("Ks", Ks), ("ts", ts), ("Rs", Rs), ("dist", dist)):
        assert np.array_equal(got[key], want), key


def test_epipolar_poses():
    """R_new = R R_left keeps the camera centre: -R_new^T t_new = -R^-1 t for a rotation."""
    rng = np.random.default_rng(4)
    Rs = np.stack([np.linalg.qr(rng.normal(0, 1, (3, 3)))[0] for _ in range(3)])
    ts = rng.normal(0, 3, (3, 3))
    Rl = [np.linalg.qr(rng.normal(0, 1, (3, 3)))[0] for _ in range(2)]
    Rn, tn = dense.epipolar_poses(Rs, ts, Rl)
    assert not Rn[0].any() and not tn[0].any()
    for i in (1, 2):
        assert np.allclose(Rn[i], Rs[i] @ Rl[i - 1])
        assert np.allclose(-np.linalg.inv(Rn[i]) @ tn[i], -np.linalg.inv(Rs[i]) @ ts[i])
