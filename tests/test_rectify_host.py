"""Stereo rectification without a device: the two restatements (tests/rectify_ref.cpp, tests/rectify_ref.py) agree to the bit on
every case, msfm_stereo_rectify (host only, no context) equals them to the bit, the closed-form cases give what their formulas
say, the rectified cameras have the epipolar property, every refusal leaves the outputs untouched, and the pose file round-trips."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from metricsfm_amd import _abi as A
from metricsfm_amd import capi, dense
from tests import rectify_data as D
from tests import rectify_ref as P

GEOMETRY = (("R_left", "R1"), ("R_right", "R2"), ("P_left", "P1"), ("P_right", "P2"), ("Q", "Q"))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("shape_name", D.SHAPES)
@pytest.mark.parametrize("case", D.CASES)
def test_the_restatements_agree(case, shape_name):
    cpp, py = D.expected(case, shape_name), D.expected_py(case, shape_name)
    assert cpp is not None and py is not None
    assert cpp["idx"] == py["idx"]
    for k in ("R1", "R2", "P1", "P2", "Q", "t_rect") + D.MAPS:
        assert same_bits(cpp[k], py[k]), k
    for k in ("left", "right"):
        assert np.array_equal(cpp[k], py[k]), k


@pytest.mark.parametrize("shape_name", D.SHAPES)
@pytest.mark.parametrize("case", D.CASES)
def test_stereo_rectify_equals_the_restatement(case, shape_name):
    w, h = D.shape(shape_name)
    want = D.expected(case, shape_name)
    got = capi.stereo_rectify(*D.pose_list(D.poses(case, w, h)), w, h)
    assert got["idx"] == want["idx"]
    for mine, theirs in GEOMETRY:
        assert same_bits(got[mine], want[theirs]), (mine, got[mine], want[theirs])


@pytest.mark.parametrize("shape_name", D.SHAPES)
@pytest.mark.parametrize("case", D.CLOSED + ("huge",))
def test_closed_forms(case, shape_name):
    """What the formulas of rectify_data.closed_form give, with neither restatement's warp involved."""
    left, right = D.pair(shape_name)
    want, got = D.closed_form(case, left, right), D.expected(case, shape_name)
    assert np.array_equal(got["R1"], np.eye(3)) and np.array_equal(got["R2"], np.eye(3)) and got["idx"] == 0
    for k in ("left", "right", "mapx_left", "mapx_right"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["mapy_left"], want["mapy"]) and np.array_equal(got["mapy_right"], want["mapy"])
    if case in ("identity", "tie"):
        assert np.array_equal(got["left"], left) and np.array_equal(got["right"], right)
    if case == "tie":   # the tie is one: half away from zero would have taken the neighbour's 1/32
        assert np.array_equal(got["mapx_left"].astype(np.float64) * 32 % 1, np.full(left.shape, 0.5))
        away = D.shifted(left, 1)
        assert not np.array_equal((31 * left.astype(np.int64) + away + 16) >> 5, left)
    if case == "half":  # the one case with an ix = -1 tap (right image, column 0) and an ix = w - 1 tap (left image, last column)
        assert np.array_equal(got["left"][:, -1], (left[:, -1].astype(np.int64) + 1) >> 1)
        assert np.array_equal(got["right"][:, 0], (right[:, 0].astype(np.int64) + 1) >> 1)
    if case == "huge":
        assert got["left"].any() == bool(left.shape[1] % 2)


def test_case_properties():
    """What the issue's cases are there for: camera 1 is the left one in the convergent cases, the vertical case is one, and the
    two convergent variants between them meet every source border with partly covered pixels, in both images."""
    for shape_name in ("odd64", "odd128", "grid128"):
        met = D.border_coverage(shape_name)
        assert all(len(v) == 4 for v in met.values())
    for case in ("convergent", "convergent_mirrored"):
        g = D.expected(case, "odd64")
        assert g["idx"] == 0 and g["P2"][0, 3] < 0
    v = D.expected("vertical", "odd64")
    assert v["idx"] == 1 and v["P2"][1, 3] != 0 and v["P2"][0, 3] == 0


@pytest.mark.parametrize("case", ["convergent", "convergent_mirrored", "vertical", "half"])
def test_epipolar_property(case):
    """Independent of all three restatements: 200 world points in front of both cameras, projected through K [R | t] and then
    through Pk_ Rk_ Kk^-1, land on rows (columns when idx == 1) that differ by less than 1e-8 pixel.  The bound is binary64
    roundoff, 2e-16, times coordinates of 1e3, times a few hundred operations, with a wide margin; and t_rect has only its idx
    component, to 1e-12 of its length."""
    w, h = D.shape("odd64")
    p = D.poses(case, w, h)
    g = capi.stereo_rectify(*D.pose_list(p), w, h)
    rng = np.random.default_rng(11)
    Xc1 = np.column_stack([rng.uniform(-2, 2, 200), rng.uniform(-2, 2, 200), rng.uniform(6, 12, 200)])   # in camera 1's frame
    Xw = (np.linalg.inv(p["R1"]) @ (Xc1 - p["t1"]).T).T
    coords = []
    for K, R, t, Pk, Rk in ((p["K1"], p["R1"], p["t1"], g["P_left"], g["R_left"]), (p["K2"], p["R2"], p["t2"], g["P_right"], g["R_right"])):
        xc = (R @ Xw.T).T + t
        assert (xc[:, 2] > 1).all()
        pix = (K @ xc.T).T
        pix = pix / pix[:, 2:3]
        q = (Pk[:, :3] @ Rk @ np.linalg.inv(K) @ pix.T).T
        coords.append(q[:, :2] / q[:, 2:3])
    other = g["idx"] ^ 1
    gap = np.abs(coords[0][:, other] - coords[1][:, other]).max()
    print("%s: largest gap across the epipolar lines %.3g pixel" % (case, gap))
    assert gap < 1e-8
    # and along them the disparity is what P_right's fourth column says: d = -P_right[idx][3] / z_rectified
    R21 = p["R2"] @ np.linalg.inv(p["R1"])
    t21 = -R21 @ p["t1"] + p["t2"]
    trect = g["R_right"] @ t21
    rest = np.delete(trect, g["idx"])
    print("%s: t_rect %s" % (case, trect))
    assert np.abs(rest).max() <= 1e-12 * np.linalg.norm(trect)
    assert abs(g["P_right"][g["idx"], 3] - trect[g["idx"]] * g["P_left"][0, 0]) <= 1e-12 * abs(g["P_right"][g["idx"], 3])
    assert abs(g["Q"][3, 2] + 1.0 / trect[g["idx"]]) <= 1e-12 * abs(g["Q"][3, 2])


def test_every_refusal_leaves_the_outputs_untouched():
    L = capi.lib()
    w, h = D.shape("odd64")
    good = D.pose_list(D.poses("convergent", w, h))
    outs = [np.full(n, 7.5) for n in (9, 9, 12, 12, 16)]
    idx = C.c_int32(-3)

    def call(args, width=w, height=h):
        ptrs = [None if a is None else A.ptr(a, A.c_double_p) for a in args]
        return L.msfm_stereo_rectify(*ptrs, width, height, *[A.ptr(o, A.c_double_p) for o in outs], C.byref(idx))

    def changed(k, fn):
        args = [a.copy() for a in good]
        fn(args[k])
        return args
    bad = []
    for k in range(6):                                                  # a NULL input, a non-finite value, each array in turn
        bad.append(good[:k] + [None] + good[k + 1:])
        for v in (np.nan, np.inf, -np.inf):
            bad.append(changed(k, lambda a, v=v: a.__setitem__((-1,) if a.ndim == 1 else (1, 1), v)))
    for k in (0, 3):                                                    # a focal length that is not positive
        for pos in ((0, 0), (1, 1)):
            for v in (0.0, -250.0):
                bad.append(changed(k, lambda a, pos=pos, v=v: a.__setitem__(pos, v)))
    same = [a.copy() for a in good]                                     # no baseline: both cameras at one centre
    same[5] = same[4] @ np.linalg.inv(same[1]) @ same[2]
    bad.append(same)
    turn = [a.copy() for a in good]                                     # a half turn about y, and one 1e-7 short of it
    turn[4] = np.diag([-1.0, 1.0, -1.0]) @ turn[1]
    bad.append(turn)
    near = [a.copy() for a in good]
    near[4] = D.rot(0, np.pi - 1e-7, 0) @ near[1]
    bad.append(near)
    singular = [a.copy() for a in good]                                 # an R1 without an inverse
    singular[1] = np.zeros((3, 3))
    bad.append(singular)
    for args in bad:
        assert call(args) == A.MSFM_E_INVAL
    for width, height in ((0, h), (w, 0), (16385, h), (w, 16385), (-1, -1)):
        assert call(good, width, height) == A.MSFM_E_INVAL
    assert all((o == 7.5).all() for o in outs) and idx.value == -3
    with pytest.raises(capi.MsfmError):
        capi.stereo_rectify(*turn, w, h)
    for args in bad:                                                    # the Python restatement refuses the same poses
        if all(a is not None for a in args):
            assert P.geometry(*args, w, h) is None
    # the limits themselves are accepted, every output is optional, and a turn of pi - 1e-5 is fine
    assert call(good, 16384, 16384) == 0 and call(good, 1, 1) == 0
    far = [a.copy() for a in good]
    far[4] = D.rot(0, np.pi - 1e-5, 0) @ far[1]
    assert call(far) == 0
    ptrs = [A.ptr(a, A.c_double_p) for a in good]
    assert L.msfm_stereo_rectify(*ptrs, w, h, None, None, None, None, None, None) == 0
    assert idx.value in (0, 1) and not (outs[0] == 7.5).any()


def test_host_checks_and_blend(tmp_path):
    """rectify_args.h compiled as plain C++: the size and stride refusals as include/msfm.h lists them, the fetch kinds, and the
    blend on taps inside, on each border and outside, against the formula written out."""
    src = tmp_path / "t.cpp"
    src.write_text('#include "rectify_args.h"\nint main() {\n'
                   '  if (!rect_check_size(1, 1).empty() || !rect_check_size(16384, 16384).empty()) return 1;\n'
                   '  if (rect_check_size(0, 5).empty() || rect_check_size(5, 0).empty() || rect_check_size(16385, 5).empty()) return 1;\n'
                   '  if (rect_check_size(5, 16385).empty() || rect_check_size(-1, 5).empty()) return 1;\n'
                   '  int z = 0;\n'
                   '  if (!rect_check_pair(&z, 64, &z, 70, 64).empty() || rect_check_pair(nullptr, 64, &z, 64, 64).empty()) return 2;\n'
                   '  if (rect_check_pair(&z, 64, nullptr, 64, 64).empty() || rect_check_pair(&z, 63, &z, 64, 64).empty()) return 2;\n'
                   '  if (rect_check_pair(&z, 64, &z, 63, 64).empty()) return 2;\n'
                   '  if (rect_fetch_item(0) != 1 || rect_fetch_item(1) != 1 || rect_fetch_item(2) != 4 || rect_fetch_item(5) != 4) return 3;\n'
                   '  if (rect_fetch_item(-1) || rect_fetch_item(6) || RECT_STATS != 3 || sizeof(RectParams) != RECT_PARAM_BYTES) return 3;\n'
                   '  const uint8_t img[6] = {10, 20, 30, 40, 50, 60};   // 3 x 2\n'
                   '  if (rect_blend(img, 3, 2, 32, 0) != 20 || rect_blend(img, 3, 2, 64, 32) != 60) return 4;\n'
                   '  if (rect_blend(img, 3, 2, 5, 7) != ((27 * 25 * 10 + 5 * 25 * 20 + 27 * 7 * 40 + 5 * 7 * 50 + 512) >> 10)) return 4;\n'
                   '  if (rect_blend(img, 3, 2, -16, 0) != ((16 * 32 * 10 + 512) >> 10) || rect_blend(img, 3, 2, 64 + 16, 0) != 15) return 5;\n'
                   '  if (rect_blend(img, 3, 2, 0, -16) != 5 || rect_blend(img, 3, 2, 0, 32 + 16) != 20) return 5;\n'
                   '  if (rect_blend(img, 3, 2, -32, 0) != 0 || rect_blend(img, 3, 2, 96, 0) != 0 || rect_blend(img, 3, 2, 0, 64) != 0) return 6;\n'
                   '  if (rect_blend(img, 3, 2, -(1 << 30) + 1, (1 << 30) - 1) != 0 || rect_blend(img, 3, 2, (1 << 30) - 1, -(1 << 30) + 1) != 0) return 6;\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "t"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(D.ROOT, "metricsfm_amd", "csrc"),
                           str(src), "-o", str(exe)])
    assert subprocess.run([str(exe)]).returncode == 0


def test_pose_file_round_trip(tmp_path):
    rng = np.random.default_rng(5)
    n = 3
    Ks = np.stack([np.array([[900.0 + rng.uniform(0, 50), 0, 640 + rng.normal()], [0, 880.0 + rng.uniform(0, 50), 360 + rng.normal()], [0, 0, 1]])
                   for _ in range(n)])
    Rs = np.stack([D.rot(*rng.normal(0, 0.3, 3)) for _ in range(n)])
    ts = rng.normal(0, 20, (n, 3))
    names, sizes = ["a_%d.jpg" % i for i in range(n)], [(1280, 720)] * n
    path = tmp_path / "sfm_sure.txt"
    dense.write_pose_file(str(path), names, sizes, Ks, ts, Rs)
    got = dense.read_pose_file(str(path))
    assert got["names"] == names and got["sizes"].tolist() == [[1280, 720]] * n
    assert not got["dist"].any()
    for key, want in (("Ks", Ks), ("ts", ts), ("Rs", Rs)):
        assert np.abs(got[key] - want).max() <= 0.5e-8 + 1e-12, key      # the 8 decimals written (and the last bit of a value near 1e3)
    with open(path) as fh:
        head = fh.readlines()[:8]
    assert head[0].split() == ["fileName", "imageWidth", "imageHeight"] and head[7].strip() == "" and "P = K [R|-Rt] X" in head[6]
