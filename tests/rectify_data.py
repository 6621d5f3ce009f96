"""The cases of the stereo-rectification tests and the C++ restatement (tests/rectify_ref.cpp) run on them once per process: built
with g++ into a temporary directory, fed one binary file, its results read back read-only and shared by every test that needs them.
The shapes are those of four dense-stereo cases (tests/sgm_data.py), so a rectified pair can go on through tests/sgm_ref.cpp."""
import functools
import math
import os
import subprocess
import tempfile

import numpy as np

from tests import rectify_ref as P
from tests import sgm_data as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ("odd64", "flat64", "odd128", "grid128")            # 83 x 37 (odd width), 64 x 5, 150 x 21, 272 x 64
CLOSED = ("identity", "tie", "ax2", "half")
CASES = CLOSED + ("convergent", "convergent_mirrored", "vertical", "huge")
MAPS = ("mapx_left", "mapy_left", "mapx_right", "mapy_right")
BASELINE = 0.25


def shape(name):
    """-> (w, h) of a shape, named as the dense-stereo case it is taken from"""
    return X.CASES[name][1], X.CASES[name][2]


def rot(ax, ay, az):
    """Rz(az) Ry(ay) Rx(ax), binary64"""
    cx, sx, cy, sy, cz, sz = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay), math.cos(az), math.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def poses(case, w, h):
    """-> dict(K1, R1, t1, K2, R2, t2); camera 1 is the left image.  x_camera = R x_world + t.
    The closed-form cases: K = [256 0 cx; 0 256 (h - 1) / 2; 0 0 1] for both cameras with cx = (w - 1) / 2 (41 and 18 at 83 x 37)
    but for camera 1's offset, R = I, t21 along -x.  Every intermediate of the header's arithmetic is exact there: R1_ = R2_ = I,
    cc.x = (cx1 + cx2) / 2, mapx = j - cc.x + cx_k, mapy = i."""
    cx, cy = (w - 1) * 0.5, (h - 1) * 0.5
    I, zero = np.eye(3), np.zeros(3)

    def K(fx, fy, x0, y0):
        return np.array([[fx, 0, x0], [0, fy, y0], [0, 0, 1]], np.float64)
    if case in CLOSED or case == "huge":
        dx1 = dict(identity=0.0, tie=1.0 / 32, ax2=3.0 / 32, half=1.0, huge=0.0)[case]
        fx, fy = (1e10, 1.0) if case == "huge" else (256.0, 256.0)
        return dict(K1=K(fx, fy, cx + dx1, cy), R1=I, t1=zero, K2=K(fx, fy, cx, cy), R2=I, t2=np.array([-BASELINE, 0, 0]))
    if case in ("convergent", "convergent_mirrored"):
        s = 1.0 if case == "convergent" else -1.0
        R1, R2 = rot(s * 0.11, s * -0.09, s * 0.10), rot(s * 0.09, s * 0.12, s * -0.09)
        c2 = np.array([1.0, 0.06, -0.04])      # camera 2's centre; camera 1 sits at the origin, to its left
        return dict(K1=K(262.0, 249.0, cx + 1.5, cy - 0.75), R1=R1, t1=zero, K2=K(247.0, 258.0, cx - 2.25, cy + 1.25), R2=R2, t2=-R2 @ c2)
    if case == "vertical":
        R1, R2 = rot(0.05, -0.04, 0.06), rot(-0.04, 0.05, -0.03)
        c2 = np.array([0.08, 1.0, 0.05])
        return dict(K1=K(262.0, 249.0, cx + 1.5, cy - 0.75), R1=R1, t1=zero, K2=K(247.0, 258.0, cx - 2.25, cy + 1.25), R2=R2, t2=-R2 @ c2)
    raise KeyError(case)


def pose_list(p):
    return [np.ascontiguousarray(p[k], np.float64) for k in ("K1", "R1", "t1", "K2", "R2", "t2")]


def pair(shape_name):
    """The images of a shape: the dense-stereo case's pair, left and right (read-only)."""
    return X.case_pair(shape_name)


@functools.lru_cache(maxsize=None)
def ref_exe():
    exe = os.path.join(tempfile.mkdtemp(prefix="rectify_ref_"), "rectify_ref")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", os.path.join(ROOT, "tests", "rectify_ref.cpp"), "-o", exe])
    return exe


def run_ref_cpp(left, right, p):
    """-> dict(idx, R1, R2, P1, P2, Q, t_rect, the four maps, left, right, seconds), arrays read-only; None where it refuses"""
    left, right = np.ascontiguousarray(left, np.uint8), np.ascontiguousarray(right, np.uint8)
    h, w = left.shape
    tmp = tempfile.mkdtemp(prefix="rectify_io_")
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as fh:
        np.array([w, h], np.int32).tofile(fh)
        for a in pose_list(p):
            a.tofile(fh)
        left.tofile(fh)
        right.tofile(fh)
    try:
        out = subprocess.run([ref_exe(), fin, fout], capture_output=True, text=True)
        assert out.returncode == 0 and "rectify_ref ok" in out.stdout, out.stdout + out.stderr
        with open(fout, "rb") as fh:
            if np.fromfile(fh, np.int32, 1)[0]:
                return None
            got = dict(idx=int(np.fromfile(fh, np.int32, 1)[0]))
            for name, shp in (("R1", (3, 3)), ("R2", (3, 3)), ("P1", (3, 4)), ("P2", (3, 4)), ("Q", (4, 4)), ("t_rect", (3,))):
                got[name] = np.fromfile(fh, np.float64, int(np.prod(shp))).reshape(shp)
            for name in MAPS:
                got[name] = np.fromfile(fh, np.float32, h * w).reshape(h, w)
            for name in ("left", "right"):
                got[name] = np.fromfile(fh, np.uint8, h * w).reshape(h, w)
    finally:
        for f in (fin, fout):
            if os.path.exists(f):
                os.remove(f)
        os.rmdir(tmp)
    for a in got.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    got["seconds"] = float(out.stdout.split(",")[1].split()[0])
    return got


@functools.lru_cache(maxsize=None)
def expected(case, shape_name):
    """The C++ restatement's result for a case at a shape, computed once and shared."""
    w, h = shape(shape_name)
    return run_ref_cpp(*pair(shape_name), poses(case, w, h))


@functools.lru_cache(maxsize=None)
def expected_py(case, shape_name):
    """The Python restatement's result for a case at a shape, computed once and shared."""
    w, h = shape(shape_name)
    return P.run(*pair(shape_name), *pose_list(poses(case, w, h)))


def shifted(img, dx):
    """q[j] = img[j + dx] along the rows, 0 outside, as int64"""
    h, w = img.shape
    q = np.zeros((h, w), np.int64)
    if dx >= 0:
        q[:, :w - dx] = img[:, dx:]
    else:
        q[:, -dx:] = img[:, :w + dx]
    return q


def closed_form(case, left, right):
    """-> dict(left, right uint8 [h][w], mapx_left, mapx_right, mapy float32 [h][w]) of a closed-form case or of `huge`, from the
    formulas, with no restatement involved.  mapx = j - cc.x + cx_k with cc.x the mean of the two cx, so left is shifted by
    +d / 2 and right by -d / 2 for an offset d of camera 1's cx:
      identity  d = 0: copies.
      tie       d = 1/32: 32 mapx = 32 j +- 1/2, exactly halfway; half to even gives 32 j, copies.
      ax2       d = 3/32: left 32 mapx = 32 j + 3/2 -> 32 j + 2 (even), ax = 2: ((30 p[j] + 2 p[j + 1]) * 32 + 512) >> 10;
                right 32 j - 3/2 -> 32 j - 2: ix = j - 1, ax = 30: ((2 p[j - 1] + 30 p[j]) * 32 + 512) >> 10.
      half      d = 1: ax = 16 on both sides, (p[j] + p[j + 1] + 1) >> 1 left and (p[j - 1] + p[j] + 1) >> 1 right.
      huge      fx = 1e10, fy = 1: mapx = 1e10 (j - cx) + cx, which the 2^30 rule turns to 0 unless j = cx (an odd width)."""
    h, w = left.shape
    j, i = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    L, R, Lp, Rm = left.astype(np.int64), right.astype(np.int64), shifted(left, 1), shifted(right, -1)
    d = dict(identity=0.0, tie=1.0 / 32, ax2=3.0 / 32, half=1.0, huge=0.0)[case]
    out = dict(mapx_left=(j + d / 2).astype(np.float32), mapx_right=(j - d / 2).astype(np.float32), mapy=i.astype(np.float32))
    if case in ("identity", "tie"):
        out["left"], out["right"] = L, R
    elif case == "ax2":
        out["left"], out["right"] = ((30 * L + 2 * Lp) * 32 + 512) >> 10, ((2 * Rm + 30 * R) * 32 + 512) >> 10
    elif case == "half":
        out["left"], out["right"] = (L + Lp + 1) >> 1, (Rm + R + 1) >> 1
    elif case == "huge":
        keep = np.zeros((h, w), bool)
        if w % 2:
            keep[:, (w - 1) // 2] = True
        out["left"], out["right"] = np.where(keep, L, 0), np.where(keep, R, 0)
        cx = (w - 1) * 0.5
        with np.errstate(all="ignore"):
            out["mapx_left"] = out["mapx_right"] = (1e10 * (j - cx) + cx).astype(np.float32)
    else:
        raise KeyError(case)
    out["left"], out["right"] = out["left"].astype(np.uint8), out["right"].astype(np.uint8)
    return out


@functools.lru_cache(maxsize=None)
def border_coverage(shape_name="odd64"):
    """From the Python restatement, over the two convergent variants: per image the set of source borders ('left', 'right', 'top',
    'bottom') at which some output pixel has some but not all of its four taps inside.  Asserts that every border is met for both
    images, and that each image of each variant has pixels with all four taps inside and pixels with none."""
    w, h = shape(shape_name)
    met = dict(left=set(), right=set())
    for case in ("convergent", "convergent_mirrored"):
        r = expected_py(case, shape_name)
        for side in ("left", "right"):
            t = r["taps_" + side]
            part = (t["taps"] > 0) & (t["taps"] < 4)
            for name, hit in (("left", t["ix"] == -1), ("right", t["ix"] == w - 1), ("top", t["iy"] == -1), ("bottom", t["iy"] == h - 1)):
                if (part & hit).any():
                    met[side].add(name)
            assert (t["taps"] == 4).any() and (t["taps"] == 0).any(), (case, side)
    for side in ("left", "right"):
        assert met[side] == {"left", "right", "top", "bottom"}, (shape_name, side, met[side])
    return met
