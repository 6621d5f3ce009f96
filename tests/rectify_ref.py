"""A second opinion on tests/rectify_ref.cpp: include/msfm.h, "Stereo rectification", restated in Python.  The geometry is scalar
Python floats (binary64, one rounding per operation, `math` for the host C library's acos, sin, cos and sqrt); maps and warp are
numpy element-wise operations, which round one by one as well.  Nothing here uses a matrix product of numpy."""
import math

import numpy as np


def _dot3(a0, b0, a1, b1, a2, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def _mat(a):
    return [[float(v) for v in row] for row in np.asarray(a, np.float64).reshape(3, 3)]


def _mm(A, B):
    return [[_dot3(A[i][0], B[0][j], A[i][1], B[1][j], A[i][2], B[2][j]) for j in range(3)] for i in range(3)]


def _mv(A, v):
    return [_dot3(A[i][0], v[0], A[i][1], v[1], A[i][2], v[2]) for i in range(3)]


def _norm(v):
    return math.sqrt(_dot3(v[0], v[0], v[1], v[1], v[2], v[2]))


def _div(a, b):
    """IEEE division of two finite binary64 values (Python raises where C gives an infinity or a NaN)."""
    return float(np.float64(a) / np.float64(b))


def _inv(a):
    c = [[a[1][1] * a[2][2] - a[1][2] * a[2][1], a[0][2] * a[2][1] - a[0][1] * a[2][2], a[0][1] * a[1][2] - a[0][2] * a[1][1]],
         [a[1][2] * a[2][0] - a[1][0] * a[2][2], a[0][0] * a[2][2] - a[0][2] * a[2][0], a[0][2] * a[1][0] - a[0][0] * a[1][2]],
         [a[1][0] * a[2][1] - a[1][1] * a[2][0], a[0][1] * a[2][0] - a[0][0] * a[2][1], a[0][0] * a[1][1] - a[0][1] * a[1][0]]]
    det = _dot3(a[0][0], c[0][0], a[0][1], c[1][0], a[0][2], c[2][0])
    with np.errstate(all="ignore"):
        return [[_div(c[i][j], det) for j in range(3)] for i in range(3)]


def _rodrigues(v):
    R = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    th = _norm(v)
    if th == 0:
        return R
    c, s = math.cos(th), math.sin(th)
    c1 = 1.0 - c
    k = [v[0] / th, v[1] / th, v[2] / th]
    skew = [[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]]
    return [[(c * R[i][j] + (c1 * k[i]) * k[j]) + s * skew[i][j] for j in range(3)] for i in range(3)]


def _finite(*arrays):
    return all(np.isfinite(np.asarray(a, np.float64)).all() for a in arrays)


def geometry(K1, R1, t1, K2, R2, t2, w, h):
    """-> dict(R1, R2 [3][3], P1, P2 [3][4], Q [4][4], t_rect [3], idx), or None where the header says MSFM_E_INVAL"""
    if not (1 <= w <= 16384 and 1 <= h <= 16384) or not _finite(K1, R1, t1, K2, R2, t2):
        return None
    K1, R1, K2, R2 = _mat(K1), _mat(R1), _mat(K2), _mat(R2)
    t1, t2 = [float(v) for v in np.ravel(t1)], [float(v) for v in np.ravel(t2)]
    if not (K1[0][0] > 0 and K1[1][1] > 0 and K2[0][0] > 0 and K2[1][1] > 0):
        return None
    R21 = _mm(R2, _inv(R1))
    if not _finite(R21):
        return None
    rt = _mv(R21, t1)
    t21 = [-rt[i] + t2[i] for i in range(3)]
    if not _finite(t21):
        return None
    c = (((R21[0][0] + R21[1][1]) + R21[2][2]) - 1.0) * 0.5
    c = min(1.0, max(-1.0, c))
    theta = math.acos(c)
    if math.pi - theta < 1e-6:
        return None
    r = [(R21[2][1] - R21[1][2]) * 0.5, (R21[0][2] - R21[2][0]) * 0.5, (R21[1][0] - R21[0][1]) * 0.5]
    s = _norm(r)
    om = [0.0, 0.0, 0.0] if s == 0 else [ri * (theta / s) for ri in r]
    rr = _rodrigues([-0.5 * v for v in om])
    t = _mv(rr, t21)
    idx = 0 if abs(t[0]) > abs(t[1]) else 1
    cidx, nt = t[idx], _norm(t)
    if not nt > 0:
        return None
    uu = [0.0, 0.0, 0.0]
    uu[idx] = 1.0 if cidx > 0 else -1.0
    ww = [t[1] * uu[2] - t[2] * uu[1], t[2] * uu[0] - t[0] * uu[2], t[0] * uu[1] - t[1] * uu[0]]
    nw = _norm(ww)
    if nw > 0:
        f = math.acos(abs(cidx) / nt) / nw
        ww = [v * f for v in ww]
    wR = _rodrigues(ww)
    rrT = [[rr[j][i] for j in range(3)] for i in range(3)]
    R1_, R2_ = _mm(wR, rrT), _mm(wR, rr)
    trect = _mv(R2_, t21)
    o = idx ^ 1
    fc = min(K1[o][o], K2[o][o])
    cc = []
    with np.errstate(all="ignore"):
        for K, R in ((K1, R1_), (K2, R2_)):
            sx = sy = 0.0
            for x, y in ((0.0, 0.0), (float(w - 1), 0.0), (0.0, float(h - 1)), (float(w - 1), float(h - 1))):
                p = _mv(R, [(x - K[0][2]) / K[0][0], (y - K[1][2]) / K[1][1], 1.0])
                sx = sx + _div(p[0], p[2]) * fc
                sy = sy + _div(p[1], p[2]) * fc
            cc.append(((w - 1) * 0.5 - sx * 0.25, (h - 1) * 0.5 - sy * 0.25))
        ccx, ccy = (cc[0][0] + cc[1][0]) * 0.5, (cc[0][1] + cc[1][1]) * 0.5
        P1 = np.array([[fc, 0, ccx, 0], [0, fc, ccy, 0], [0, 0, 1, 0]], np.float64)
        P2 = P1.copy()
        P2[idx, 3] = trect[idx] * fc
        Q = np.array([[1, 0, 0, -ccx], [0, 1, 0, -ccy], [0, 0, 0, fc], [0, 0, -_div(1.0, trect[idx]), 0]], np.float64)
    g = dict(R1=np.array(R1_), R2=np.array(R2_), P1=P1, P2=P2, Q=Q, t_rect=np.array(trect), idx=idx)
    return g if _finite(g["R1"], g["R2"], P1, P2, Q) else None


def maps(P, R, K, w, h):
    """-> (mapx, mapy) float32 [h][w] of one camera"""
    K = _mat(K)
    iR = _inv(_mm(_mat(np.asarray(P)[:, :3]), _mat(R)))
    j, i = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    f = np.float64
    with np.errstate(all="ignore"):
        X = (f(iR[0][0]) * j + f(iR[0][1]) * i) + f(iR[0][2])
        Y = (f(iR[1][0]) * j + f(iR[1][1]) * i) + f(iR[1][2])
        W = (f(iR[2][0]) * j + f(iR[2][1]) * i) + f(iR[2][2])
        wi = f(1.0) / W
        mapx = (f(K[0][0]) * (X * wi) + f(K[0][2])).astype(np.float32)
        mapy = (f(K[1][1]) * (Y * wi) + f(K[1][2])).astype(np.float32)
    return mapx, mapy


def warp(src, mapx, mapy):
    """-> (out uint8 [h][w], dict(taps [h][w]: how many of the pixel's four taps lie inside the source, 0 where the 2^30 rule
    applies; ix, iy [h][w]: the first tap's column and row))"""
    src = np.asarray(src, np.uint8)
    h, w = src.shape
    with np.errstate(all="ignore"):
        px, py = mapx * np.float32(32.0), mapy * np.float32(32.0)
        ok = np.isfinite(px) & np.isfinite(py) & (np.abs(px) < np.float32(2.0 ** 30)) & (np.abs(py) < np.float32(2.0 ** 30))
    sx = np.rint(np.where(ok, px, 0)).astype(np.int64)
    sy = np.rint(np.where(ok, py, 0)).astype(np.int64)
    ix, iy, ax, ay = sx >> 5, sy >> 5, sx & 31, sy & 31
    big = src.astype(np.int64)
    S = np.zeros((h, w), np.int64)
    taps = np.zeros((h, w), np.int64)
    for dx, dy, wt in ((0, 0, (32 - ax) * (32 - ay)), (1, 0, ax * (32 - ay)), (0, 1, (32 - ax) * ay), (1, 1, ax * ay)):
        x, y = ix + dx, iy + dy
        inside = ok & (x >= 0) & (x < w) & (y >= 0) & (y < h)
        S += np.where(inside, wt * big[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)], 0)
        taps += inside
    return np.where(ok, (S + 512) >> 10, 0).astype(np.uint8), dict(taps=taps, ix=ix, iy=iy)


def run(left, right, K1, R1, t1, K2, R2, t2):
    """-> the dict of `geometry` with mapx_left, mapy_left, mapx_right, mapy_right, left, right, and taps_left, taps_right (the
    dicts of `warp`); None if refused"""
    h, w = np.asarray(left).shape
    g = geometry(K1, R1, t1, K2, R2, t2, w, h)
    if g is None:
        return None
    g["mapx_left"], g["mapy_left"] = maps(g["P1"], g["R1"], K1, w, h)
    g["mapx_right"], g["mapy_right"] = maps(g["P2"], g["R2"], K2, w, h)
    g["left"], g["taps_left"] = warp(left, g["mapx_left"], g["mapy_left"])
    g["right"], g["taps_right"] = warp(right, g["mapx_right"], g["mapy_right"])
    return g
