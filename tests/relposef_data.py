"""Shared by the unknown-focal seed-pair tests: the sequential CPU restatement tests/relposef_ref.cpp (compiled with g++ into
a temporary directory and loaded with ctypes), synthetic pairs whose two focal lengths differ, and a numpy restatement of
the single-sample eight-point fit."""
import ctypes as C
import os
import subprocess

import numpy as np

from metricsfm_amd import _abi as A

HERE = os.path.dirname(os.path.abspath(__file__))
SEED_F8 = 0x4D53464D38
F_REF, F_CUR = 4800.0, 4200.0
# Hartley's formula is singular when the two optical axes are parallel or meet: the default second view is generic.
ROT_GENERIC = np.array([0.12, -0.35, 0.2])
CENTRE_GENERIC = np.array([38.0, -14.0, 9.0])


def build_ref(tmpdir):
    so = os.path.join(str(tmpdir), "relposef_ref.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-o", so,
                           os.path.join(HERE, "relposef_ref.cpp")])
    L = C.CDLL(so)
    dp, ip = A.c_double_p, A.c_int_p
    L.rf_relpose_8pt_batch.argtypes = [C.c_int, ip, dp, dp, C.c_int, C.c_uint64, dp, dp, dp, dp, dp, dp, A.c_u8_p, ip, dp, ip]
    L.rf_sample8.argtypes = [C.c_uint64, C.c_int, C.c_int, C.c_int, ip]
    L.rf_sample8.restype = None
    L.rf_fit.argtypes = [dp, dp, C.c_int, dp]
    L.rf_focal_from_F.argtypes = [dp, dp, dp, dp, dp]
    L.rf_pose_from_E.argtypes = [dp, C.c_int, dp, dp, C.c_double, C.c_double, dp, dp]
    L.rf_pose_from_E.restype = None
    return L


def _pts(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1, 2))


def ref_relpose_8pt(L, offsets, pts_ref, pts_cur, ransac_times=200, seed=SEED_F8):
    """-> (F, f_ref, f_cur, E, R, t, ok, best_iter, best_error, n_candidates), the order of Context.relpose_8pt"""
    offsets = np.ascontiguousarray(offsets, dtype=np.int32)
    pts_ref, pts_cur = _pts(pts_ref), _pts(pts_cur)
    n = len(offsets) - 1
    m = max(1, n)
    F = np.zeros((m, 3, 3)); E = np.zeros((m, 3, 3)); R = np.zeros((m, 3, 3)); t = np.zeros((m, 3))
    f1 = np.zeros(m); f2 = np.zeros(m); ok = np.zeros(m, np.uint8)
    bi = np.zeros(m, np.int32); be = np.zeros(m); nc = np.zeros(m, np.int32)
    dp = A.c_double_p
    rc = L.rf_relpose_8pt_batch(n, A.ptr(offsets, A.c_int_p), A.ptr(pts_ref, dp), A.ptr(pts_cur, dp), ransac_times, seed,
                                A.ptr(F, dp), A.ptr(f1, dp), A.ptr(f2, dp), A.ptr(E, dp), A.ptr(R, dp), A.ptr(t, dp),
                                A.ptr(ok, A.c_u8_p), A.ptr(bi, A.c_int_p), A.ptr(be, dp), A.ptr(nc, A.c_int_p))
    assert rc == 0
    return F[:n], f1[:n], f2[:n], E[:n], R[:n], t[:n], ok[:n], bi[:n], be[:n], nc[:n]


def ref_sample8(L, seed, problem, it, n):
    idx = np.zeros(8, np.int32)
    L.rf_sample8(seed, problem, it, n, A.ptr(idx, A.c_int_p))
    return idx


def ref_fit(L, x1, x2):
    x1, x2 = _pts(x1), _pts(x2)
    F = np.zeros((3, 3))
    good = L.rf_fit(A.ptr(x1, A.c_double_p), A.ptr(x2, A.c_double_p), len(x1), A.ptr(F, A.c_double_p))
    return bool(good), F


def ref_focal_from_F(L, F):
    """-> good, f1, f2, epipole1 (F e1 = 0), epipole2 (F^T e2 = 0)"""
    F = np.ascontiguousarray(F, dtype=np.float64)
    f1, f2 = np.zeros(1), np.zeros(1)
    e1, e2 = np.zeros(3), np.zeros(3)
    dp = A.c_double_p
    good = L.rf_focal_from_F(A.ptr(F, dp), A.ptr(f1, dp), A.ptr(f2, dp), A.ptr(e1, dp), A.ptr(e2, dp))
    return bool(good), f1[0], f2[0], e1, e2


def ref_pose_from_E(L, E, pts_ref, pts_cur, f1, f2):
    E = np.ascontiguousarray(E, dtype=np.float64)
    pts_ref, pts_cur = _pts(pts_ref), _pts(pts_cur)
    R, t = np.zeros((3, 3)), np.zeros(3)
    dp = A.c_double_p
    L.rf_pose_from_E(A.ptr(E, dp), len(pts_ref), A.ptr(pts_ref, dp), A.ptr(pts_cur, dp), f1, f2, A.ptr(R, dp), A.ptr(t, dp))
    return R, t


def rodrigues(a):
    th = np.linalg.norm(a)
    if th < 1e-12:
        return np.eye(3)
    k = a / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def make_pair(rng, n, noise=0.0, outlier_frac=0.0, f_ref=F_REF, f_cur=F_CUR, rot=ROT_GENERIC, centre=CENTRE_GENERIC, jitter=0.02):
    """n matches (float64 centred pixels) of a generic two-view scene: points as in twoview.make_relpose_batch, the second
    camera rotated by about `rot` (rad, axis-angle) with its centre at about `centre`.
    Returns x_ref, x_cur, R, t (X_cur = R X + t), X."""
    X = np.column_stack([rng.uniform(-40, 40, n), rng.uniform(-30, 30, n), rng.uniform(80, 120, n)])
    R = rodrigues(np.asarray(rot) + rng.normal(0, jitter, 3))
    c = np.asarray(centre) + rng.normal(0, 25 * jitter, 3)
    t = -R @ c
    x1 = f_ref * X[:, :2] / X[:, 2:3] + rng.normal(0, 1.0, (n, 2)) * noise
    Xc = X @ R.T + t
    x2 = f_cur * Xc[:, :2] / Xc[:, 2:3] + rng.normal(0, 1.0, (n, 2)) * noise
    nout = int(round(outlier_frac * n))
    if nout:
        bad = rng.choice(n, nout, replace=False)
        x2[bad] = np.column_stack([rng.uniform(-2000, 2000, nout), rng.uniform(-1500, 1500, nout)])
    return x1, x2, R, t, X


def batch(parts):
    """[(x_ref, x_cur), ...] -> offsets, x_ref, x_cur"""
    off = np.zeros(len(parts) + 1, np.int32)
    off[1:] = np.cumsum([len(a) for a, _ in parts])
    a = np.concatenate([np.asarray(p, dtype=np.float64).reshape(-1, 2) for p, _ in parts]) if parts else np.zeros((0, 2))
    b = np.concatenate([np.asarray(p, dtype=np.float64).reshape(-1, 2) for _, p in parts]) if parts else np.zeros((0, 2))
    return off, np.ascontiguousarray(a), np.ascontiguousarray(b)


MIXED_SIZES = [300, 0, 7, 8, 9, 15, 16, 2500, 60]


def make_mixed_batch(seed, sizes=MIXED_SIZES, noise=0.5):
    """Generic scenes with 0.5 px noise, 15 % outliers in every third pair, and the last pair pure uniform noise."""
    rng = np.random.default_rng(seed)
    parts = []
    for k, n in enumerate(sizes):
        if k == len(sizes) - 1:
            parts.append((np.column_stack([rng.uniform(-2000, 2000, n), rng.uniform(-1500, 1500, n)]),
                          np.column_stack([rng.uniform(-2000, 2000, n), rng.uniform(-1500, 1500, n)])))
            continue
        a, b, _, _, _ = make_pair(rng, n, noise=noise, outlier_frac=0.15 if k % 3 == 0 else 0.0)
        parts.append((a, b))
    return batch(parts)


def numpy_fit(x1, x2):
    """The normalised eight-point fit in numpy (LAPACK SVD nullspace, rank 2, denormalised); F with x2^T F x1 = 0."""
    def normalise(x):
        c = x.mean(axis=0)
        s = np.sqrt(2.0) / np.sqrt(((x - c) ** 2).sum() / len(x))
        T = np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1.0]])
        return (x - c) * s, T
    a, T1 = normalise(np.asarray(x1, dtype=np.float64))
    b, T2 = normalise(np.asarray(x2, dtype=np.float64))
    ah = np.column_stack([a, np.ones(len(a))])
    Acon = np.column_stack([ah * b[:, :1], ah * b[:, 1:2], ah])
    Fn = np.linalg.svd(Acon)[2][-1].reshape(3, 3)
    U, s, Vt = np.linalg.svd(Fn)
    s[2] = 0.0
    return T2.T @ (U @ np.diag(s) @ Vt) @ T1


def unit_F(F):
    """unit Frobenius norm, largest entry positive"""
    F = np.asarray(F, dtype=np.float64) / np.linalg.norm(F)
    k = np.argmax(np.abs(F))
    return F if F.flat[k] > 0 else -F
