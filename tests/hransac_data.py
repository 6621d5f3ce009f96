"""Shared by the homography / SLAM-prior tests: the sequential CPU restatement tests/hransac_ref.cpp (compiled with g++ into
a temporary directory and loaded with ctypes) and synthetic correspondence sets."""
import ctypes as C
import os
import subprocess

import numpy as np

from metricsfm_amd import _abi as A

HERE = os.path.dirname(os.path.abspath(__file__))
SEED_H = 0x4D53464D48


def build_ref(tmpdir):
    so = os.path.join(str(tmpdir), "hransac_ref.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-o", so,
                           os.path.join(HERE, "hransac_ref.cpp")])
    L = C.CDLL(so)
    L.hr_homography_ransac_batch.argtypes = [C.c_int, A.c_int_p, A.c_float_p, A.c_float_p, C.c_double, C.c_double, C.c_int, C.c_int,
                                             C.c_uint64, A.c_double_p, A.c_u8_p, A.c_int_p, A.c_u8_p]
    L.hr_update_num_iters.argtypes = [C.c_double, C.c_double, C.c_int, C.c_int]
    return L


def ref_hransac(L, offsets, pt1, pt2, threshold=3.0, confidence=0.995, max_iterations=2000, polish=1, seed=SEED_H):
    offsets = np.ascontiguousarray(offsets, dtype=np.int32)
    pt1 = np.ascontiguousarray(np.asarray(pt1, dtype=np.float32).reshape(-1, 2))
    pt2 = np.ascontiguousarray(np.asarray(pt2, dtype=np.float32).reshape(-1, 2))
    n = len(offsets) - 1
    H = np.zeros((max(1, n), 3, 3)); inl = np.zeros(max(1, len(pt1)), np.uint8)
    nin = np.zeros(max(1, n), np.int32); ok = np.zeros(max(1, n), np.uint8)
    rc = L.hr_homography_ransac_batch(n, A.ptr(offsets, A.c_int_p), A.ptr(pt1, A.c_float_p), A.ptr(pt2, A.c_float_p), threshold,
                                      confidence, max_iterations, polish, seed, A.ptr(H, A.c_double_p), A.ptr(inl, A.c_u8_p),
                                      A.ptr(nin, A.c_int_p), A.ptr(ok, A.c_u8_p))
    assert rc == 0
    return H[:n], inl[:len(pt1)], nin[:n], ok[:n]


def random_H(rng):
    H = np.eye(3) + np.array([[rng.normal(0, 0.1), rng.normal(0, 0.1), rng.normal(0, 30)],
                              [rng.normal(0, 0.1), rng.normal(0, 0.1), rng.normal(0, 30)],
                              [rng.normal(0, 2e-5), rng.normal(0, 2e-5), 0.0]])
    return H / H[2, 2]


def apply_H(H, x):
    y = np.column_stack([x, np.ones(len(x))]) @ H.T
    return y[:, :2] / y[:, 2:3]


def make_pair(rng, N, outlier_frac, planar=True, noise=0.3):
    """N correspondences (float32) in centred pixels; planar: image 2 = H_true(image 1) + noise; otherwise two views of a
    scene with relief (depth 60 .. 140).  Returns pt1, pt2, H_true (planar) or None, true-inlier mask."""
    x1 = np.column_stack([rng.uniform(-900, 900, N), rng.uniform(-600, 600, N)])
    if planar:
        Ht = random_H(rng)
        x2 = apply_H(Ht, x1)
    else:
        Ht = None
        Z = rng.uniform(60, 140, N)
        X = np.column_stack([x1 * Z[:, None] / 1000.0, Z])
        t = np.array([8.0, 1.5, 2.0])
        Xc = X + t
        x2 = 1000.0 * Xc[:, :2] / Xc[:, 2:3]
    x2 = x2 + rng.normal(0, noise, x2.shape)
    good = np.ones(N, bool)
    n_out = int(round(outlier_frac * N))
    if n_out:
        idx = rng.choice(N, n_out, replace=False)
        x2[idx] = np.column_stack([rng.uniform(-900, 900, n_out), rng.uniform(-600, 600, n_out)])
        good[idx] = False
    return x1.astype(np.float32), x2.astype(np.float32), Ht, good


def batch(parts):
    """[(pt1, pt2), ...] -> offsets, pt1, pt2"""
    off = np.zeros(len(parts) + 1, np.int32)
    off[1:] = np.cumsum([len(a) for a, _ in parts])
    p1 = np.concatenate([a for a, _ in parts]) if parts else np.zeros((0, 2), np.float32)
    p2 = np.concatenate([b for _, b in parts]) if parts else np.zeros((0, 2), np.float32)
    return off, p1.astype(np.float32).reshape(-1, 2), p2.astype(np.float32).reshape(-1, 2)


def transfer_err32(H, p1, p2):
    """err = (float)(dx^2 + dy^2) of the transfer of p1 into image 2, as the kernels form it (binary64, then rounded)."""
    x, y = p1[:, 0].astype(np.float64), p1[:, 1].astype(np.float64)
    ww = 1.0 / (H[2, 0] * x + H[2, 1] * y + 1.0)
    dx = (H[0, 0] * x + H[0, 1] * y + H[0, 2]) * ww - p2[:, 0].astype(np.float64)
    dy = (H[1, 0] * x + H[1, 1] * y + H[1, 2]) * ww - p2[:, 1].astype(np.float64)
    return (dx * dx + dy * dy).astype(np.float32)
