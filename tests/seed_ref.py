"""Loader of tests/seed_ref.cpp, the sequential restatement of the seed-pair loop (sfm_incremental.cc:235-390), and the
literal Python loop of IncrementalSfM::SortImagePairs (:1790-1829) that metricsfm_amd/seed.py::sort_image_pairs is held to."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

from metricsfm_amd import _abi as A

HERE = os.path.dirname(os.path.abspath(__file__))
FETCHED = ("arm", "pose_ok", "pass", "n_matches", "f", "R", "t", "c", "pt_off", "pt_match", "X", "mse")   # + "winner"


def build_ref(tmpdir):
    so = os.path.join(str(tmpdir), "seed_ref.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "seed_ref.cpp")])
    L = C.CDLL(so)
    dp, ip, up, fp = A.c_double_p, A.c_int_p, A.c_u8_p, A.c_float_p
    L.sr_gather.argtypes = [C.c_int, ip, ip, ip, ip, fp, C.c_int, ip, ip, dp, dp]
    L.sr_reconstruct.argtypes = [C.c_int, ip, ip, ip, ip, fp, C.c_int, ip, dp, up, up, dp, dp, dp, C.c_double, C.c_double, C.c_int,
                                 up, up, up, ip, dp, dp, dp, dp, ip, ip, dp, dp, ip]
    return L


def _store(n_features, pairs, match_off, matches, keypoints):
    nf = np.ascontiguousarray(n_features, dtype=np.int32)
    fo = np.ascontiguousarray(np.concatenate([[0], np.cumsum(nf)]), dtype=np.int32)
    pr = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    mo = np.ascontiguousarray(match_off, dtype=np.int32)
    m = np.ascontiguousarray(np.asarray(matches, dtype=np.int32).reshape(-1, 2))
    kp = np.ascontiguousarray(np.asarray(keypoints, dtype=np.float32).reshape(-1, 2))
    assert len(kp) == fo[-1]
    return fo, pr, mo, m, kp


def gather(L, n_features, pairs, match_off, matches, keypoints, hyp_img):
    """-> n_matches [n], pts1, pts2 [sum][2] (float64) in hypothesis order: what the pose estimators are handed (:294-304)."""
    fo, pr, mo, m, kp = _store(n_features, pairs, match_off, matches, keypoints)
    hyp = np.ascontiguousarray(np.asarray(hyp_img, dtype=np.int32).reshape(-1, 2))
    n = len(hyp)
    nm = np.zeros(max(1, n), np.int32)
    args = [len(pr), A.ptr(pr, A.c_int_p), A.ptr(mo, A.c_int_p), A.ptr(m, A.c_int_p), A.ptr(fo, A.c_int_p), A.ptr(kp, A.c_float_p), n,
            A.ptr(hyp, A.c_int_p), A.ptr(nm, A.c_int_p)]
    assert L.sr_gather(*args, None, None) == 0
    total = int(nm[:n].sum())
    p1, p2 = np.zeros((max(1, total), 2)), np.zeros((max(1, total), 2))
    assert L.sr_gather(*args, A.ptr(p1, A.c_double_p), A.ptr(p2, A.c_double_p)) == 0
    return nm[:n], p1[:total], p2[:total]


def reconstruct(L, n_features, pairs, match_off, matches, keypoints, hyp_img, cam_fk, same_model, pose_ok, R, t, f8,
                th_mse_reprojection=3.0, th_angle_small=3.0 / 180.0 * 3.1415, th_seedpair_structures=20):
    """The dict `Context.seed_hypotheses` returns (without h2d_bytes), from the restatement; poses as input."""
    fo, pr, mo, m, kp = _store(n_features, pairs, match_off, matches, keypoints)
    hyp = np.ascontiguousarray(np.asarray(hyp_img, dtype=np.int32).reshape(-1, 2))
    n = len(hyp)
    k = max(1, n)
    fk = np.ascontiguousarray(np.asarray(cam_fk, dtype=np.float64).reshape(-1, 2, 3))
    same = np.ascontiguousarray(np.asarray(same_model, dtype=np.uint8).reshape(-1))
    pok = np.ascontiguousarray(pose_ok, dtype=np.uint8)
    Rin, tin, fin = (np.ascontiguousarray(x, dtype=np.float64) for x in (R, t, f8))
    nm, _, _ = gather(L, n_features, pairs, match_off, matches, keypoints, hyp)
    cap = max(1, int(nm.sum()))
    o = dict(arm=np.zeros(k, np.uint8), pose_ok=np.zeros(k, np.uint8), **{"pass": np.zeros(k, np.uint8)}, n_matches=np.zeros(k, np.int32),
             f=np.zeros((k, 2)), R=np.zeros((k, 3, 3)), t=np.zeros((k, 3)), c=np.zeros((k, 3)), pt_off=np.zeros(n + 1, np.int32),
             pt_match=np.zeros(cap, np.int32), X=np.zeros((cap, 3)), mse=np.zeros(cap))
    win = np.zeros(1, np.int32)
    dp, ip, up = A.c_double_p, A.c_int_p, A.c_u8_p
    rc = L.sr_reconstruct(len(pr), A.ptr(pr, ip), A.ptr(mo, ip), A.ptr(m, ip), A.ptr(fo, ip), A.ptr(kp, A.c_float_p), n, A.ptr(hyp, ip),
                          A.ptr(fk, dp), A.ptr(same, up), A.ptr(pok, up), A.ptr(Rin, dp), A.ptr(tin, dp), A.ptr(fin, dp),
                          th_mse_reprojection, th_angle_small, th_seedpair_structures,
                          A.ptr(o["arm"], up), A.ptr(o["pose_ok"], up), A.ptr(o["pass"], up), A.ptr(o["n_matches"], ip), A.ptr(o["f"], dp),
                          A.ptr(o["R"], dp), A.ptr(o["t"], dp), A.ptr(o["c"], dp), A.ptr(o["pt_off"], ip), A.ptr(o["pt_match"], ip),
                          A.ptr(o["X"], dp), A.ptr(o["mse"], dp), A.ptr(win, ip))
    assert rc == 0
    npt = int(o["pt_off"][n])
    for key in ("arm", "pose_ok", "pass", "n_matches", "f", "R", "t", "c"):
        o[key] = o[key][:n]
    for key in ("pt_match", "X", "mse"):
        o[key] = o[key][:npt]
    o["winner"] = int(win[0])
    return o


def sort_image_pairs_loop(match_graph, processed):
    """SortImagePairs :1790-1829 line by line, with struct-packed binary32 values instead of numpy scalars; ties (which
    std::sort leaves open) to the lower i * n + j."""
    import struct

    def f32(x):
        return struct.unpack("f", struct.pack("f", x))[0]

    g = [[int(v) for v in row] for row in match_graph]
    n = len(g)
    strength = []
    for i in range(n):
        s = 0.0
        for j in range(n):
            s = f32(s + f32(float(g[i][j])))           # math::sum: T sum += data[i]
        strength.append(f32(math.log(s + 2.0)))        # :1797, the float promoted to double by the 2.0
    pairs = []
    for i in range(n - 1):
        if processed[i]:
            continue
        for j in range(i + 1, n):
            if not g[i][j] or processed[j]:
                continue
            strength_ij = f32(strength[i] * strength[j]) * math.log(float(g[i][j]))   # :1817: float * float, then double
            pairs.append((i * n + j, f32(strength_ij)))                              # :1818: stored as float
    pairs.sort(key=lambda p: p[0])
    pairs.sort(key=lambda p: p[1], reverse=True)       # stable: equal strengths keep the ascending key
    return [(k // n, k % n) for k, _ in pairs]
