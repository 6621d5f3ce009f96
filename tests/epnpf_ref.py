"""CPU reference of the focal sweep (AbsolutePoseEstimation::AbsolutePoseWithoutFocalLength, absolute_pose_estimation.cc:28-40
-> AbsolutePoseEPNPF::EPNPF, absolute_pose_via_epnpf.cc:34-63), composed from the oracle's pieces:

  * step i of image p is problem p * n_steps + i of `oracle.epnp_ransac` at f_i = (f_ratio_min + i * f_ratio_step) * f_init[p]
    (:49); the expanded batch is given that index by leading empty problems;
  * the step's error is the kept sample's error over its own four points (EPNPRansac's `error`, absolute_pose_via_epnp.cc:129-133),
    which the batch call does not return: the kept sample's indices are recomputed with `sample4` below, a restatement of
    pose::sample (oracle/pose_oracle.cpp:38-57), and `oracle._test_epnp4` solves those four points again - its R, t must be
    the batch's, bit for bit, or the restated sampler is wrong;
  * then the sequential loop of :46-62: error = 1000000.0, step i is taken if error_i < error.
"""
import numpy as np

M64 = (1 << 64) - 1
EPNP_SALT = 0x45506E50


def num_steps(f_ratio_min, f_ratio_max, f_ratio_step):
    return int((f_ratio_max - f_ratio_min) / f_ratio_step)   # int num_sample = ... :44, in binary64


def _sm64(s):
    s = (s + 0x9E3779B97F4A7C15) & M64
    z = s
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return s, z ^ (z >> 31)


def sample4(seed, problem, it, n):
    """The four distinct indices of [0, n) of sample `it` of problem `problem` (splitmix64 stream, duplicates redrawn)."""
    s = (seed ^ EPNP_SALT ^ ((problem * 0xD1342543DE82EF95) & M64) ^ ((it * 0xA24BAED4963EE407) & M64)) & M64
    idx = []
    while len(idx) < 4:
        s, z = _sm64(s)
        v = int(z % n)
        if v not in idx:
            idx.append(v)
    return idx


def epnpf_sweep(O, offsets, pts_w, pts_2d, f_init, f_ratio_min=0.5, f_ratio_max=4.0, f_ratio_step=0.01, max_iter=200,
                seed=0x4D53464D50):
    """Returns f [n], R [n,3,3], t [n,3], errors [total], avg_error [n], best_step [n], best_iter [n], step_error [n, n_steps]
    - the tuple Context.epnpf_sweep(..., keep_step_errors=True) returns."""
    offsets = np.asarray(offsets, dtype=np.int32)
    pts_w = np.asarray(pts_w, dtype=np.float64).reshape(-1, 3)
    pts_2d = np.asarray(pts_2d, dtype=np.float64).reshape(-1, 2)
    n = len(offsets) - 1
    f_init = np.broadcast_to(np.asarray(f_init, dtype=np.float64), (n,))
    S = num_steps(f_ratio_min, f_ratio_max, f_ratio_step)
    f = np.zeros(n); R = np.zeros((n, 3, 3)); t = np.zeros((n, 3)); errors = np.zeros(len(pts_w)); avg = np.zeros(n)
    best_step = np.zeros(n, np.int32); best_iter = np.zeros(n, np.int32); step_error = np.zeros((n, S))
    for p in range(n):
        o, N = int(offsets[p]), int(offsets[p + 1] - offsets[p])
        X, x = pts_w[o:o + N], pts_2d[o:o + N]
        fs = np.array([(f_ratio_min + i * f_ratio_step) * float(f_init[p]) for i in range(S)])   # :49
        off = np.concatenate([np.zeros(p * S, np.int64), np.arange(S + 1) * N]).astype(np.int32)
        ff = np.concatenate([np.ones(p * S), fs])
        Rs, ts, es, avgs, its = O.epnp_ransac(off, np.tile(X, (S, 1)), np.tile(x, (S, 1)), ff, max_iter=max_iter, seed=seed)
        Rs, ts, avgs, its, es = Rs[p * S:], ts[p * S:], avgs[p * S:], its[p * S:], es.reshape(S, N)
        for i in range(S):
            if its[i] < 0:
                step_error[p, i] = 1e9   # EPNPRansac's starting value: no sample ran
                continue
            idx = sample4(seed, p * S + i, int(its[i]), N)
            R4, t4, e4 = O._test_epnp4(X[idx], x[idx], fs[i])
            assert np.array_equal(R4, Rs[i], equal_nan=True) and np.array_equal(t4, ts[i], equal_nan=True), (p, i, idx)
            step_error[p, i] = e4
        error, b = 1000000.0, -1   # :46
        for i in range(S):
            if step_error[p, i] < error:   # :56
                error, b = step_error[p, i], i
        best_step[p] = b
        if b >= 0:
            f[p], R[p], t[p], errors[o:o + N], avg[p], best_iter[p] = fs[b], Rs[b], ts[b], es[b], avgs[b], its[b]
        else:   # nothing taken: the pose stays as constructed, Error (:35) runs on it at the untouched f
            f[p], best_iter[p] = f_init[p], -1
            R0, t0, e0, a0, _ = O.epnp_ransac(np.array([0, min(N, 3)], np.int32), X[:3], x[:3], f_init[p], max_iter=max_iter, seed=seed)
            assert N < 4
            R[p], t[p], errors[o:o + N], avg[p] = R0[0], t0[0], e0[:N], a0[0]
    return f, R, t, errors, avg, best_step, best_iter, step_error
