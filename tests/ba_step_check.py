"""The linear solve inside one Levenberg-Marquardt iteration, checked at any size.

An LM loop tolerates a wrong linear solve: a bad step is rejected, the radius shrinks and the cost still falls.  So the
solve itself is checked here, against the CPU oracle's reduced camera system S y = rhs (damped, Jacobi-scaled, at the
start parameters x0; oracle.ba_reduced_system): the camera step of an accepted first iteration, y = -(x1 - x0)_c / scale,
must have a small normwise backward error

    eta = |S y - rhs| / (|S|_F |y| + |rhs|)

with S symmetrised from its stored upper triangle.  That costs one Schur build and one n^2 mat-vec, where the oracle's
own factorisation is O(n^3).  Used by tests/test_step_check.py (the checker against known good and corrupted steps) and by
tests/test_gpu_ba_large.py (the GPU's step at sizes where the factorisation changes code paths).
"""
import numpy as np

from metricsfm_amd import _abi as A

# no stopping rule fires (negative tolerances): exactly the iterations asked for are run
NO_STOP = dict(function_tolerance=-1.0, gradient_tolerance=-1.0, parameter_tolerance=-1.0)

# Bar on eta.  Calibrated on the CPU (tests/test_step_check.py): the oracle's own first step gives eta = 2.9e-17 at n = 360
# (40 cameras with one model each, GPS rows) and 1.5e-17 at n = 3 003 (config 3's shape); one 64-column block of y scaled by
# 1 + 1e-6 gives 1.6e-9 .. 2.1e-8 at n = 360 and 5.7e-10 .. 9.4e-10 at n = 3 003, two blocks swapped 1e-3 .. 5e-2.  The bar
# leaves five decades for a GPU that assembles S in another order and three below the smallest corruption at n = 360.
STEP_BAR = 1e-12
# iteration 0 of the GPU against the oracle at the same x0: cost (sums over millions of rows in different orders) and
# the gradient's max-norm
COST_RTOL = 1e-12
GMAX_RTOL = 1e-10


def _mask(m, n):
    return np.ones(n, bool) if m is None else np.asarray(m) != 0


def reduced_blocks(arrays):
    """Cameras and intrinsics blocks that are parameters, in the order of the reduced columns (ba_setup in
    oracle/msfm_oracle.cpp: a block exists iff some residual uses it)."""
    a = arrays
    cm, mm = _mask(a.cam_mutable, len(a.cam_pose)), _mask(a.model_mutable, len(a.cam_model))
    pm = _mask(a.pt_mutable, len(a.point))
    use = cm[a.obs_cam] & (cm[a.obs_cam] | pm[a.obs_pt])
    cu = np.zeros(len(a.cam_pose), bool)
    cu[a.obs_cam[use]] = True
    if a.gps_xyz is not None:
        cu |= cm
    m = a.cam_model_of_cam[a.obs_cam[use]]
    mu = np.zeros(len(a.cam_model), bool)
    mu[m[mm[m]]] = True
    return cu, mu


def reduced_vector(arrays, cu, mu):
    return np.concatenate([arrays.cam_pose[cu].ravel(), arrays.cam_model[mu].ravel()])


def reference(oracle, arrays, radius=1e4):
    """The oracle's reduced system at the arrays' parameters, with the Jacobi scale of its columns."""
    opts = oracle.default_options(initial_trust_region_radius=radius)
    S, rhs, cost, gmax, scale = oracle.ba_reduced_system(arrays, radius=radius, options=opts, with_scale=True)
    cu, mu = reduced_blocks(arrays)
    assert len(rhs) == 6 * int(cu.sum()) + 3 * int(mu.sum())
    return dict(S=S, rhs=rhs, cost=cost, gmax=gmax, scale=scale, x0=reduced_vector(arrays, cu, mu), cu=cu, mu=mu)


def scaled_step(ref, arrays_after):
    """y of S y = rhs from the parameters after one accepted step: x1 = x0 - y * scale."""
    x1 = reduced_vector(arrays_after, ref["cu"], ref["mu"])
    return -(x1 - ref["x0"]) / ref["scale"]


def backward_error(S, y, rhs, rows=1024):
    """eta with S = triu(S) + triu(S, 1)^T, formed row block by row block (no second n x n array: S alone is 4.3 GB at
    n = 23 k).  Returns eta and the residual S y - rhs."""
    n = len(y)
    Sy = np.zeros(n)
    fro2 = 0.0
    for i0 in range(0, n, rows):
        i1 = min(n, i0 + rows)
        k = i1 - i0
        U = S[i0:i1, i0:].copy()                 # rows i0..i1 from the diagonal on
        U[:, :k][np.tril_indices(k, -1)] = 0.0   # (below the diagonal: not stored)
        d = U[np.arange(k), np.arange(k)].copy()
        Sy[i0:i1] += U @ y[i0:]
        Sy[i0:] += U.T @ y[i0:i1]                # the mirrored lower triangle ...
        Sy[i0:i1] -= d * y[i0:i1]                # ... without the diagonal twice
        fro2 += 2.0 * float(np.einsum("ij,ij->", U, U)) - float(d @ d)
    res = Sy - rhs
    eta = np.linalg.norm(res) / (np.sqrt(fro2) * np.linalg.norm(y) + np.linalg.norm(rhs))
    return float(eta), res


def worst_block(res, width=64):
    """(index, norm) of the 64-column block with the largest residual."""
    n = len(res)
    nb = -(-n // width)
    r = np.zeros(nb * width)
    r[:n] = res
    norms = np.sqrt((r.reshape(nb, width) ** 2).sum(1))
    b = int(np.argmax(norms))
    return b, float(norms[b])


def check_step(ref, y, bar):
    """Asserts eta <= bar; on failure names the 64-column block with the largest residual.  Returns eta."""
    eta, res = backward_error(ref["S"], y, ref["rhs"])
    if not eta <= bar:
        b, nb = worst_block(res)
        raise AssertionError("backward error %.3e > %.1e (n = %d): largest residual in columns %d..%d, norm %.3e of %.3e"
                             % (eta, bar, len(y), 64 * b, min(len(y), 64 * b + 64) - 1, nb, np.linalg.norm(res)))
    return eta


def oracle_step(oracle, make_arrays, radius=1e4, num_threads=1):
    """The oracle's own first LM iteration (stopping rules off): summary and the arrays after it."""
    a = make_arrays()
    r = oracle.ba_solve(a, oracle.default_options(max_num_iterations=1, num_threads=num_threads, initial_trust_region_radius=radius,
                                                  **NO_STOP))
    return r, a


def gpu_step(ctx, make_arrays, radius=1e4):
    """One GPU LM iteration (stopping rules off) on a resident problem: summary, layout (solve_paths of that iteration) and
    the arrays after it."""
    from metricsfm_amd import capi
    a = make_arrays()
    ba = ctx.ba(a)
    try:
        r = ba.run(capi.default_options(max_num_iterations=1, initial_trust_region_radius=radius, **NO_STOP))
        lay = ba.layout()
        a.cam_pose[:], a.cam_model[:], a.point[:] = ba.download()
    finally:
        ba.close()
    return r, lay, a


def step_arrays(sc, gps=True):
    """BaArrays of a scene, with the SLAMGPS rows (weight count1 / cams_.size(), integer division: slam_gps.cc:824)."""
    kw = dict(gps_xyz=sc.gps_xyz, gps_weight=float(sc.n_obs // sc.n_cams)) if gps and sc.gps_xyz is not None else {}
    return A.BaArrays.from_scene(sc, **kw)
