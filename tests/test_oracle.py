"""CPU tests of the oracle itself (the checker must be right before it checks anything):
known answers, the dual-number evaluation, an independent dense LM, and the committed goldens."""
import os

import numpy as np
import pytest

from metricsfm_amd import _abi as A
from metricsfm_amd import scene

GOLD = os.path.join(os.path.dirname(__file__), "golden")

SEED_C1_HARD = 77


def test_rotation_known_answers(oracle):
    # 90 degrees about z: x -> y (basic_funcs.cc:118-158 / :160-225)
    aa = np.array([0, 0, np.pi / 2])
    np.testing.assert_allclose(oracle.rotate_point(aa, [1, 0, 0]), [0, 1, 0], atol=1e-15)
    np.testing.assert_allclose(oracle.angle_axis_to_R(aa) @ [1, 0, 0], [0, 1, 0], atol=1e-15)
    # small-angle branch (theta^2 <= DBL_EPSILON): R = I + [w]x exactly
    w = np.array([1e-9, -2e-9, 3e-9])
    R = oracle.angle_axis_to_R(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    assert (R == np.eye(3) + K).all()
    np.testing.assert_array_equal(oracle.rotate_point(w, [1, 2, 3]), np.array([1, 2, 3]) + np.cross(w, [1, 2, 3]))
    # round trip through the quaternion path, incl. theta near pi (trace < 0 branch)
    rng = np.random.default_rng(0)
    for _ in range(200):
        a = rng.standard_normal(3)
        a *= rng.uniform(0.01, np.pi - 1e-3) / np.linalg.norm(a)
        np.testing.assert_allclose(oracle.R_to_angle_axis(oracle.angle_axis_to_R(a)), a, atol=1e-9)
        np.testing.assert_allclose(scene.angle_axis_to_R(a), oracle.angle_axis_to_R(a), atol=1e-15)


def test_residual_known_answers(oracle):
    cam = np.array([4800.0, 0, 0])
    # identity pose, point on the optical axis: prediction (0,0), r = -w * obs exactly
    r, J = oracle.reproj(np.zeros(6), cam, [0, 0, 10.0], [3.0, 4.0], 2.0)
    assert (r == [-6.0, -8.0]).all()
    assert J[0, 3] == 2.0 * 4800 / 10 and J[1, 4] == 2.0 * 4800 / 10  # d u / d tx = w f / z
    # +z forward, NO sign flip despite the comment at reprojection_error_pose_cam_xyz.h:48-50
    r, _ = oracle.reproj(np.zeros(6), cam, [1.0, 2.0, 10.0], [0, 0], 1.0)
    np.testing.assert_allclose(r, [480.0, 960.0], rtol=1e-15)
    # radial distortion: d = 1 + r2 (k1 + k2 r2)
    r, _ = oracle.reproj(np.zeros(6), [100.0, 0.1, 0.01], [1.0, 0.0, 1.0], [0, 0], 1.0)
    np.testing.assert_allclose(r, [100 * (1 + 0.1 + 0.01), 0.0], rtol=1e-15)
    # pure translation
    r, _ = oracle.reproj([0, 0, 0, 1.0, -1.0, 5.0], cam, [0, 0, 5.0], [0, 0], 1.0)
    np.testing.assert_allclose(r, [480.0, -480.0], rtol=1e-15)


def test_jacobian_analytic_matches_jets(oracle):
    """Closed-form derivatives (what the HIP kernel evaluates) == forward-mode duals of the functor
    (what ceres::AutoDiffCostFunction evaluates), incl. the small-angle branch at 0 and at eps."""
    rng = np.random.default_rng(1)
    for scale in (0.0, 1e-9, 1.4e-8, 1.6e-8, 0.05, 1.0, 3.1):
        for _ in range(50):
            aa = rng.standard_normal(3)
            aa = aa / np.linalg.norm(aa) * scale
            pose = np.concatenate([aa, rng.standard_normal(3) * 5])
            cam = np.array([4800 + rng.standard_normal() * 100, rng.standard_normal() * 1e-2, rng.standard_normal() * 1e-3])
            X = rng.standard_normal(3) * 10 + [0, 0, 60]
            obs = rng.standard_normal(2) * 500
            r1, J1 = oracle.reproj(pose, cam, X, obs, 1.7)
            r2, J2 = oracle.reproj(pose, cam, X, obs, 1.7, dual=True)
            np.testing.assert_allclose(r1, r2, rtol=1e-13, atol=1e-9)
            np.testing.assert_allclose(J1, J2, rtol=1e-10, atol=1e-7 * np.abs(J2).max())


def test_huber(oracle):
    assert (oracle.huber(1.0, 0.25) == [0.25, 1.0, 0.0]).all()
    rho = oracle.huber(1.0, 4.0)  # 2 a sqrt(s) - a^2 = 3 ; a / sqrt(s) = 0.5 ; -rho' / (2 s)
    np.testing.assert_allclose(rho, [3.0, 0.5, -0.0625])
    assert (oracle.huber(1.0, 1.0) == [1.0, 1.0, 0.0]).all()  # s == b is still the quadratic branch


def test_lm_against_independent_dense_solver(oracle):
    """Same LM, no Schur complement, finite-difference Jacobian, scipy Cholesky."""
    from tests.independent_lm import DenseLM
    sc = scene.make_ring_scene(4, 24, seed=7, rot_sigma=0.02, trans_sigma=0.2, point_sigma=0.2)
    arr = A.BaArrays.from_scene(sc)
    res = oracle.ba_solve(arr, oracle.default_options(max_num_iterations=6, function_tolerance=-1.0,
                                                      parameter_tolerance=-1.0, gradient_tolerance=-1.0))
    x, traj = DenseLM(sc).run(6)
    np.testing.assert_allclose(res["iterations"]["cost"], traj, rtol=2e-6)
    # nothing fixes the 7-DoF gauge (sfm_incremental.cc:1016-1026), so parameters are compared through
    # the gauge-invariant predictions; the finite-difference Jacobian limits this to ~1e-4 px
    p, m, X = DenseLM(sc).split(x)
    uv_o, _ = scene.project(arr.cam_pose[sc.obs_cam], arr.cam_model[sc.cam_model_of_cam[sc.obs_cam]], arr.point[sc.obs_pt])
    uv_d, _ = scene.project(p[sc.obs_cam], m[sc.cam_model_of_cam[sc.obs_cam]], X[sc.obs_pt])
    assert np.abs(uv_o - uv_d).max() < 2e-3


def test_lm_converges_to_noise_floor(oracle):
    sc = scene.config_scene(1)
    arr = A.BaArrays.from_scene(sc)
    res = oracle.ba_solve(arr, oracle.default_options(max_num_iterations=50))
    assert res["termination"] == "CONVERGENCE_FUNCTION"
    uv, _ = scene.project(arr.cam_pose[sc.obs_cam], arr.cam_model[sc.cam_model_of_cam[sc.obs_cam]], arr.point[sc.obs_pt])
    e = np.linalg.norm(uv - sc.obs_xy, axis=1)
    assert 0.4 < e.mean() < 0.8  # 0.5 px noise per axis
    assert res["num_residuals"] == 2 * sc.n_obs and res["num_reduced_params"] == 63


def test_lm_reduced_system_is_schur_complement(oracle):
    """S and rhs from the eliminator == dense J^T J Schur complement computed with numpy."""
    from tests.independent_lm import DenseLM
    sc = scene.make_ring_scene(3, 10, seed=3, rot_sigma=0.01, trans_sigma=0.1, point_sigma=0.1)
    arr = A.BaArrays.from_scene(sc)
    S, rhs, cost, gmax = oracle.ba_reduced_system(arr, radius=1e4)
    lm = DenseLM(sc)
    r, J = lm.corrected(lm.x)
    scale = 1.0 / (1.0 + np.sqrt((J * J).sum(0)))
    J = J * scale
    D2 = np.sqrt(np.clip((J * J).sum(0), 1e-6, 1e32) / 1e4) ** 2
    H, g = J.T @ J + np.diag(D2), J.T @ r
    nf = 6 * 3 + 3
    Sd = H[:nf, :nf] - H[:nf, nf:] @ np.linalg.solve(H[nf:, nf:], H[nf:, :nf])
    gd = g[:nf] - H[:nf, nf:] @ np.linalg.solve(H[nf:, nf:], g[nf:])
    Su = np.triu(S)
    np.testing.assert_allclose(Su + np.triu(Su, 1).T, Sd, rtol=1e-5, atol=1e-7 * np.abs(Sd).max())
    np.testing.assert_allclose(rhs, gd, rtol=1e-5, atol=1e-7 * np.abs(gd).max())
    assert abs(cost - lm.cost(lm.x)) < 1e-9 * cost


def test_triangulation_known_answers(oracle):
    sc = scene.make_ring_scene(6, 50, seed=5, noise_px=0.0)
    R, t, c, fk = scene.cameras_for_tracks(sc)
    tr = A.TrackArrays(sc.track_offsets(), sc.obs_cam, sc.obs_xy, R, t, c, fk)
    for fn in (oracle.triangulate_midpoint, oracle.triangulate_dlt):
        X, mse, ok = fn(tr, 1.0, np.deg2rad(2.0))
        np.testing.assert_allclose(X, sc.point_gt, atol=1e-8)  # noise-free tracks recover X
        assert ok.all() and mse.max() < 1e-12
    # angle gate: two nearly parallel rays are rejected (structure.cc:325-355)
    off = np.array([0, 2]); cams = np.array([0, 0]); xy = np.vstack([sc.obs_xy[0], sc.obs_xy[0]])
    tr2 = A.TrackArrays(off, cams, xy, R, t, c, fk)
    _, _, ok = oracle.triangulate_dlt(tr2, 10.0, np.deg2rad(2.0))
    assert not ok[0]
    mse = oracle.reproject_mse(tr, sc.point_gt)
    assert mse.max() < 1e-12


def test_knn_oracle_against_exact_integers(oracle):
    """64 x 64 integer descriptors with planted ties vs int64 arithmetic + stable argsort."""
    rng = np.random.default_rng(2)
    tr = scene._sift_like(rng, 64).astype(np.float32)
    qu = scene._sift_like(rng, 64).astype(np.float32)
    tr[40] = tr[4]; qu[0] = tr[4]; qu[1] = tr[9]
    d = ((tr.astype(np.int64)[None] - qu.astype(np.int64)[:, None]) ** 2).sum(-1)
    order = np.argsort(d, axis=1, kind="stable")[:, :2]
    for fast in (False, True):
        ids, sq = oracle.knn2(tr, qu, fast=fast)
        np.testing.assert_array_equal(ids, order)
        np.testing.assert_array_equal(sq, np.take_along_axis(d, order, 1).astype(np.float32))
    assert (ids[0] == [4, 40]).all()
    code, na, ng = oracle.ratio_codes(ids, sq)
    # query 0 has two exact duplicates in train: ratio = 0/0 = NaN, `ratio < th` is false in the
    # reference loop (fine_matching_graph.cc:118-129) -> no match; query 1 has a unique twin -> good
    assert code[0] == -1 and code[1] == (9 | A.MSFM_MATCH_GOOD) and na >= ng >= 1
    with pytest.raises(ValueError):
        oracle.knn2(tr[:1], qu)


def test_epipolar_filter_known_answer(oracle):
    # F for a pure x-translation: epipolar lines are horizontal, distance = |y2 - y1|
    F = np.array([[0, 0, 0], [0, 0, -1.0], [0, 1.0, 0]])
    p1 = np.array([[10, 20], [0, 0], [5, 5]], np.float32)
    p2 = np.array([[99, 22.5], [50, 3.0], [7, 1.9]], np.float32)
    np.testing.assert_array_equal(oracle.epipolar_filter(p1, p2, F, 3.0), [1, 0, 0])


def test_golden_vectors(oracle):
    """The committed fixtures (tests/golden/, made by tests/golden/make_golden.py) pin the oracle
    against accidental change; the GPU tests compare against the same files."""
    g = np.load(os.path.join(GOLD, "ba_c1_small.npz"))
    arr = A.BaArrays(g["cam_pose0"], g["cam_model0"], g["cam_model_of_cam"], g["point0"], g["obs_cam"], g["obs_pt"],
                     g["obs_xy"], g["pt_weight"], cam_mutable=g["cam_mutable"], pt_mutable=g["pt_mutable"])
    res = oracle.ba_solve(arr, oracle.default_options(max_num_iterations=int(g["max_it"])))
    np.testing.assert_allclose(res["iterations"]["cost"], g["traj_cost"], rtol=1e-10)
    np.testing.assert_array_equal(res["iterations"]["step_is_successful"], g["traj_ok"])
    np.testing.assert_allclose(arr.cam_pose, g["cam_pose"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(arr.point, g["point"], rtol=1e-9, atol=1e-12)
    k = np.load(os.path.join(GOLD, "knn_small.npz"))
    ids, sq = oracle.knn2(k["train"], k["query"])
    np.testing.assert_array_equal(ids, k["ids"])
    np.testing.assert_array_equal(sq, k["sqd"])
    t = np.load(os.path.join(GOLD, "tri_small.npz"))
    tr = A.TrackArrays(t["off"], t["cam"], t["xy"], t["R"], t["t"], t["c"], t["fk"])
    X, mse, ok = oracle.triangulate_midpoint(tr, 3.0, float(t["th_angle"]))
    np.testing.assert_allclose(X, t["X_mid"], rtol=1e-12, atol=1e-12)
    np.testing.assert_array_equal(ok, t["ok_mid"])
    X, mse, ok = oracle.triangulate_dlt(tr, 3.0, float(t["th_angle"]))
    np.testing.assert_allclose(X, t["X_dlt"], rtol=1e-10, atol=1e-10)
    f = np.load(os.path.join(GOLD, "fransac_small.npz"))
    F, inl, nin, ok = oracle.fundamental_ransac(f["off"], f["pt1"], f["pt2"])
    np.testing.assert_array_equal(F, f["F"]); np.testing.assert_array_equal(inl, f["inlier"])
    np.testing.assert_array_equal(nin, f["n_inliers"]); np.testing.assert_array_equal(ok, f["ok"])
    k = np.load(os.path.join(GOLD, "tracks_small.npz"))
    mo = k["match_off"]
    got = oracle.build_tracks([tuple(p) for p in k["pairs"]], [k["matches"][mo[i]:mo[i + 1]] for i in range(len(k["pairs"]))])
    for g_, name in zip(got, ("track_off", "obs_image", "obs_feature")):
        np.testing.assert_array_equal(g_, k[name])


# ---- geometric verification: FM_RANSAC restatement ----
def test_fundamental_ransac_recovers_two_view_geometry(oracle):
    O = oracle
    from tests.twoview import make_batch
    sizes = [400, 60, 29, 0, 1500]
    off, p1, p2, good = make_batch(11, sizes, outlier_frac=0.35)
    F, inl, nin, ok = O.fundamental_ransac(off, p1, p2)
    assert list(ok) == [1, 1, 0, 0, 1]          # < 30 points -> false (geo_verification.cc:34)
    assert nin[2] == 0 and not inl[off[2]:off[3]].any() and not F[2].any()
    for p in (0, 1, 4):
        s = slice(off[p], off[p + 1])
        g = good[s]
        # nearly every true correspondence is kept and nearly every gross outlier rejected
        assert inl[s][g].mean() > 0.9
        assert inl[s][~g].mean() < 0.1
        assert nin[p] == inl[s].sum()
        assert abs(np.linalg.det(F[p])) < 1e-6 * np.abs(F[p]).max() ** 3 + 1e-12   # rank 2
        # the closed-form filter of geo_verification.cc:60-79 agrees with the RANSAC mask up to its one-sided error
        one_sided = O.epipolar_filter(p1[s], p2[s], F[p], 3.0)
        assert (one_sided >= inl[s]).all()


def test_fundamental_ransac_gates_and_determinism(oracle):
    O = oracle
    from tests.twoview import make_batch
    # 40 matches but only ~20 consistent ones: a model is found, the 30-inlier gate says no (geo_verification.cc:54-56)
    off, p1, p2, good = make_batch(5, [40], outlier_frac=0.5)
    F, inl, nin, ok = O.fundamental_ransac(off, p1, p2)
    assert ok[0] == 0 and 7 <= nin[0] < 30 and F[0].any()
    F2, inl2, nin2, ok2 = O.fundamental_ransac(off, p1, p2)
    assert (F == F2).all() and (inl == inl2).all()
    F3, inl3, _, _ = O.fundamental_ransac(off, p1, p2, seed=99)
    assert not (F == F3).all()
    # degenerate input: every match identical -> no model, no crash
    z1 = np.ones((50, 2), np.float32)
    Fz, inz, nz, okz = O.fundamental_ransac(np.array([0, 50], np.int32), z1, z1)
    assert okz[0] == 0 and nz[0] == 0 and not Fz.any()


def test_threaded_oracle_is_bit_identical_to_one_thread(oracle):
    """bench.py times the oracle on one core and on all cores.  Threads only split work whose result does not
    depend on the split - every sum keeps the single-thread order - so the trajectory and the parameters must agree
    bit for bit, with masks, several intrinsics blocks and GPS rows in play."""
    sc = scene.make_aerial_scene(40, 3000, seed=81, n_models=3, gps_sigma=0.5)
    rng = np.random.default_rng(2)
    cm = (np.arange(sc.n_cams) % 5 != 0).astype(np.uint8)
    pm = (rng.random(sc.n_points) > 0.1).astype(np.uint8)
    mk = lambda: A.BaArrays.from_scene(sc, cam_mutable=cm, pt_mutable=pm, gps_xyz=sc.gps_xyz, gps_weight=float(sc.n_obs // sc.n_cams))
    runs = []
    for nt in (1, 4):
        a = mk()
        r = oracle.ba_solve(a, oracle.default_options(max_num_iterations=12, num_threads=nt))
        runs.append((r, a))
    (r1, a1), (r4, a4) = runs
    assert r1["num_iterations"] == r4["num_iterations"] >= 5
    for f in ("cost", "gradient_max_norm", "step_norm", "relative_decrease", "trust_region_radius"):
        np.testing.assert_array_equal(r1["iterations"][f], r4["iterations"][f])
    for f in ("cam_pose", "cam_model", "point"):
        np.testing.assert_array_equal(getattr(a1, f), getattr(a4, f))
    # kNN: queries are independent
    d = [np.random.default_rng(s).uniform(0, 255, (300, 128)).astype(np.float32) for s in (1, 2)]
    oracle.set_num_threads(1)
    i1, s1 = oracle.knn2(d[0], d[1])
    oracle.set_num_threads(4)
    i4, s4 = oracle.knn2(d[0], d[1])
    oracle.set_num_threads(1)
    np.testing.assert_array_equal(i1, i4)
    np.testing.assert_array_equal(s1, s4)


def _compare_with_sparse_lm(oracle, arr_factory, iters, radius=1e4, tol=1e-9, opts=None, huber=1.0):
    """The oracle against SparseLM on the same problem.  Without `opts` the stopping rules are off and the run has `iters`
    iterations; `opts` (msfm_ba_options fields) go to both solvers.  Same termination, number of recorded rows, accept and
    valid sequences; cost to `tol`, |gradient|_max and |step| to 1e-6, the radius to 1e-6."""
    from tests.independent_lm import SparseLM
    from tests import ba_option_cases as K
    arr = arr_factory()
    o = dict(max_num_iterations=iters, function_tolerance=-1.0, parameter_tolerance=-1.0, gradient_tolerance=-1.0,
             initial_trust_region_radius=radius)
    o.update(opts or {})
    res = oracle.ba_solve(arr, oracle.default_options(**o))
    (p, m, X), rec, term = SparseLM(arr_factory(), huber=o.get("huber_delta", huber)).run(o["max_num_iterations"], **K.sparse_lm_kwargs(o))
    it = res["iterations"]
    assert res["termination"] == term, (res["termination"], term)
    assert len(it) == len(rec) == res["num_iterations"] + 1
    if opts is None:
        assert len(it) == iters + 1
    np.testing.assert_array_equal(it["step_is_successful"], [q["ok"] for q in rec])
    np.testing.assert_array_equal(it["step_is_valid"], [q["valid"] for q in rec])
    np.testing.assert_allclose(it["cost"], [q["cost"] for q in rec], rtol=tol)
    np.testing.assert_allclose(it["gradient_max_norm"], [q["gmax"] for q in rec], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(it["step_norm"][1:], [q["step"] for q in rec[1:]], rtol=1e-6)
    np.testing.assert_allclose(it["trust_region_radius"], [q["radius"] for q in rec], rtol=1e-6)
    res["sparse_lm"] = rec
    return arr, (p, m, X), it


def test_lm_against_sparse_complex_step_solver_c1(oracle):
    """The independent pin at BASELINE config 1's size (10 cameras / 2000 points / 20000 observations): exact (complex-step)
    Jacobian, no Schur complement, sparse LU.  Trajectory agreement to 1e-9 in cost over 8 iterations; the damped step is
    unique, so the parameters agree too (loosely: nothing fixes the 7-DoF gauge, cond ~ radius)."""
    sc = scene.config_scene(1)
    arr, (p, m, X), it = _compare_with_sparse_lm(oracle, lambda: A.BaArrays.from_scene(sc), 8)
    assert it["step_is_successful"].all() and it["cost"][-1] < 1e-3 * it["cost"][0]
    assert np.abs(arr.cam_pose - p).max() < 1e-6 * np.abs(p).max() and np.abs(arr.point - X).max() < 1e-6 * np.abs(X).max()
    assert np.abs(arr.cam_model - m).max() < 1e-6 * np.abs(m).max()


def test_lm_rejected_steps_against_sparse_solver(oracle):
    """Frozen cameras left at their perturbed poses make the first trial steps fail: rejected steps (radius /2, /4, ... with
    the LM diagonal reused, the candidate's cost recorded) interleaved with accepted ones - the same sequence in both."""
    sc = scene.make_aerial_scene(14, 2000, seed=17)
    cm = np.ones(sc.n_cams, np.uint8); cm[::4] = 0
    pm = (np.arange(sc.n_points) % 11 != 0).astype(np.uint8)
    arr, _, it = _compare_with_sparse_lm(oracle, lambda: A.BaArrays.from_scene(sc, cam_mutable=cm, pt_mutable=pm), 12, tol=1e-8)
    ok = it["step_is_successful"][1:]
    assert (ok == 0).sum() >= 4 and (ok == 1).sum() >= 3


def test_lm_masks_gps_huber_against_sparse_solver(oracle):
    """Frozen cameras / points / one frozen intrinsics block, GPS rows on the free cameras (r = w |t - g|, z at w / 5,
    Huber(1), gps_error_pose_absolute.h:31-44) and 3 % gross outliers that keep the Huber corrector active."""
    sc = scene.make_aerial_scene(12, 2000, seed=91, n_models=2, gps_sigma=0.5, rot_sigma=0.02, trans_sigma=0.3, point_sigma=0.2)
    rng = np.random.default_rng(5)
    bad = rng.random(sc.n_obs) < 0.03
    sc.obs_xy[bad] += rng.normal(0, 50.0, (int(bad.sum()), 2))
    cm = np.ones(sc.n_cams, np.uint8); cm[[1, 6]] = 0
    pm = (rng.random(sc.n_points) > 0.15).astype(np.uint8)
    mm = np.array([1, 0], np.uint8)
    w = np.where(np.diff(sc.track_offsets()) >= 3, 2.0, 1.0)
    mk = lambda: A.BaArrays(sc.cam_pose, sc.cam_model, sc.cam_model_of_cam, sc.point, sc.obs_cam, sc.obs_pt, sc.obs_xy, w, cam_mutable=cm,
                            model_mutable=mm, pt_mutable=pm, gps_xyz=sc.gps_xyz, gps_weight=float(sc.n_obs // sc.n_cams))
    arr, (p, m, X), it = _compare_with_sparse_lm(oracle, mk, 8)
    assert it["cost"][-1] < it["cost"][0]
    np.testing.assert_array_equal(arr.cam_pose[cm == 0], sc.cam_pose[cm == 0])
    np.testing.assert_array_equal(arr.cam_model[1], sc.cam_model[1])
    assert np.abs(arr.cam_pose - p).max() < 1e-7 * np.abs(p).max() and np.abs(arr.point - X).max() < 1e-7 * np.abs(X).max()


def test_slam_gate_known_answers(oracle):
    """slam_gps.cc:466-503 on hand-made cases: `ratio > th` keeps equality and 0/0, the epipolar distance of a point to a
    known line, the homography transfer distance at 40 x th_distance, the order of the three checks."""
    O = oracle
    F = np.array([[0, 0, 0], [0, 0, -1.0], [0, 1.0, 0]])      # pure x-translation: l = (0, -1, y1) -> distance |y2 - y1|
    H = np.eye(3)
    kp1 = np.array([[10, 20], [30, 40], [50, 60], [70, 80], [1, 2], [3, 4]], np.float32)
    kp2 = np.array([[300, 20.0], [30, 42.0], [50, 62.5], [70 + 199.0, 80], [1 + 201.0, 2], [3, 4]], np.float32)
    ids = np.array([[0, 1], [1, 0], [2, 0], [3, 0], [4, 0], [5, 0]], np.int32)
    d = np.array([[8, 10], [1, 2], [1, 2], [1, 2], [1, 2], [0, 0]], np.float32)
    code, nr, nk = O.slam_gate(ids, d, kp1, kp2, F, H, 0.8, 2.0, 5.0)
    # m0: ratio 0.8 == th kept by `>`, epi 0, homography distance 290 > 200 -> rejected by check3
    # m1: epi 2.0 == th kept, transfer 2 -> kept;  m2: epi 2.5 > 2 rejected;  m3: transfer 199 kept;  m4: 201 rejected
    # m5: 0/0 = NaN passes check1 (NaN > th is false), distances 0 -> kept
    assert code.tolist() == [-1, 1, -1, 3, -1, 5] and (nr, nk) == (6, 3)
    code, nr, nk = O.slam_gate(ids, d, kp1, kp2, F, H, 0.79, 2.0, 5.0)
    assert nr == 5 and code[0] == -1                 # ratio 0.8 > 0.79
    # a degenerate epipolar line (F = 0): 0 / 0 = NaN is not > th, the match falls through to the homography check
    code, _, nk = O.slam_gate(ids, d, kp1, kp2, np.zeros((3, 3)), H, 0.8, 2.0, 5.0)
    assert code.tolist() == [-1, 1, 2, 3, -1, 5]
    # general F / H against a numpy evaluation in the same operation order
    rng = np.random.default_rng(3)
    F = np.array([[0, 0, 0], [0, 0, -1.0], [0, 1.0, 0]]) + 1e-7 * rng.normal(size=(3, 3))
    H = np.eye(3) + 1e-5 * rng.normal(size=(3, 3))
    kp1 = rng.uniform(-2000, 2000, (500, 2)).astype(np.float32)
    kp2 = (kp1[::-1] + np.column_stack([rng.uniform(-300, 300, 500), rng.normal(0, 1.5, 500)])).astype(np.float32)
    ids = np.column_stack([np.arange(500)[::-1], np.zeros(500)]).astype(np.int32)
    d = np.column_stack([rng.uniform(0, 1, 500), np.ones(500)]).astype(np.float32)
    code, nr, nk = O.slam_gate(ids, d, kp1, kp2, F, H, 0.8, 2.0, 5.0)
    want = []
    for m in range(500):
        if np.float32(d[m, 0]) / np.float32(d[m, 1]) > np.float32(0.8):
            want.append(-1); continue
        p1 = np.array([kp1[ids[m, 0], 0], kp1[ids[m, 0], 1], 1.0], np.float64)
        p2 = np.array([kp2[m, 0], kp2[m, 1], 1.0], np.float64)
        l = [(F[r, 0] * p1[0] + F[r, 1] * p1[1]) + F[r, 2] * p1[2] for r in range(3)]
        epi = abs((l[0] * p2[0] + l[1] * p2[1]) + l[2] * p2[2]) / np.sqrt(l[0] * l[0] + l[1] * l[1])
        if epi > np.float32(2.0):
            want.append(-1); continue
        q = [(H[r, 0] * p1[0] + H[r, 1] * p1[1]) + H[r, 2] * p1[2] for r in range(3)]
        sc = 1.0 / q[2]
        dx, dy = p2[0] - q[0] * sc, p2[1] - q[1] * sc
        want.append(-1 if np.sqrt(dx * dx + dy * dy) > np.float32(40) * np.float32(5.0) else int(ids[m, 0]))
    assert code.tolist() == want and nk == sum(w >= 0 for w in want) and 0 < nk < nr


# ---- the oracle's handling of msfm_ba_options, its stopping rules and its failure path, pinned before the GPU is compared with it ----
def _option_case(oracle, name):
    from tests import ba_option_cases as K
    c = K.CASES[name]
    tol = 1e-8 if c["scene"] == "J" else 1e-9      # (J: rejected trial steps with costs 300x the accepted ones)
    arr, (p, m, X), it = _compare_with_sparse_lm(oracle, lambda: K.case_arrays(name), None, tol=tol, opts=c["opts"])
    if name in K.EXPECT:
        res = oracle.ba_solve(K.case_arrays(name), oracle.default_options(**c["opts"]))
        assert (res["termination"], res["num_iterations"]) == K.EXPECT[name]
    # both solvers end at the same parameters (loosely: nothing fixes the gauge, cond ~ radius)
    for g, r in ((arr.cam_pose, p), (arr.cam_model, m), (arr.point, X)):
        assert np.abs(g - r).max() <= 1e-6 * np.abs(r).max()
    return it


@pytest.mark.parametrize("name", ["huber-O-0.25", "huber-O-4", "huber-O-1e6", "huber-G-0.25", "huber-G-4", "huber-J-0.25", "huber-J-400"])
def test_oracle_huber_delta_against_sparse_solver(oracle, name):
    """huber_delta other than 1: reprojection rows of free and frozen blocks and GPS rows on both sides of the threshold."""
    _option_case(oracle, name)


@pytest.mark.parametrize("name", ["lmdiag-default", "lmdiag-min10", "lmdiag-max1e-4", "lmdiag-noscale", "lmdiag-zero-weight"])
def test_oracle_lm_diagonal_options_against_sparse_solver(oracle, name):
    """min_lm_diagonal / max_lm_diagonal clamps that bind, with and without the Jacobi scaling, and points of zero weight
    whose blocks are the clamped diagonal alone."""
    _option_case(oracle, name)


@pytest.mark.parametrize("name", ["cap-R", "mrd-O", "mrd-J", "minrad-R", "minrad-J", "grad-R", "grad-R-late", "grad-J", "param-R", "func-R"])
def test_oracle_radius_and_stopping_rules_against_sparse_solver(oracle, name):
    """The radius cap, min_relative_decrease, and every termination by a radius or a tolerance, in the Ceres 1.13 order."""
    _option_case(oracle, name)


@pytest.mark.parametrize("name", ["fail-Z-5", "fail-Z-3", "fail-Z-1", "grad-Z"])
def test_oracle_invalid_steps_and_failure_against_sparse_solver(oracle, name):
    """All weights zero: the model cost change is exactly 0, every step invalid; the radius is divided by 2, 4, 8, ... and the
    max_num_consecutive_invalid_steps-th invalid step in a row ends the run with FAILURE, unrecorded."""
    from tests import ba_option_cases as K
    it = _option_case(oracle, name)
    assert (it["cost"] == 0).all() and (it["step_is_valid"][1:] == 0).all()
    np.testing.assert_array_equal(it["trust_region_radius"], [1e4, 5e3, 1.25e3, 156.25, 9.765625][:len(it)])


def test_option_cases_meet_the_condition_on_their_inputs(oracle):
    """Every decision of every compared trajectory has a margin in the oracle (tests/ba_option_cases.py: decision_margins,
    firing_margin) and ends as the table says - so that the GPU comparison never sits on the rounding floor."""
    from tests import ba_option_cases as K
    for name, c in K.CASES.items():
        res = oracle.ba_solve(K.case_arrays(name), oracle.default_options(**c["opts"]))
        K.decision_margins(res, c["opts"], gradient_factor=1.3 if name == "grad-J" else 2.0)
        if name in K.EXPECT:
            assert (res["termination"], res["num_iterations"]) == K.EXPECT[name], name
    for name in ("param-R", "func-R"):
        K.firing_margin(oracle.ba_solve, oracle.default_options, name)
