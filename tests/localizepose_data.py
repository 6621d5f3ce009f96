"""Inputs shared by tests/test_localizepose_ref.py, tests/test_gpu_localizepose*.py and tests/golden/make_localizepose_golden.py:
one localisation round on tests/localize_data.ring_round(wrong=0.2, exact=True) - 10 cameras, 200 points, candidates 6-9 - with
what IncrementalSfM::LocalizeImage (sfm_incremental.cc:565-729) distinguishes planted into it, and a second scene whose one
candidate has more than 1 100 correspondences (several workgroups per row).

ring case: keypoint noise of 0.3 / 6.0 / 1.5 / 0.0 px on images 6 / 7 / 8 / 9 (default_rng(5)), fail_times = [1, 0, 0, 0], so
the rank is 7, 8, 9, 6 and image 7, tried first, misses the 5.0 px gate.  Every candidate gets N_DUP extra features 200.. whose
keypoints copy those of the features DUP_FEATS (kept free of noise, so they are inliers wherever the pose is good) and which
match the same registered feature of image 0: the point is named twice among the inliers, the copy (equal mse, higher feature)
comes second.  NEW_ADDED points carry is_new_added_ on entry.

The expected patterns (EXPECT) were recorded from tests/localizepose_ref.py over the oracle; tests/test_localizepose_ref.py
verifies them on the CPU."""
import functools

import numpy as np

from metricsfm_amd import scene
from metricsfm_amd.tracks import flat_matches_from_scene
from tests import localize_data as D
from tests.localize_ref import localize_ref

N_DUP = 3
NOISE = {6: 0.3, 7: 6.0, 8: 1.5, 9: 0.0}
FAIL = [1, 0, 0, 0]
NEW_ADDED = [60, 61, 62, 63, 120]
SWEEP = dict(f_ratio_min=0.8, f_ratio_max=1.2, f_ratio_step=0.05, max_iter=200, seed=0x4D53464D50)   # 8 steps; step 4 is ~ f_init

# ring case, rows in rank order (images 7, 8, 9, 6): every row on the known-focal arm / rows 1 and 3 on the sweep arm (SWEEP, f_init
# = the true focal length) / the known-focal arm without NEW_ADDED.  The avg_error are 6.77, 2.36, 1.20, 1.12 (known) and 6.39,
# 1.28 (rows 1 and 3 swept: image 8 keeps step 3, f = 0.95 f_init, and misses the gate).
EXPECT = dict(
    images=[7, 8, 9, 6], n_corr=[203, 203, 203, 203], dup_feats=[1, 4, 5],
    known=dict(passes=[0, 1, 1, 1], winner=1, next_row=-1, n_inliers=[0, 104, 102, 100], n_outliers=[0, 95, 95, 98], state3=[0, 4, 6, 5]),
    mixed=dict(arm=[1, 2, 1, 2], passes=[0, 0, 1, 1], winner=2, best_step=[-1, 3, -1, 4], n_inliers=[0, 0, 102, 103], n_outliers=[0, 0, 95, 95]),
    not_added=dict(n_inliers=[0, 105, 106, 103], state3=[0, 3, 2, 2]),
)
# big case: one row of 1 200 correspondences, known focal length: avg_error 1.58
EXPECT_BIG = dict(n_corr=[1200], passes=[1], winner=0, n_inliers=[681], n_outliers=[511], state3=[8])


def _add_extra_features(c, cands, dup_feats):
    """Every candidate image gets len(dup_feats) more features; feature n0 + e copies the keypoint of feature dup_feats[e] and
    matches feature dup_feats[e] of image 0, behind the pair's other matches."""
    nf = c["n_features"].astype(np.int64)
    start = np.concatenate([[0], np.cumsum(nf)])
    kp_rows, new_nf = [], nf.copy()
    for im in range(len(nf)):
        rows = c["keypoints"][start[im]:start[im + 1]]
        if im in cands:
            rows = np.concatenate([rows, rows[dup_feats]])
            new_nf[im] += len(dup_feats)
        kp_rows.append(rows)
    lens = np.diff(c["match_off"]).astype(np.int64)
    per_pair = [c["matches"][c["match_off"][p]:c["match_off"][p + 1]] for p in range(len(c["pairs"]))]
    for p, (i, j) in enumerate(c["pairs"]):
        if int(i) in cands and int(j) == 0:
            extra = np.column_stack([nf[i] + np.arange(len(dup_feats)), dup_feats]).astype(np.int32)
            per_pair[p] = np.concatenate([per_pair[p], extra])
            lens[p] += len(dup_feats)
    c["n_features"] = new_nf.astype(np.int32)
    c["keypoints"] = np.ascontiguousarray(np.concatenate(kp_rows), np.float32)
    c["matches"] = np.ascontiguousarray(np.concatenate(per_pair), np.int32)
    c["match_off"] = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def _first_correct_features(c, k):
    """The first k features f for which every candidate's correspondence of f is point f (its first qualifying match is no
    planted wrong one), skipping the points of NEW_ADDED."""
    ref = localize_ref(*D.store_args(c), *D.problem_args(c))
    good = None
    for r in range(len(ref["rank"])):
        b, e = ref["corr_off"][r], ref["corr_off"][r + 1]
        ok = set(int(f) for f, p in zip(ref["corr_feat"][b:e], ref["corr_point"][b:e]) if f == p)
        good = ok if good is None else good & ok
    return np.array(sorted(good - set(NEW_ADDED))[:k], np.int64)


@functools.lru_cache(maxsize=None)
def ring_case():
    c = D.ring_round(wrong=0.2, exact=True)
    c["fail_times"] = np.array(FAIL, np.int32)
    n_pts = len(c["pt_mse"])
    dup = _first_correct_features(c, N_DUP)
    rng = np.random.default_rng(5)
    kp = c["keypoints"].astype(np.float64)
    for im in (6, 7, 8, 9):
        noise = rng.normal(0.0, 1.0, (n_pts, 2)) * NOISE[im]
        noise[dup] = 0.0
        kp[im * n_pts:(im + 1) * n_pts] += noise
    c["keypoints"] = kp.astype(np.float32)
    _add_extra_features(c, (6, 7, 8, 9), dup)
    c["dup_feats"] = dup
    c["pt_new_added"] = np.zeros(n_pts, np.uint8)
    c["pt_new_added"][NEW_ADDED] = 1
    c["f"] = float(scene.FOCAL)
    c["loc"] = localize_ref(*D.store_args(c), *D.problem_args(c), point_xyz=c["point_xyz"], keypoints=c["keypoints"])
    return c


@functools.lru_cache(maxsize=None)
def big_case():
    """4 cameras, 1 200 points: cameras 0-2 registered, image 3 the one candidate, 0.5 px noise."""
    sc = scene.make_ring_scene(4, 1200, seed=scene.SEED_BASE + 43)
    nf, pairs, moff, m = flat_matches_from_scene(sc, wrong=0.1, seed=9)
    rng = np.random.default_rng(9)
    n_reg, n_pts = 3, sc.n_points
    kp = np.zeros((sc.n_cams * n_pts, 2), np.float64)
    kp[sc.obs_cam.astype(np.int64) * n_pts + sc.obs_pt] = sc.obs_xy
    kp[3 * n_pts:] += rng.normal(0.0, 0.5, (n_pts, 2))
    added = np.zeros(n_pts, np.uint8)
    added[::97] = 1
    c = dict(n_features=nf, pairs=pairs, match_off=moff, matches=m, cam_img=np.arange(n_reg, dtype=np.int32),
             feat_point=np.tile(np.arange(n_pts, dtype=np.int32), n_reg), pt_bad=np.zeros(n_pts, np.uint8), pt_mse=rng.uniform(0.0, 4.0, n_pts),
             pt_views=rng.integers(2, 6, n_pts).astype(np.int32), cand_img=np.array([3], np.int32), fail_times=np.zeros(1, np.int32),
             point_xyz=sc.point_gt.copy(), keypoints=kp.astype(np.float32), pt_new_added=added, f=float(scene.FOCAL))
    c["loc"] = localize_ref(*D.store_args(c), *D.problem_args(c), point_xyz=c["point_xyz"], keypoints=c["keypoints"])
    return c


ROW_ARRAYS = ("tried", "arm", "pass", "f", "R", "t", "avg_error", "best_step", "best_iter", "n_inliers", "n_outliers")
CORR_ARRAYS = ("errors", "corr_state")
SCALARS = ("n_tried", "winner", "next_row")

ROW_F = dict(known=lambda c: np.full(4, c["f"]), mixed=lambda c: np.array([c["f"], 0.0, c["f"], 0.0]), not_added=lambda c: np.full(4, c["f"]))


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement over the oracle, computed once per process: "known", "mixed", "not_added" (ring case), "big"."""
    from oracle import oracle as O
    from tests import localizepose_ref as PR
    known, swept = PR.oracle_solvers(O, sweep=SWEEP)
    if name == "big":
        c = big_case()
        return PR.localize_poses_ref(c["loc"], c["f"], None, len(c["pt_mse"]), c["pt_new_added"], known, swept)
    c = ring_case()
    added = None if name == "not_added" else c["pt_new_added"]
    return PR.localize_poses_ref(c["loc"], ROW_F[name](c), c["f"], len(c["pt_mse"]), added, known, swept)


def state_count(res, loc, state):
    off = loc["corr_off"]
    return [int((res["corr_state"][off[r]:off[r + 1]] == state).sum()) for r in range(len(off) - 1)]


# ---- one round in both hosts: tests/localizepose_host_check.cc and metricsfm_amd/localize.py ----
def host_round():
    """The ring case as the flat state of metricsfm_amd/newpoints.py plus the per-image settings: every image its own camera
    model; image 8 (row 1) without a focal length, so that row takes the sweep (default options) around the true value."""
    c = ring_case()
    sc = c["scene"]
    n_img, n_reg = len(c["n_features"]), len(c["cam_img"])
    R = scene.angle_axis_to_R(sc.cam_pose_gt[:n_reg, :3])
    t = sc.cam_pose_gt[:n_reg, 3:]
    state = dict(n_features=c["n_features"], cam_img=c["cam_img"].copy(), feat_point=c["feat_point"].copy(), cam_R=R, cam_t=t.copy(),
                 cam_c=-np.einsum("nji,nj->ni", R, t), cam_fk=np.tile([c["f"], 0.0, 0.0], (n_reg, 1)), point_xyz=c["point_xyz"].copy(),
                 pt_bad=c["pt_bad"].copy(), pt_mse=c["pt_mse"].copy(), pt_views=c["pt_views"].copy(), pt_new_added=c["pt_new_added"].copy())
    image_f = np.full(n_img, c["f"])
    image_f[8] = 0.0
    fail = np.zeros(n_img, np.int32)
    fail[c["cand_img"]] = c["fail_times"]
    match_count = np.zeros((n_img, n_img), np.int32)
    match_count[c["pairs"][:, 0], c["pairs"][:, 1]] = np.diff(c["match_off"])
    return dict(case=c, state=state, image_f=image_f, image_f_init=np.full(n_img, c["f"]), image_model=np.arange(n_img, dtype=np.int32),
                fail_times=fail, match_count=match_count)


def host_check_command(exe):
    """The compiler call for tests/localizepose_host_check.cc against this tree's library."""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "metricsfm_amd")
    return ["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(root, "host"), "-I", os.path.join(root, "include"),
            os.path.join(root, "tests", "localizepose_host_check.cc"), os.path.join(root, "host", "objectsfm.cc"), "-o", str(exe),
            "-L" + lib, "-lmsfm", "-Wl,-rpath," + lib, "-Wl,-rpath-link,/opt/rocm/lib"]


def write_host_round(path, h):
    """A round in the byte layout tests/localizepose_host_check.cc reads."""
    c, s = h["case"], h["state"]
    i32 = lambda x: np.ascontiguousarray(np.asarray(x, dtype=np.int32).reshape(-1))
    f64 = lambda x: np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1))
    with open(path, "wb") as fh:
        for a in ([len(c["n_features"])], c["n_features"], [len(c["pairs"])], c["pairs"], c["match_off"], c["matches"], [len(s["cam_img"])],
                  s["cam_img"], s["feat_point"], [len(s["pt_mse"])], s["pt_bad"], s["pt_views"], s["pt_new_added"], h["fail_times"], h["image_model"]):
            fh.write(i32(a).tobytes())
        for a in (s["pt_mse"], s["point_xyz"], s["cam_R"], s["cam_t"], s["cam_c"], s["cam_fk"], h["image_f"], h["image_f_init"]):
            fh.write(f64(a).tobytes())
        fh.write(np.ascontiguousarray(c["keypoints"], dtype=np.float32).tobytes())


def read_host_round_result(path, h):
    raw = open(path, "rb").read()
    pos = [0]

    def take(dtype, n):
        a = np.frombuffer(raw, dtype, n, pos[0])
        pos[0] += a.nbytes
        return a
    image, n_failed = (int(v) for v in take(np.int32, 2))
    out = dict(image=image, failed=take(np.int32, n_failed))
    n_pts = len(h["state"]["pt_mse"])
    if image >= 0:
        out["feat_row"] = take(np.int32, int(h["case"]["n_features"][image]))
    out["pt_bad"], out["pt_views"], out["pt_new_added"] = take(np.int32, n_pts), take(np.int32, n_pts), take(np.int32, n_pts)
    out["visible"] = take(np.int32, int(take(np.int32, 1)[0]))
    n_new = int(take(np.int32, 1)[0])
    out["new"] = take(np.int32, 3 * n_new).reshape(n_new, 3)
    if image >= 0:
        out["f"], out["R"], out["t"], out["c"] = float(take(np.float64, 1)[0]), take(np.float64, 9).reshape(3, 3), take(np.float64, 3), take(np.float64, 3)
    out["X"], out["mse"] = take(np.float64, 3 * n_new).reshape(n_new, 3), take(np.float64, n_new)
    assert pos[0] == len(raw)
    return out
