"""Inputs shared by tests/test_localize_ref.py and tests/test_gpu_localize*.py: hand-made cases of a few matches each that pin
the quirks of IncrementalSfM::FindImageToLocalize (sfm_incremental.cc:440-562) with expectations written out by hand, and
the ring-scene round."""
import numpy as np

from metricsfm_amd import scene
from metricsfm_amd.tracks import flat_matches_from_scene

# Five images: 0 and 1 are registered (cameras 0 and 1), 2, 3 and 4 are not.  Camera 0 holds point f under feature f,
# camera 1 holds point 10 + f under feature f, except its features 6 and 7, which hold none.
N_FEATURES = [10, 8, 12, 4, 12]
CAM_IMG = [0, 1]
FEAT_POINT = list(range(10)) + [10, 11, 12, 13, 14, 15, -1, -1]
N_POINTS = 18


def _case(pairs, cand, fail, expect, bad=(), views2=(), mse=None):
    pt_bad = np.zeros(N_POINTS, np.uint8); pt_bad[list(bad)] = 1
    pt_views = np.full(N_POINTS, 3, np.int32); pt_views[list(views2)] = 2
    keys = sorted(pairs)
    lens = [len(pairs[k]) for k in keys]
    flat = [m for k in keys for m in pairs[k]]
    e = dict(rank=[], corr_off=[0], corr_feat=[], corr_point=[], vis_off=[0], vis_cam=[])
    for k, corr, vis in expect:
        e["rank"].append(k)
        e["corr_feat"] += [f for f, _ in corr]; e["corr_point"] += [p for _, p in corr]; e["corr_off"].append(len(e["corr_feat"]))
        e["vis_cam"] += vis; e["vis_off"].append(len(e["vis_cam"]))
    return dict(n_features=np.array(N_FEATURES, np.int32), pairs=np.array(keys, np.int32).reshape(-1, 2),
                match_off=np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), matches=np.array(flat, np.int32).reshape(-1, 2),
                cam_img=np.array(CAM_IMG, np.int32), feat_point=np.array(FEAT_POINT, np.int32), pt_bad=pt_bad,
                pt_mse=np.arange(N_POINTS) * 0.125 if mse is None else np.asarray(mse, np.float64), pt_views=pt_views,
                cand_img=np.array(cand, np.int32), fail_times=np.array(fail, np.int32),
                expect={k: np.array(v, np.int32) for k, v in e.items()})


_SIX = [(f, f) for f in range(6)]
_NINE = [(f, f) for f in range(9)]

# name -> case; expect = [(index into cand_img, [(feature, point) in output order], [visible cameras])] in rank order
QUIRKS = {
    # feature 0 twice in pair (2, 0): the first match keeps it (point 0, not 1), both count -> 6 > 5, camera 0 visible;
    # feature 1 again in pair (2, 1): it keeps point 2 of the earlier pair; image 3 has no pair at all and is absent
    "duplicates_first_wins_all_counted": _case(
        {(2, 0): [(0, 0), (0, 1), (1, 2), (2, 3), (3, 4), (4, 5)], (2, 1): [(1, 0), (5, 1)]}, [2, 3], [0, 0],
        [(0, [(0, 0), (1, 2), (2, 3), (3, 4), (4, 5), (5, 11)], [0])]),
    # point 5 is badly estimated: 5 correspondences, count 5 -> camera 0 not visible
    "bad_point_does_not_count": _case({(2, 0): _SIX}, [2], [0], [(0, [(f, f) for f in range(5)], [])], bad=[5]),
    # point 0 has two views: its 0.0 becomes 3.0 and goes behind 0.125 .. 0.625
    "two_views_add_three": _case({(2, 0): _SIX}, [2], [0], [(0, [(1, 1), (2, 2), (3, 3), (4, 4), (5, 5), (0, 0)], [0])], views2=[0]),
    # equal mse: the lower feature first (points 1 and 2 share 0.5; feature 7 -> point 1, feature 3 -> point 2)
    "equal_mse_lower_feature_first": _case(
        {(2, 0): [(7, 1), (3, 2), (0, 3), (1, 4), (2, 5)]}, [2], [0], [(0, [(0, 3), (1, 4), (2, 5), (3, 2), (7, 1)], [])],
        mse=[0, 0.5, 0.5, 0.125, 0.25, 0.375] + [1.0] * 12),
    # NaN sorts last
    "nan_mse_last": _case({(2, 0): _SIX}, [2], [0], [(0, [(0, 0), (1, 1), (3, 3), (4, 4), (5, 5), (2, 2)], [0])],
                          mse=[0, 0.125, float("nan"), 0.375, 0.5, 0.625] + [1.0] * 12),
    # exactly 5 matches through camera 0, 6 through camera 1: only camera 1 is visible
    "count_five_versus_six": _case(
        {(2, 0): [(f, f) for f in range(5)], (2, 1): [(6 + f, f) for f in range(6)]}, [2], [0],
        [(0, [(f, f) for f in range(5)] + [(6 + f, 10 + f) for f in range(6)], [1])]),
    # 9 / (5 + 0) = 1 stays, 9 / (5 + 5) = 0 goes
    "score_is_an_integer_division": _case({(2, 0): _NINE, (4, 0): _NINE}, [2, 4], [0, 5], [(0, [(f, f) for f in range(9)], [0])]),
    # the higher score first, although its image id is higher: 10 / 5 = 2 against 9 / 5 = 1
    "higher_score_first": _case({(2, 0): _NINE, (4, 0): _NINE + [(9, 9)]}, [2, 4], [0, 0],
                                [(1, [(f, f) for f in range(10)], [0]), (0, [(f, f) for f in range(9)], [0])]),
    # image 4: a pair without matches and a pair whose matches all name features without a point
    "pair_without_qualifying_matches": _case({(2, 0): _SIX, (4, 0): [], (4, 1): [(0, 6), (1, 7)]}, [2, 4], [0, 0],
                                             [(0, [(f, f) for f in range(6)], [0])]),
}

ARRAYS = ("rank", "corr_off", "corr_feat", "corr_point", "vis_off", "vis_cam")


def problem_args(c):
    """The arguments of localize_ref / Context.localize_candidates behind the store."""
    return [c[k] for k in ("cam_img", "feat_point", "pt_bad", "pt_mse", "pt_views", "cand_img", "fail_times")]


def store_args(c):
    return [c[k] for k in ("n_features", "pairs", "match_off", "matches")]


def ring_round(wrong=0.2, seed=7, exact=False):
    """make_ring_scene(10 cameras, 200 points): cameras 0-5 registered, 6-9 candidates.  Every camera sees every point in point
    order, so feature f of an image is point f.  About 10 % of the registered features hold no point, about 5 % of the points are
    bad, views are mixed 2 / 3+, mse is seeded with exact ties planted (also across the + 3.0).  exact=True: every feature
    holds its point, nothing is bad (the round that goes on to EPnP)."""
    sc = scene.make_ring_scene(10, 200, seed=scene.SEED_BASE + 41)
    nf, pairs, moff, m = flat_matches_from_scene(sc, wrong=wrong, seed=seed)
    rng = np.random.default_rng(seed)
    n_reg, n_pts = 6, sc.n_points
    fp = np.tile(np.arange(n_pts, dtype=np.int32), n_reg)
    pt_bad = np.zeros(n_pts, np.uint8)
    if not exact:
        fp[rng.random(len(fp)) < 0.10] = -1
        pt_bad[rng.random(n_pts) < 0.05] = 1
    pt_views = np.where(rng.random(n_pts) < 0.4, 2, rng.integers(3, 9, n_pts)).astype(np.int32)
    pt_mse = rng.uniform(0.0, 4.0, n_pts)
    pt_mse[10:20] = pt_mse[0:10]                       # ties between points
    pt_mse[30:40] = 0.75; pt_views[30:35] = 2; pt_views[35:40] = 3
    pt_mse[40:45] = 3.75; pt_views[40:45] = 5          # ties of 0.75 + 3.0 with 3.75
    kp = np.zeros((sc.n_cams * n_pts, 2), np.float32)
    kp[sc.obs_cam.astype(np.int64) * n_pts + sc.obs_pt] = sc.obs_xy
    fail = np.array([0, 2, 0, 1], np.int32)
    return dict(n_features=nf, pairs=pairs, match_off=moff, matches=m, cam_img=np.arange(n_reg, dtype=np.int32), feat_point=fp,
                pt_bad=pt_bad, pt_mse=pt_mse, pt_views=pt_views, cand_img=np.arange(n_reg, sc.n_cams, dtype=np.int32), fail_times=fail,
                point_xyz=sc.point_gt.copy(), keypoints=kp, scene=sc)


def write_round(path, c, fail_by_image):
    """One localisation round in the byte layout tests/localize_host_check.cc reads."""
    with open(path, "wb") as fh:
        def ints(*xs):
            for x in xs:
                np.ascontiguousarray(np.asarray(x, dtype=np.int32)).tofile(fh)
        ints([len(c["n_features"])], c["n_features"], [len(c["pairs"])], c["pairs"], c["match_off"], c["matches"], [len(c["cam_img"])], c["cam_img"],
             c["feat_point"], [len(c["pt_bad"])], c["pt_bad"], c["pt_views"])
        np.ascontiguousarray(c["pt_mse"], dtype=np.float64).tofile(fh)
        ints(fail_by_image)


def read_round_result(path):
    """What localize_host_check.cc wrote: image_ids, per image the (feature, point) rows and the visible cameras."""
    raw = np.fromfile(path, dtype=np.int32)
    n, pos = int(raw[0]), 1
    ids = raw[pos:pos + n].tolist(); pos += n
    corres, visible = [], []
    for _ in range(n):
        k = int(raw[pos]); corres.append(raw[pos + 1:pos + 1 + 2 * k].reshape(-1, 2)); pos += 1 + 2 * k
        k = int(raw[pos]); visible.append(raw[pos + 1:pos + 1 + k]); pos += 1 + k
    assert pos == len(raw)
    return ids, corres, visible


def host_check_command(exe):
    """The compiler call for tests/localize_host_check.cc against this tree's library."""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "metricsfm_amd")
    return ["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(root, "host"), "-I", os.path.join(root, "include"),
            os.path.join(root, "tests", "localize_host_check.cc"), os.path.join(root, "host", "objectsfm.cc"), "-o", str(exe),
            "-L" + lib, "-lmsfm", "-Wl,-rpath," + lib, "-Wl,-rpath-link,/opt/rocm/lib"]
