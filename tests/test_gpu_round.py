"""msfm_round_adjust - PartialBundleAdjustment, FullBundleAdjustment and RemovePointOutliers of a round (sfm_incremental.cc:172-186)
on the flat state in one call - against tests/round_ref.py, a literal dict / sorted(map) walk of the same rules: the assembled
problems, the masks, the view counts, the outlier flags and every count identical; the solves identical to msfm_ba_solve on the
restated arrays, iteration row for iteration row.  (tests/test_round_ref.py holds the walk to metricsfm_amd/window.py and asserts
the margins of the seeded cases.)"""
import types

import numpy as np
import pytest

from metricsfm_amd import _abi as A
from metricsfm_amd import adjust, capi, scene
from tests import round_data as D
from tests import round_ref as RR

pytestmark = pytest.mark.gpu
STAGES = ("partial", "full")
PROBLEM = ("kept", "obs_cam", "obs_pt", "obs_xy", "pt_weight", "cam_mutable", "pt_mutable")
SUMMARY = ("termination", "num_iterations", "num_successful_steps", "num_unsuccessful_steps", "initial_cost", "final_cost", "num_residuals",
           "num_reduced_params")
WEIGHT = (2.0, 1.0)


@pytest.fixture(scope="module")
def main():
    return D.main_case()


def run(ctx, c, store=None, **kw):
    own = store is None
    store = ctx.match_store(*D.store_args(c)) if own else store
    kw.setdefault("keypoints", c["keypoints"])
    kw.setdefault("new_cam", c["new_cam"])
    kw.setdefault("visible", c["visible"])
    kw.setdefault("pt_new_added", c["pt_new_added"])
    try:
        return ctx.round_adjust(store, *D.call_args(c), **kw)
    finally:
        if own:
            store.close()


def same(got, want, keys):
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, w.dtype, g.shape, w.shape)
        np.testing.assert_array_equal(g, w, err_msg=k)


def check_assembly(c, got, partial, full):
    """fetch_problem of every stage that ran, the masks, the view counts and the "adjust" counts against the walk."""
    pm = None
    for stage, on in enumerate((partial, full)):
        if not on:
            continue
        cam_mut, pm = RR.masks(c, STAGES[stage], c["new_cam"], c["visible"], pt_mutable=pm)
        want = RR.gather(c, cam_mut, pm, WEIGHT[stage])
        same(got["problem"][stage], want, PROBLEM)
        assert got["adjust_cams"][stage] == int(cam_mut.sum()) and got["adjust_pts"][stage] == int(pm.sum())
        assert got["solved"][stage] == int(len(want["obs_cam"]) > 0)
        assert (got["summary"][stage] is not None) == bool(got["solved"][stage])
    same(got, dict(pt_mutable=c["pt_mutable"] if pm is None else pm, pt_views=RR.views(c)), ("pt_mutable", "pt_views"))
    return pm


def check_outliers(c, got, th=1.0):
    """The flags, pt_mse and the three counts against the walk on the cameras and points the call returned."""
    want = RR.remove_outliers(c, got["cam_R"], got["cam_t"], got["cam_fk"], th, point_xyz=got["point_xyz"])
    same(got, want, ("pt_mse", "pt_bad", "pt_new_added"))
    for k in ("count_outliers", "count_new_add", "count_outliers_new_add"):
        assert got[k] == want[k], (k, got[k], want[k])
    return want


def test_assembly_is_the_walk(ctx, main):
    c = main
    got = run(ctx, c, partial=True, full=True, outliers=False, keep_problem=1, partial_options=dict(max_num_iterations=3),
              full_options=dict(max_num_iterations=3))
    pm = check_assembly(c, got, True, True)
    assert got["solved"].tolist() == [1, 1] and got["adjust_cams"].tolist() == [len(D.MAIN_FREE), 8]
    p0, p1 = got["problem"]
    assert 0 < len(p0["obs_cam"]) < len(p1["obs_cam"]) < len(c["obs_point"]) and len(p0["kept"]) < len(p1["kept"])
    assert p0["cam_mutable"].tolist() == [int(k in D.MAIN_FREE) for k in range(8)] and p1["cam_mutable"].all()
    assert not np.isin(c["tag"]["frozen_only"], p0["kept"]).any() and np.isin(c["tag"]["frozen_only"], p1["kept"]).all()
    assert np.isin(c["tag"]["unheld"], p0["kept"]).tolist() == [True, True, False, True]
    assert pm[c["tag"]["unheld"]].tolist() == [0, 1, 0, 1]
    # outliers off: the flags and pt_mse pass through
    same(got, c, ("pt_bad", "pt_mse", "pt_new_added"))
    assert got["count_outliers"] == got["count_new_add"] == 0 and got["h2d_bytes"] > 0


SIZES = {"255": lambda: D.sized_case(255), "256": lambda: D.sized_case(256), "257": lambda: D.sized_case(257),
         "rows257": lambda: D.sized_case(128, n_rows=257), "track70": D.long_track_case, "all_bad": lambda: D.sized_case(40, all_bad=True),
         "empty": D.empty_case, "no_rows": D.points_without_rows_case}


@pytest.mark.parametrize("name", list(SIZES))
def test_sizes(ctx, name):
    c = SIZES[name]()
    got = run(ctx, c, partial=True, full=True, outliers=True, keep_problem=1, partial_options=dict(max_num_iterations=2),
              full_options=dict(max_num_iterations=2))
    check_assembly(c, got, True, True)
    check_outliers(c, got)
    if name in ("255", "256", "257"):
        assert len(c["pt_bad"]) == int(name) and got["solved"].tolist() == [1, 1]
    if name == "rows257":
        assert len(c["obs_point"]) == 257 and len(got["problem"][1]["obs_cam"]) == 256
    if name == "track70":
        assert got["pt_views"][c["long"]] == 70 and got["pt_views"].max() == 70 and len(c["cam_img"]) == 72
        q = got["problem"][1]
        assert (q["obs_pt"] == np.nonzero(q["kept"] == c["long"])[0][0]).sum() == 70
    if name in ("all_bad", "empty"):
        assert got["solved"].tolist() == [0, 0] and got["summary"] == [None, None] and len(got["problem"][0]["obs_cam"]) == 0
        assert got["count_outliers"] == got["count_new_add"] == got["count_outliers_new_add"] == 0
        same(got, c, ("point_xyz", "pt_bad", "pt_mse", "pt_new_added", "cam_pose", "cam_model"))
    if name == "empty":
        assert len(c["obs_point"]) == 0 and len(got["pt_views"]) == 0
    if name == "no_rows":          # n_obs = 0 with points: every stage skipped, every live point's mse is 0 / 0 and it is no outlier
        live = c["pt_bad"] == 0
        assert len(c["obs_point"]) == 0 and len(c["pt_bad"]) == 300 and got["solved"].tolist() == [0, 0] and not got["pt_views"].any()
        assert np.isnan(got["pt_mse"][live]).all() and got["count_outliers"] == 0 and got["count_new_add"] == int(c["pt_new_added"][live].sum())
        same(got, c, ("pt_mutable", "pt_bad", "point_xyz"))


def public_solve(ctx, c, stage, pose, model, xyz, pm):
    """The stage through the public path: the walk's arrays into msfm_ba_solve."""
    cam_mut, pm = RR.masks(c, STAGES[stage], c["new_cam"], c["visible"], pt_mutable=pm)
    g = RR.gather(c, cam_mut, pm, WEIGHT[stage], point_xyz=xyz)
    arr = A.BaArrays(pose, model, c["cam_model_of_cam"], g["point"], g["obs_cam"], g["obs_pt"], g["obs_xy"], g["pt_weight"],
                     cam_mutable=g["cam_mutable"], pt_mutable=g["pt_mutable"])
    s = ctx.ba_solve(arr, capi.default_options(max_num_iterations=100))
    xyz = np.array(xyz)
    xyz[g["kept"]] = arr.point
    return s, arr.cam_pose, arr.cam_model, xyz, pm, g


def same_summary(got, want):
    for k in SUMMARY:
        assert got[k] == want[k], (k, got[k], want[k])
    np.testing.assert_array_equal(got["iterations"], want["iterations"])


@pytest.mark.parametrize("full", [False, True])
def test_solve_is_the_public_path(ctx, main, full):
    c = main
    got = run(ctx, c, partial=True, full=full, outliers=False)
    s0, pose, model, xyz, pm, g0 = public_solve(ctx, c, 0, c["cam_pose"], c["cam_model"], c["point_xyz"], None)
    same_summary(got["summary"][0], s0)
    assert s0["num_iterations"] >= 1 and s0["final_cost"] < s0["initial_cost"]
    # what the partial solve must not touch: points outside the problem, frozen points, frozen cameras
    out = np.ones(len(xyz), bool)
    out[g0["kept"][g0["pt_mutable"] != 0]] = False
    assert out.sum() > 10 and (g0["pt_mutable"] == 0).any()
    np.testing.assert_array_equal(xyz[out], c["point_xyz"][out])
    np.testing.assert_array_equal(pose[D.MAIN_FROZEN], c["cam_pose"][D.MAIN_FROZEN])
    assert (pose[D.MAIN_FREE] != c["cam_pose"][D.MAIN_FREE]).any() and (xyz[~out] != c["point_xyz"][~out]).any()
    if full:
        s1, pose, model, xyz, pm, _ = public_solve(ctx, c, 1, pose, model, xyz, pm)   # from the partial stage's result
        same_summary(got["summary"][1], s1)
        assert got["summary"][1]["initial_cost"] != got["summary"][0]["initial_cost"]
    else:
        assert got["summary"][1] is None and got["solved"].tolist() == [1, 0]
        np.testing.assert_array_equal(got["point_xyz"][out], c["point_xyz"][out])
        np.testing.assert_array_equal(got["cam_pose"][D.MAIN_FROZEN], c["cam_pose"][D.MAIN_FROZEN])
    same(got, dict(cam_pose=pose, cam_model=model, point_xyz=xyz, pt_mutable=pm), ("cam_pose", "cam_model", "point_xyz", "pt_mutable"))


def test_outliers_bit_for_bit(ctx):
    c = D.outlier_case()
    tag = c["tag"]
    got = run(ctx, c, partial=False, full=False, outliers=True)
    want = check_outliers(c, got)
    assert got["solved"].tolist() == [0, 0]
    same(got, c, ("point_xyz", "cam_pose", "cam_model", "pt_mutable"))
    # the cameras as Camera::UpdatePoseFromData keeps them; two sin / cos implementations differ by a few ulp of entries <= 1
    R, t, cc, fk = scene.cameras_for_tracks(types.SimpleNamespace(cam_model_of_cam=c["cam_model_of_cam"]), pose=c["cam_pose"], model=c["cam_model"])
    np.testing.assert_allclose(got["cam_R"].reshape(-1, 9), R, rtol=0, atol=1e-14)
    np.testing.assert_array_equal(got["cam_t"], c["cam_pose"][:, 3:])
    np.testing.assert_allclose(got["cam_c"], cc, rtol=0, atol=1e-12)
    np.testing.assert_array_equal(got["cam_fk"], fk)
    assert got["pt_mse"][tag["behind_second"]] == 100000.0 == got["pt_mse"][tag["behind_first"]]
    assert got["pt_bad"][[tag["behind_second"], tag["behind_first"]]].all()
    for k in ("nan", "no_rows"):
        assert np.isnan(got["pt_mse"][tag[k]]) and got["pt_bad"][tag[k]] == 0 and got["pt_new_added"][tag[k]] == 0
    assert got["pt_new_added"][tag["bad"]].tolist() == [1, 0] and got["pt_mse"][tag["bad"]].tolist() == c["pt_mse"][tag["bad"]].tolist()
    root = np.sqrt(got["pt_mse"][tag["spread"]])
    assert (root < 1.0).sum() >= 10 and (root > 1.0).sum() >= 10 and got["count_outliers"] == int(want["pt_bad"].sum() - c["pt_bad"].sum())
    # another threshold moves the flags with it
    got = run(ctx, c, partial=False, full=False, outliers=True, th_mse_outliers=2.5)
    check_outliers(c, got, th=2.5)
    assert got["count_outliers"] < want["count_outliers"]


def test_the_whole_call_after_a_solve(ctx, main):
    c = main
    got = run(ctx, c, partial=True, full=False, outliers=True, keep_problem=1)
    check_assembly(c, got, True, False)
    want = check_outliers(c, got)
    assert 0 < got["count_outliers"] < int((c["pt_bad"] == 0).sum()) and got["count_outliers_new_add"] > 0
    assert (got["point_xyz"] != c["point_xyz"]).any() and (got["pt_mse"][c["pt_bad"] == 0] != c["pt_mse"][c["pt_bad"] == 0]).all()
    np.testing.assert_array_equal(got["pt_mse"][c["pt_bad"] != 0], c["pt_mse"][c["pt_bad"] != 0])
    assert want["pt_bad"][c["pt_bad"] != 0].all()
    # the host-side pair: the same call on a state dict, written back in place
    state = {k: np.array(c[k]) for k in D.STATE}
    store = ctx.match_store(*D.store_args(c))
    try:
        r = adjust.adjust_round(ctx, store, state, c["cam_pose"], c["cam_model"], c["cam_model_of_cam"], c["new_cam"], c["visible"],
                                keypoints=c["keypoints"])
    finally:
        store.close()
    pose, model = adjust.apply_round(state, r)
    same(state, got, ("point_xyz", "pt_bad", "pt_mse", "pt_mutable", "pt_new_added", "cam_R", "cam_t", "cam_c", "cam_fk"))
    same(dict(cam_pose=pose, cam_model=model), got, ("cam_pose", "cam_model"))


def refused(ctx, c, store=None, **kw):
    with pytest.raises(capi.MsfmError) as e:
        run(ctx, c, store, **kw)
    assert e.value.code == A.MSFM_E_INVAL, e.value
    return str(e.value)


def test_refusals(ctx, main):
    c = main
    n_cams, n_points = len(c["cam_img"]), len(c["pt_bad"])
    store = ctx.match_store(*D.store_args(c))
    fo = np.concatenate([[0], np.cumsum(c["n_features"][c["cam_img"]])])

    def edited(key, at, value):
        d = dict(c)
        d[key] = np.array(c[key])
        d[key][at] = value
        return d
    quick = dict(partial_options=dict(max_num_iterations=1))
    # an index outside its array, found on the device
    assert "feat_point of camera 3, feature 2" in refused(ctx, edited("feat_point", fo[3] + 2, n_points), store, **quick)
    for key, value in (("obs_point", n_points), ("obs_point", -1), ("obs_cam", n_cams), ("obs_cam", -2),
                       ("obs_feat", int(c["n_features"][c["cam_img"][c["obs_cam"][17]]])), ("obs_feat", -1)):
        assert "observation 17" in refused(ctx, edited(key, 17, value), store, **quick)
        assert "observation 17" in refused(ctx, edited(key, 17, value), store, partial=False, full=False)   # (found at the final wait)
    # cameras
    assert "new_cam" in refused(ctx, c, store, new_cam=n_cams)
    assert "visible[1]" in refused(ctx, c, store, visible=[7, n_cams])
    assert "visible[0]" in refused(ctx, c, store, visible=[-1])
    assert "do_partial without new_cam" in refused(ctx, c, store, new_cam=-1)
    assert "no image of the store" in refused(ctx, edited("cam_img", 2, len(c["n_features"])), store)
    twice = edited("cam_img", 1, c["cam_img"][0])
    twice["feat_point"] = np.full(int(c["n_features"][twice["cam_img"]].sum()), -1, np.int32)
    assert "two cameras" in refused(ctx, twice, store)
    assert "cam_model_of_cam" in refused(ctx, edited("cam_model_of_cam", 4, 2), store)
    # keypoints: this store was not made from a chain
    assert "no keypoints of image" in refused(ctx, c, store, keypoints=None)
    # thresholds
    for th in (np.nan, -1.0):
        assert "th_mse_outliers" in refused(ctx, c, store, th_mse_outliers=th)
    assert "weight" in refused(ctx, c, store, weight_partial=np.nan)
    # a key that does not fit: 65537 cameras (17 bits) and an image of 65536 features (16 bits); one camera less fits
    def wide(n):
        nf = np.ones(n, np.int32)
        nf[0] = 65536
        total = int(nf.sum())
        return dict(n_features=nf, keypoints=np.zeros((total, 2), np.float32), cam_img=np.arange(n, dtype=np.int32),
                    feat_point=np.full(total, -1, np.int32), obs_point=np.zeros(0, np.int32), obs_cam=np.zeros(0, np.int32),
                    obs_feat=np.zeros(0, np.int32), cam_pose=np.zeros((n, 6)), cam_model=np.array([[D.F, 0.0, 0.0]]),
                    cam_model_of_cam=np.zeros(n, np.int32), point_xyz=np.zeros((0, 3)), pt_bad=np.zeros(0, np.uint8), pt_mse=np.zeros(0),
                    pt_mutable=np.zeros(0, np.uint8), pt_new_added=np.zeros(0, np.uint8), new_cam=0, visible=np.array([0], np.int32))
    assert "17 + 16 bits" in refused(ctx, wide(65537))
    assert run(ctx, wide(65536))["solved"].tolist() == [0, 0]
    # the context still answers
    got = run(ctx, c, store, partial=True, outliers=True, keep_problem=1)
    check_assembly(c, got, True, False)
    check_outliers(c, got)
    store.close()
