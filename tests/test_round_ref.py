"""tests/round_ref.py - the literal walk tests/test_gpu_round.py holds msfm_round_adjust to - against the project's own window
selection (metricsfm_amd/window.py) on a Scene; what the state helpers do with the point side of the flat state; and the margins
the seeded cases of tests/round_data.py must keep."""
import types

import numpy as np
import pytest

from metricsfm_amd import adjust, localize, newpoints, scene, window
from tests import round_data as D
from tests import round_ref as RR


@pytest.fixture(scope="module")
def sc():
    s = scene.make_aerial_scene(40, 800, seed=31, n_models=20)
    s.obs_xy = s.obs_xy.astype(np.float32).astype(np.float64)      # the state keeps keypoints as floats
    return s


def _bad(s):
    bad = np.zeros(s.n_points, bool)
    bad[np.random.default_rng(2).choice(s.n_points, 40, replace=False)] = True
    return bad


def _same_problem(got, arr, kept):
    np.testing.assert_array_equal(got["kept"], kept)
    np.testing.assert_array_equal(got["obs_cam"], arr.obs_cam)
    np.testing.assert_array_equal(got["obs_pt"], arr.obs_pt)
    np.testing.assert_array_equal(got["obs_xy"], arr.obs_xy)
    np.testing.assert_array_equal(got["pt_weight"], arr.pt_weight)
    np.testing.assert_array_equal(got["point"], arr.point)


def test_partial_problem_is_the_window_modules(sc):
    bad = _bad(sc)
    st = D.scene_state(sc, bad)
    for idx in (0, 17, 39):
        arr, info = window.partial_bundle_adjustment_problem(sc, idx, bad, compact=True)
        cam_mut, pt_mut = RR.masks(st, "partial", idx, info["visible"])
        got = RR.gather(st, cam_mut, pt_mut, window.PARTIAL_WEIGHT)
        assert 0 < len(info["kept"]) and len(arr.obs_cam) < int((~bad)[sc.obs_pt].sum())     # a window, not the whole scene
        _same_problem(got, arr, info["kept"])
        np.testing.assert_array_equal(got["cam_mutable"], arr.cam_mutable)
        np.testing.assert_array_equal(got["pt_mutable"], arr.pt_mutable)
        seen = np.bincount(sc.obs_pt, minlength=sc.n_points) > 0
        np.testing.assert_array_equal(pt_mut[seen], info["pt_mutable"][seen])


def test_full_problem_is_the_window_modules(sc):
    bad = _bad(sc)
    st = D.scene_state(sc, bad)
    arr, kept = window.gather(sc, bad=bad, compact=True)
    cam_mut, pt_mut = RR.masks(st, "full")
    got = RR.gather(st, cam_mut, pt_mut, window.FULL_WEIGHT)
    _same_problem(got, arr, kept)
    assert cam_mut.all() and got["pt_mutable"].all() and arr.cam_mutable is None and arr.pt_mutable is None
    np.testing.assert_array_equal(RR.views(st), np.bincount(sc.obs_pt, minlength=sc.n_points))


def test_main_case_holds_what_it_is_for():
    c = D.main_case()
    tag = c["tag"]
    cam_mut, pt_mut = RR.masks(c, "partial", c["new_cam"], c["visible"])
    assert np.nonzero(cam_mut)[0].tolist() == D.MAIN_FREE
    g = RR.gather(c, cam_mut, pt_mut, 2.0)
    v = RR.views(c)
    assert {2, 3, 5} <= set(v.tolist()) and len(c["pt_bad"]) > 256 and len(c["obs_point"]) > 3 * 256
    assert len(np.unique(np.column_stack([c["obs_point"], c["obs_cam"], c["obs_feat"]]), axis=0)) == len(c["obs_point"]) - 4   # duplicate rows
    assert (np.diff(c["obs_point"]) < 0).any()                                               # rows in shuffled order
    assert not pt_mut[tag["frozen_only"]].any() and not np.isin(tag["frozen_only"], g["kept"]).any()
    for k in ("bad_inside", "bad_outside", "bad_far"):
        assert c["pt_bad"][tag[k]].all() and not pt_mut[tag[k]].any() and not np.isin(tag[k], g["kept"]).any()
    held = np.zeros(len(c["pt_bad"]), bool)
    held[c["feat_point"][c["feat_point"] >= 0]] = True
    assert not held[tag["unheld"]].any() and held[tag["takes1_failed"]].all() and held[tag["takes2_failed"]].all()
    # a point no camera holds keeps its incoming flag: rows on free cameras stay either way, rows on frozen ones only with the flag
    assert pt_mut[tag["unheld"]].tolist() == c["pt_mutable"][tag["unheld"]].tolist() == [0, 1, 0, 1]
    assert np.isin(tag["unheld"], g["kept"]).tolist() == [True, True, False, True]
    # the full stage frees what a camera holds, bad ones included, and leaves the others
    _, pt_full = RR.masks(c, "full", pt_mutable=pt_mut)
    assert pt_full[held].all() and pt_full[tag["unheld"]].tolist() == [0, 1, 0, 1]
    # key order is image order: some point's rows are not in camera index order
    cams_ = RR.point_side(c)
    assert any([cam for _, (cam, _) in sorted(m.items())] != sorted(cam for cam, _ in m.values()) for m in cams_)


def test_outlier_case_keeps_its_margin():
    c = D.outlier_case()
    tag = c["tag"]
    R = scene.angle_axis_to_R(c["cam_pose"][:, :3])
    r = RR.remove_outliers(c, R, c["cam_pose"][:, 3:], c["cam_model"][c["cam_model_of_cam"]])
    root = np.sqrt(r["pt_mse"])
    visited = c["pt_bad"] == 0
    assert np.nanmin(np.abs(root[visited] - 1.0)) >= 1e-6, "change SEED_OUTLIERS"
    sp = root[tag["spread"]]
    assert (sp < 1.0).sum() >= 10 and (sp > 1.0).sum() >= 10
    assert r["pt_mse"][tag["behind_second"]] == 100000.0 == r["pt_mse"][tag["behind_first"]] and r["pt_bad"][tag["behind_second"]] == 1
    assert r["pt_mse"][tag["back_view"]] < 1.0
    for k in ("nan", "no_rows"):
        assert np.isnan(r["pt_mse"][tag[k]]) and r["pt_bad"][tag[k]] == 0 and r["pt_new_added"][tag[k]] == 0
    np.testing.assert_array_equal(r["pt_mse"][tag["bad"]], c["pt_mse"][tag["bad"]])
    np.testing.assert_array_equal(r["pt_new_added"][tag["bad"]], c["pt_new_added"][tag["bad"]])
    assert c["pt_new_added"][tag["bad"]].tolist() == [1, 0] and not r["pt_new_added"][visited].any()
    assert r["count_new_add"] == int(c["pt_new_added"][visited].sum()) and 0 < r["count_outliers_new_add"] < r["count_outliers"]


# ---- the state helpers ----
def _loc_state():
    nf = np.array([4, 5, 6], np.int32)
    st = dict(n_features=nf, cam_img=np.array([0, 2], np.int32), feat_point=np.array([0, 1, -1, 2, 0, -1, 1, 2, -1, -1], np.int32),
              cam_R=np.array([np.eye(3)] * 2), cam_t=np.zeros((2, 3)), cam_c=np.zeros((2, 3)), cam_fk=np.array([[1000.0, 0, 0]] * 2),
              point_xyz=np.arange(9.0).reshape(3, 3), pt_bad=np.zeros(3, np.uint8), pt_mse=np.array([0.1, 0.2, 0.3]),
              pt_views=np.full(3, 2, np.int32))
    side = dict(obs_point=np.array([0, 0, 1, 1, 2, 2], np.int32), obs_cam=np.array([0, 1, 0, 1, 0, 1], np.int32),
                obs_feat=np.array([0, 0, 1, 2, 3, 3], np.int32), pt_mutable=np.ones(3, np.uint8))
    res = dict(image=1, R=np.eye(3), t=np.array([1.0, 2.0, 3.0]), f=900.0, visible=[0, 1], corr_feat=np.array([4, 0, 2, 3]),
               corr_point=np.array([2, 0, 1, 0]), corr_state=np.array([2, 1, 2, 0]))
    return st, side, res


def _new_points():
    return newpoints.NewPoints(X=np.array([[1.0, 2, 3], [4, 5, 6], [7, 8, 9]]), mse=np.array([0.5, 1.5, 2.5]), cam2=np.array([0, 1, 0], np.int32),
                               feat1=np.array([1, 1, 3], np.int32), feat2=np.array([2, 5, 2], np.int32), takes1=np.array([1, 0, 1], np.uint8),
                               takes2=np.array([1, 1, 0], np.uint8))


def _equal_states(a, b, keys):
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k


def test_state_helpers_append_the_point_side():
    st, side, res = _loc_state()
    st.update({k: v.copy() for k, v in side.items()})
    vis = localize.apply_localized_image(st, res)
    assert vis == [2, 0, 1]
    # one row per state-2 correspondence, in correspondence order: (point 2, feature 4), (point 1, feature 2)
    assert st["obs_point"].tolist() == side["obs_point"].tolist() + [2, 1]
    assert st["obs_cam"].tolist() == side["obs_cam"].tolist() + [2, 2] and st["obs_feat"].tolist() == side["obs_feat"].tolist() + [4, 2]
    assert st["pt_mutable"].tolist() == [1, 1, 1] and all(st[k].dtype == np.int32 for k in ("obs_point", "obs_cam", "obs_feat"))
    ids = newpoints.apply_new_points(st, _new_points())
    assert ids.tolist() == [3, 4, 5]
    # two rows per new point, the new camera's first, whether or not the camera-side inserts took
    assert st["obs_point"][8:].tolist() == [3, 3, 4, 4, 5, 5] and st["obs_cam"][8:].tolist() == [2, 0, 2, 1, 2, 0]
    assert st["obs_feat"][8:].tolist() == [1, 2, 1, 5, 3, 2]
    assert st["pt_mutable"].tolist() == [1] * 6 and st["pt_mutable"].dtype == np.uint8
    fo = 4 + 6
    assert st["feat_point"][fo + 1] == 3 and st["feat_point"][2] == 3 and st["feat_point"][4 + 5] == 4 and st["feat_point"][fo + 3] == 5
    assert (st["feat_point"] == 5).sum() == 1          # takes2 of the third point failed: an observation, no camera-side entry


def test_state_helpers_leave_a_state_without_the_keys_alone():
    with_keys, side, res = _loc_state()
    with_keys.update({k: v.copy() for k, v in side.items()})
    without, _, _ = _loc_state()
    for st in (with_keys, without):
        localize.apply_localized_image(st, res)
        newpoints.apply_new_points(st, _new_points())
    assert not set(adjust.POINT_SIDE) & set(without)
    assert set(with_keys) - set(without) == set(adjust.POINT_SIDE)
    _equal_states(without, with_keys, sorted(without))


def test_point_side_from_seed():
    seed = dict(point=np.zeros((3, 3)), obs_cam=np.tile(np.array([0, 1], np.int32), 3), obs_pt=np.repeat(np.arange(3, dtype=np.int32), 2),
                obs_feature=np.array([7, 1, 8, 2, 9, 3], np.int32))
    side = adjust.point_side_from_seed(seed)
    assert sorted(side) == sorted(adjust.POINT_SIDE)
    assert side["obs_point"].tolist() == [0, 0, 1, 1, 2, 2] and side["obs_cam"].tolist() == [0, 1] * 3
    assert side["obs_feat"].tolist() == [7, 1, 8, 2, 9, 3] and side["pt_mutable"].tolist() == [1, 1, 1]
    with pytest.raises(ValueError):
        adjust.point_side_from_seed(dict(point=np.zeros((1, 3))))


def test_a_round_of_state_helpers_reaches_the_library_call():
    """apply_localized_image -> apply_new_points -> adjust_round: every array of the state keeps one entry per point, so the
    argument checks of Context.round_adjust pass and the library is called (here with no context, which it refuses)."""
    from metricsfm_amd import _abi as A
    from metricsfm_amd import capi

    class Reached(Exception):
        pass

    class NoContext:
        _h = None

        def check(self, rc):
            raise Reached(rc)

        round_adjust = capi.Context.round_adjust

    st, side, res = _loc_state()
    st.update({k: v.copy() for k, v in side.items()})
    visible = localize.apply_localized_image(st, res)
    newpoints.apply_new_points(st, _new_points())
    n = len(st["pt_mse"])
    assert n == 6 and all(len(st[k]) == n for k in ("point_xyz", "pt_bad", "pt_views", "pt_mutable", "pt_new_added"))
    assert st["pt_new_added"].tolist() == [0, 1, 1, 1, 1, 1] and st["pt_new_added"].dtype == np.uint8     # state-2 points, then the new ones
    store = types.SimpleNamespace(_h=None, n_features=st["n_features"])
    with pytest.raises(Reached) as e:
        adjust.adjust_round(NoContext(), store, st, np.zeros((3, 6)), [[1000.0, 0.0, 0.0]], [0, 0, 0], visible[0], visible,
                            keypoints=np.zeros((15, 2), np.float32))
    assert e.value.args[0] == A.MSFM_E_INVAL
    # without pt_new_added the new points do not create it
    bare, _, _ = _loc_state()
    newpoints.apply_new_points(bare, _new_points(), new_cam=1)
    assert "pt_new_added" not in bare
