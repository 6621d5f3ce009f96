"""The SLAM + GPS registration steps on the resident chain (msfm_chain_accuracy / _gps_register / _ba_create_gps /
_store_points) against the host-array calls on the fetched arrays, and metricsfm_amd.gpsreg.slam_gps_register against the same
steps composed by hand.

One scene: 16 images x 2048 features of scene.add_features(scene.make_aerial_scene(16, 3000)), every ordered pair matched, with
a GPS track planted on the true camera centres as in tests/gpsreg_data.py (scale 3.7, a general rotation, a translation of
4e5, 0.3 units of noise).  The verification gates leave well over 200 tracks with >= 3 views at this size (asserted), so
config 2's shape is not needed."""
import numpy as np
import pytest

from metricsfm_amd import _abi as A
from metricsfm_amd import capi, gpsreg, scene, window
from tests import gpsreg_data as D

pytestmark = pytest.mark.gpu

SEED = 0x4D53464D
ITER = 12       # iterations of the adjustments here (the driver's default is the reference's 200)


@pytest.fixture(scope="module")
def world(ctx):
    sc = scene.add_features(scene.make_aerial_scene(16, 3000, seed=77, name="gpsreg"), 2048)
    kps = [np.ascontiguousarray(k, np.float32) for k in sc.kp_xy]
    ds = ctx.descset(sc.desc, keypoints=kps)
    res = ds.match_pairs(scene.all_pairs(sc.n_cams), 0.6, 0.85)
    R, t, c, fk = scene.cameras_for_tracks(sc)      # the model in its own frame: the true cameras
    gps = D.PLANTED_SCALE * c @ D.rodrigues(D.PLANTED_AA).T + D.PLANTED_T + np.random.default_rng(9).normal(0, D.GPS_NOISE, c.shape)
    w = dict(sc=sc, kps=kps, ds=ds, res=res, R=R, c=c, fk=fk, gps=gps, model=sc.cam_model_gt.copy(), moc=sc.cam_model_of_cam)
    yield w
    res.close(); ds.close()


def _chain(w):
    ch = capi.Chain(w["res"])
    ch.verify(3.0, seed=SEED)
    ch.build_tracks()
    return ch


@pytest.fixture(scope="module")
def manual(ctx, world):
    """slam_gps.cc:98-119 step by step on a chain, every intermediate fetched."""
    w = world
    ch = _chain(w)
    m = dict(ch=ch)
    m["off"], m["img"], feat = ch.fetch_tracks()
    m["xy"] = np.array([w["kps"][i][f] for i, f in zip(m["img"], feat)], dtype=np.float64).reshape(-1, 2)
    o = m["o"] = capi.gps_orient_global(w["R"], w["c"], w["gps"])
    m["n_accepted"] = ch.triangulate(o["cam_R"], o["cam_t"], o["cam_c"], w["fk"], gpsreg.TH_OUTLIER, gpsreg.TH_TRI_ANGLE)
    m["tri"] = tuple(x.copy() for x in ch.fetch_points())
    m["acc1_counts"] = ch.accuracy(o["cam_R"], o["cam_t"], w["fk"])
    m["acc1"] = tuple(x.copy() for x in ch.fetch_accuracy())
    m["pts1"] = tuple(x.copy() for x in ch.fetch_points())
    ch.gps_register(o["cam_c"], o["gps"])
    m["pts2"] = tuple(x.copy() for x in ch.fetch_points())
    _, _, m["pose"] = gpsreg.set_ac_pose(o["cam_aa"], o["gps"])
    opts = capi.default_options(max_num_iterations=ITER)
    ba = m["ba"] = ch.ba_create(m["pose"], w["model"], w["moc"], gps_xyz=o["gps"])
    m["summary"] = ba.run(opts)
    m["adjusted"] = ba.download()
    ch.store_points(ba)
    m["pts3"] = tuple(x.copy() for x in ch.fetch_points())
    R2, t2 = gpsreg.pose_cameras(m["adjusted"][0])
    m["cams2"] = (R2, t2, m["adjusted"][1][w["moc"]])
    m["acc2_counts"] = ch.accuracy(*m["cams2"])
    m["acc2"] = tuple(x.copy() for x in ch.fetch_accuracy())
    m["pts4"] = tuple(x.copy() for x in ch.fetch_points())
    yield m
    ba.close(); ch.close()


def test_every_chain_step_is_its_host_array_call(ctx, world, manual):
    w, m, o = world, manual, manual["o"]
    off, img, xy = m["off"], m["img"], m["xy"]
    lens = np.diff(off)
    assert int(((m["tri"][2] != 0) & (lens >= 3)).sum()) >= 200
    tr = A.TrackArrays(off, img, xy, o["cam_R"], o["cam_t"], o["cam_c"], w["fk"])
    X0, mse0, ok0 = ctx.triangulate_midpoint(tr, gpsreg.TH_OUTLIER, gpsreg.TH_TRI_ANGLE)
    for g, h in zip(m["tri"], (X0, mse0, ok0)):
        np.testing.assert_array_equal(g, h)
    # GetAccuracy: ok_out lands in the chain's ok, X and mse stay
    e_avg, e_mse, used, ok1, n_out, n_in = ctx.point_accuracy(tr, X0, ok0)
    assert m["acc1_counts"] == (n_out, n_in) and n_out + n_in == len(lens)
    for g, h in zip(m["acc1"], (e_avg, e_mse, used)):
        np.testing.assert_array_equal(g, h)
    np.testing.assert_array_equal(m["pts1"][0], X0); np.testing.assert_array_equal(m["pts1"][1], mse0); np.testing.assert_array_equal(m["pts1"][2], ok1)
    assert 0 < ok1.sum() < ok0.sum()      # (two-view tracks at least go)
    # GPSRegistration2
    X2 = ctx.gps_register_points(off, img, ok1, o["cam_c"], o["gps"], X0)
    np.testing.assert_array_equal(m["pts2"][0], X2); np.testing.assert_array_equal(m["pts2"][2], ok1)
    assert np.abs(X2 - X0)[ok1 != 0].max() > 0 and (X2[ok1 == 0] == X0[ok1 == 0]).all()
    # FullBundleAdjustment with the GPS rows against msfm_ba_solve on the same arrays
    keep = (ok1 != 0) & (lens >= 3)
    kept = np.nonzero(keep)[0]
    ba = m["ba"]
    np.testing.assert_array_equal(ba.track_of_point, kept)
    obs_sel = np.repeat(keep, lens)
    n_obs = int(obs_sel.sum())
    assert ba.n_obs == n_obs and ba.gps_weight_used == window.gps_weight(n_obs, w["sc"].n_cams) > 0
    arrays = A.BaArrays(m["pose"].copy(), w["model"].copy(), w["moc"], X2[keep].copy(), img[obs_sel],
                        np.repeat(np.cumsum(keep) - 1, lens)[obs_sel].astype(np.int32), xy[obs_sel], np.ones(len(kept)),
                        gps_xyz=o["gps"], gps_weight=window.gps_weight(n_obs, w["sc"].n_cams))
    r_h = ctx.ba_solve(arrays, capi.default_options(max_num_iterations=ITER))
    r = m["summary"]
    assert r["num_iterations"] == r_h["num_iterations"] and r["num_residuals"] == r_h["num_residuals"] > 2 * n_obs
    for k in r["iterations"].dtype.names:
        np.testing.assert_array_equal(r["iterations"][k], r_h["iterations"][k], err_msg=k)
    cam_d, model_d, pt_d = m["adjusted"]
    np.testing.assert_array_equal(cam_d, arrays.cam_pose); np.testing.assert_array_equal(pt_d, arrays.point); np.testing.assert_array_equal(model_d, arrays.cam_model)
    assert r["final_cost"] < r["initial_cost"]
    # store_points: the adjusted points scattered by track_of_point, every other track unchanged
    X3 = X2.copy()
    X3[kept] = pt_d
    np.testing.assert_array_equal(m["pts3"][0], X3); np.testing.assert_array_equal(m["pts3"][2], ok1)
    assert (X3[kept] != X2[kept]).any()
    # the second GetAccuracy, with the adjusted cameras
    R2, t2, fk2 = m["cams2"]
    tr2 = A.TrackArrays(off, img, xy, R2, t2, o["cam_c"], fk2)
    e_avg, e_mse, used, ok4, n_out, n_in = ctx.point_accuracy(tr2, X3, ok1)
    assert m["acc2_counts"] == (n_out, n_in)
    for g, h in zip(m["acc2"], (e_avg, e_mse, used)):
        np.testing.assert_array_equal(g, h)
    np.testing.assert_array_equal(m["pts4"][0], X3); np.testing.assert_array_equal(m["pts4"][2], ok4)


def test_ba_create_without_gps_is_unchanged(ctx, world, manual):
    """msfm_chain_ba_create shares its body with the GPS form: on a second chain it gives what the host-array path gives, by the
    assertions of test_gpu_chain.py::test_config2_chain_matches_the_host_array_path."""
    w, o = world, manual["o"]
    ch = _chain(w)
    ch.triangulate(o["cam_R"], o["cam_t"], o["cam_c"], w["fk"], 7.0, np.deg2rad(3.0))
    X_h, _, tok_h = ch.fetch_points()
    off_h, img_h, xy = manual["off"], manual["img"], manual["xy"]
    opts = capi.default_options(max_num_iterations=8)
    ba = ch.ba_create(manual["pose"], w["model"], w["moc"], min_views=3, weight_ge3=1.0)
    assert not hasattr(ba, "gps_weight_used")
    r = ba.run(opts)
    cam_d, model_d, pt_d = ba.download()
    keep = (tok_h != 0) & (np.diff(off_h) >= 3)
    kept = np.nonzero(keep)[0]
    np.testing.assert_array_equal(ba.track_of_point, kept)
    obs_sel = np.repeat(keep, np.diff(off_h))
    new_pt = np.cumsum(keep) - 1
    arrays = A.BaArrays(manual["pose"].copy(), w["model"].copy(), w["moc"], X_h[keep].copy(), img_h[obs_sel],
                        np.repeat(new_pt, np.diff(off_h))[obs_sel].astype(np.int32), xy[obs_sel], np.ones(len(kept)))
    r_h = ctx.ba_solve(arrays, opts)
    assert r["num_iterations"] == r_h["num_iterations"] and r["num_residuals"] == r_h["num_residuals"] == 2 * int(obs_sel.sum())
    np.testing.assert_array_equal(r["iterations"]["cost"], r_h["iterations"]["cost"])
    np.testing.assert_array_equal(cam_d, arrays.cam_pose); np.testing.assert_array_equal(pt_d, arrays.point); np.testing.assert_array_equal(model_d, arrays.cam_model)
    assert r["final_cost"] < r["initial_cost"]
    # a problem of another chain is not this chain's to store
    with pytest.raises(capi.MsfmError) as e:
        ch.store_points(manual["ba"])
    assert e.value.code == A.MSFM_E_INVAL
    np.testing.assert_array_equal(ch.fetch_points()[0], X_h)
    ch.store_points(ba)
    X3 = X_h.copy()
    X3[kept] = pt_d
    np.testing.assert_array_equal(ch.fetch_points()[0], X3)
    ba.close(); ch.close()


def test_calls_out_of_order_are_refused(ctx, world):
    ch = _chain(world)
    o = capi.gps_orient_global(world["R"], world["c"], world["gps"])
    for call in (lambda: ch.accuracy(o["cam_R"], o["cam_t"], world["fk"]), lambda: ch.gps_register(o["cam_c"], o["gps"]), ch.fetch_accuracy):
        with pytest.raises(capi.MsfmError) as e:     # before the triangulation
            call()
        assert e.value.code == A.MSFM_E_INVAL
    ch.triangulate(o["cam_R"], o["cam_t"], o["cam_c"], world["fk"], 3.0, gpsreg.TH_TRI_ANGLE)
    with pytest.raises(capi.MsfmError):
        ch.fetch_accuracy()                          # before the first msfm_chain_accuracy
    with pytest.raises(capi.MsfmError):
        ch.accuracy(o["cam_R"][:3], o["cam_t"][:3], world["fk"][:3])     # fewer cameras than images
    ch.close()


def test_the_driver_returns_the_steps_composed_by_hand(ctx, world, manual):
    w, m = world, manual
    ch = _chain(w)
    rec = gpsreg.slam_gps_register(ch, w["R"], w["c"], w["model"], w["moc"], w["gps"], options=capi.default_options(max_num_iterations=ITER))
    o = m["o"]
    for k in ("scale", "err", "offset", "Rg", "tg", "weight", "gps"):
        np.testing.assert_array_equal(rec[k], o[k], err_msg=k)
    assert rec["n_accepted"] == m["n_accepted"]
    assert (rec["n_outliers"], rec["n_inliers"]) == m["acc1_counts"] and (rec["n_outliers_adjusted"], rec["n_inliers_adjusted"]) == m["acc2_counts"]
    assert rec["gps_weight_used"] == m["ba"].gps_weight_used and rec["n_points"] == len(m["ba"].track_of_point) and rec["n_obs"] == m["ba"].n_obs
    for k in ("termination", "num_iterations", "initial_cost", "final_cost", "num_residuals"):
        assert rec["summary"][k] == m["summary"][k], k
    np.testing.assert_array_equal(rec["summary"]["iterations"]["cost"], m["summary"]["iterations"]["cost"])
    np.testing.assert_array_equal(rec["cam_pose"], m["adjusted"][0]); np.testing.assert_array_equal(rec["cam_model"], m["adjusted"][1])
    for g, h in zip(ch.fetch_points(), m["pts4"]):
        np.testing.assert_array_equal(g, h)
    for g, h in zip(ch.fetch_accuracy(), m["acc2"]):
        np.testing.assert_array_equal(g, h)
    assert rec["summary"]["final_cost"] < rec["summary"]["initial_cost"]
    rec["ba"].close(); ch.close()
