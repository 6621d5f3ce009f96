"""The SLAM arm of the resident chain (msfm_chain_create on a msfm_match_pairs_slam result + msfm_chain_verify_slam, the tail of
SLAMGPS::FeatureMatching step 2, slam_gps.cc:503-541): planted pairs against the sequential restatement of
tests/slam_chain_ref.py bit for bit, the planted SLAM scene end to end against the host-array composition of the same calls,
metricsfm_amd.slam against the calls made by hand, the match store, the refusals and the C++ host mirror."""
import os
import subprocess

import numpy as np
import pytest

from metricsfm_amd import _abi as A
from metricsfm_amd import capi, gpsreg, matchfiles, scene, slam
from tests import gpsreg_data as D
from tests import slam_chain_ref as R
from tests.localize_ref import localize_ref
from tests.slam_scene import planted_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x4D53464D46
N_CAMS = 16
ITER = 12


# ---------------------------------------------------------------------------------------------------------------------
# planted pairs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted():
    pl = R.planted_pairs()
    return pl, R.planted_reference(pl, seed=SEED)


def _planted_result(ctx, pl):
    ds = ctx.descset(pl["descs"], keypoints=[k if len(k) else None for k in pl["kps"]])
    res = ds.match_pairs_slam(pl["pairs"], pl["F"], pl["H"], th_first_second_ratio=R.TH_RATIO, th_epipolar=R.LOOSE, th_distance=R.LOOSE)
    return ds, res


def test_chain_takes_a_slam_result(ctx, planted):
    """msfm_chain_create refused the SLAM form before this arm existed."""
    pl, _ = planted
    ds, res = _planted_result(ctx, pl)
    ch = capi.Chain(res)
    assert ch.slam and ch.n_pairs == len(pl["pairs"])
    ch.close(); res.close(); ds.close()


def test_planted_pairs_equal_the_restatement(ctx, planted):
    """Query counts 0, 1, 255, 256, 257, 600; survivor counts 0, 1, 29, 30, 31, 40, 200; survivors only in the last 256-chunk;
    >= 30 survivors with 1..29 inliers (ok = 0, matches kept); ok = 1; an empty pair between two full ones; images that are train
    in one pair and query in another (tests/test_slam_chain_ref.py asserts that all of these occur)."""
    pl, ref = planted
    ds, res = _planted_result(ctx, pl)
    na, _ = res.counts()
    for p in range(len(pl["pairs"])):
        np.testing.assert_array_equal(res.fetch(p)[0][:len(ref["codes"][p])], ref["codes"][p], err_msg="codes of pair %d" % p)
    np.testing.assert_array_equal(na, pl["want"])
    ch = capi.Chain(res)
    n_m, ok, F = ch.verify_slam(seed=SEED)
    np.testing.assert_array_equal(n_m, ref["n_matches"])
    np.testing.assert_array_equal(ok, ref["ok"])
    np.testing.assert_array_equal(F, ref["F"])
    assert ((ok == 0) & (n_m > 0)).any()
    for p in range(len(pl["pairs"])):
        np.testing.assert_array_equal(ch.fetch_matches(p), ref["kept"][p], err_msg="matches of pair %d" % p)
    nt, no = ch.build_tracks()
    off, img, feat = ch.fetch_tracks()
    for g, h in zip((off, img, feat), ref["tracks"]):
        np.testing.assert_array_equal(g, h)
    assert nt == len(ref["tracks"][0]) - 1 and no == len(ref["tracks"][1])
    ch.close(); res.close(); ds.close()


def test_refusals_leave_the_chain_usable(ctx, planted):
    pl, ref = planted
    ds, res = _planted_result(ctx, pl)
    other = ds.match_pairs_slam(pl["pairs"], pl["F"], pl["H"], th_first_second_ratio=R.TH_RATIO, th_epipolar=R.LOOSE, th_distance=R.LOOSE)
    usable = [(0, 1), (0, 2), (0, 4), (1, 0), (2, 1), (4, 1)]                      # pairs whose images all have features
    plain = ds.match_pairs(np.array(usable, np.int32), 0.6, 0.85)

    def refused(call, *words):
        with pytest.raises(capi.MsfmError) as e:
            call()
        assert e.value.code == A.MSFM_E_INVAL
        for w in words:
            assert w in str(e.value), (w, str(e.value))

    ch = capi.Chain(res)
    refused(lambda: ch.verify(3.0, seed=SEED), "msfm_chain_verify_slam")          # the other form's call
    refused(lambda: ch.verify_slam(res=other, seed=SEED), "not the match result")   # a result the chain was not made from
    refused(lambda: ch.verify_slam(res=plain, seed=SEED), "not the match result")
    refused(lambda: ch.verify_slam(max_iterations=0), "bad options")
    refused(lambda: ch.verify_slam(max_iterations=65537), "bad options")
    refused(lambda: ch.verify_slam(threshold=0.0), "bad options")
    refused(ch.build_tracks)                                                       # nothing above has verified it
    n_m, ok, F = ch.verify_slam(seed=SEED)                                          # ... and the chain is intact
    np.testing.assert_array_equal(n_m, ref["n_matches"]); np.testing.assert_array_equal(ok, ref["ok"]); np.testing.assert_array_equal(F, ref["F"])
    refused(lambda: ch.verify_slam(seed=SEED), "already done")
    refused(lambda: ch.verify(3.0, seed=SEED))
    np.testing.assert_array_equal(ch.fetch_matches(0), ref["kept"][0])
    assert ch.build_tracks()[0] == len(ref["tracks"][0]) - 1
    # a chain of the other form refuses msfm_chain_verify_slam and then verifies as before
    cp = capi.Chain(plain)
    assert not cp.slam
    refused(lambda: cp.verify_slam(seed=SEED), "msfm_chain_verify")
    n_p, ok_p, _ = cp.verify(3.0, seed=SEED)
    assert len(n_p) == len(usable) and ok_p[0] == 1 and n_p[0] >= 150
    cp.close(); ch.close(); plain.close(); other.close(); res.close(); ds.close()


# ---------------------------------------------------------------------------------------------------------------------
# the planted SLAM scene end to end
# ---------------------------------------------------------------------------------------------------------------------
def _host_path(ctx, res, pairs, kps, seed):
    """slam_gps.cc:503-541 + :565-635 through host arrays: the codes fetched, the survivors gathered on the host,
    msfm_fundamental_ransac_batch on all of them, kept by mask, msfm_tracks_build_device from host arrays."""
    surv = []
    for p in range(len(pairs)):
        code = res.fetch(p)[0]
        m = np.nonzero(code >= 0)[0]
        surv.append(np.column_stack([code[m] & A.MSFM_MATCH_ID_MASK, m]).astype(np.int32).reshape(-1, 2))
    off = np.concatenate([[0], np.cumsum([len(s) for s in surv])]).astype(np.int32)
    p1 = np.concatenate([kps[i][s[:, 0]] for (i, j), s in zip(pairs, surv)]); p2 = np.concatenate([kps[j][s[:, 1]] for (i, j), s in zip(pairs, surv)])
    F, inl, nin, ok = ctx.fundamental_ransac(off, p1, p2, seed=seed)
    fin = [surv[p][inl[off[p]:off[p + 1]] != 0] for p in range(len(pairs))]
    n_feat = np.array([len(k) for k in kps], np.int32)
    moff = np.concatenate([[0], np.cumsum([len(m) for m in fin])]).astype(np.int32)
    flat = (n_feat, A.as_c(pairs, np.int32), moff, A.as_c(np.concatenate(fin).reshape(-1, 2), np.int32))
    return F, ok, fin, moff, surv, ctx.build_tracks(None, None, None, flat=flat)


@pytest.fixture(scope="module")
def world(ctx):
    """tests/slam_scene.planted_scene(16) with 900 features per image; the steps of SLAMGPS::FeatureMatching made by hand with
    the thresholds of resize_ratio = 1 (2 px, 5 px: the scene's observations are at the resolution of its features)."""
    sc, toff, tcam, txy = planted_scene(N_CAMS)
    scene.add_features(sc, 900)
    kps = [np.ascontiguousarray(k, np.float32) for k in sc.kp_xy]
    ds = ctx.descset(sc.desc, keypoints=kps)
    th_e, th_d = slam.thresholds(1.0)
    assert (th_e, th_d) == (2.0, 5.0)
    pairs, Fp, Hp, cand = ctx.slam_priors(N_CAMS, toff, tcam, txy, th_epipolar=th_e, th_distance=th_d)
    res = ds.match_pairs_slam(pairs, Fp, Hp, th_first_second_ratio=0.80, th_epipolar=th_e, th_distance=th_d)
    R_, t, c, fk = scene.cameras_for_tracks(sc)
    gps = D.PLANTED_SCALE * c @ D.rodrigues(D.PLANTED_AA).T + D.PLANTED_T + np.random.default_rng(9).normal(0, D.GPS_NOISE, c.shape)
    w = dict(sc=sc, toff=toff, tcam=tcam, txy=txy, kps=kps, ds=ds, res=res, pairs=pairs, Fp=Fp, Hp=Hp, cand=cand, R=R_, t=t, c=c, fk=fk, gps=gps,
             model=sc.cam_model_gt.copy(), moc=sc.cam_model_of_cam)
    yield w
    res.close(); ds.close()


def test_end_to_end_equals_the_host_array_path(ctx, world):
    w, sc, pairs, kps = world, world["sc"], world["pairs"], world["kps"]
    assert len(pairs) >= 10 and [tuple(p) for p in pairs] == sorted(tuple(p) for p in pairs)
    ch = capi.Chain(w["res"])
    n_m, ok, F = ch.verify_slam(seed=SEED)
    nt, no = ch.build_tracks()
    n_acc = ch.triangulate(w["R"], w["t"], w["c"], w["fk"], 7.0, np.deg2rad(3.0))
    F_h, ok_h, fin_h, moff, surv, (off_h, img_h, feat_h) = _host_path(ctx, w["res"], pairs, kps, SEED)
    na, _ = w["res"].counts()
    np.testing.assert_array_equal(na, [len(s) for s in surv])
    np.testing.assert_array_equal(ok, ok_h)
    np.testing.assert_array_equal(F, F_h)
    np.testing.assert_array_equal(n_m, [len(m) for m in fin_h])
    for p in range(len(pairs)):
        np.testing.assert_array_equal(ch.fetch_matches(p), fin_h[p])
    off, img, feat = ch.fetch_tracks()
    np.testing.assert_array_equal(off, off_h); np.testing.assert_array_equal(img, img_h); np.testing.assert_array_equal(feat, feat_h)
    xy = np.array([kps[i][f] for i, f in zip(img_h, feat_h)], dtype=np.float64)
    tr = A.TrackArrays(off_h, img_h, xy, w["R"], w["t"], w["c"], w["fk"])
    X_h, mse_h, tok_h = ctx.triangulate_midpoint(tr, 7.0, np.deg2rad(3.0))
    X, mse, tok = ch.fetch_points()
    np.testing.assert_array_equal(tok, tok_h); np.testing.assert_array_equal(X, X_h); np.testing.assert_array_equal(mse, mse_h)
    assert ok.sum() >= 10 and nt > 500 and n_acc == int(tok_h.sum()) > 0
    # the project's quality bars: kept matches are true correspondences, tracks are single points of the scene
    good = total = 0
    for (i, j), m in zip(pairs, fin_h):
        fi, fj = sc.feat_point[i][m[:, 0]], sc.feat_point[j][m[:, 1]]
        good += int(((fi == fj) & (fi >= 0)).sum()); total += len(m)
    assert total > 500 and good / total > 0.9, (good, total)
    pid = np.array([sc.feat_point[i][f] for i, f in zip(img_h, feat_h)])
    same = np.array([len(set(pid[off_h[k]:off_h[k + 1]])) == 1 for k in range(0, nt, 5)])
    assert same.mean() > 0.95
    ch.close()


def test_store_from_a_slam_chain(ctx, world):
    w, sc, pairs, kps = world, world["sc"], world["pairs"], world["kps"]
    ch = capi.Chain(w["res"])
    with pytest.raises(capi.MsfmError) as e:
        capi.MatchStore.from_chain(ch)                 # before verify_slam
    assert e.value.code == A.MSFM_E_INVAL
    n_m, _, _ = ch.verify_slam(seed=SEED)
    st_c = capi.MatchStore.from_chain(ch)
    fetched = [ch.fetch_matches(p) for p in range(len(pairs))]
    moff = np.concatenate([[0], np.cumsum(n_m)]).astype(np.int32)
    ch.close()
    st_h = ctx.match_store([len(k) for k in kps], pairs, moff, np.concatenate(fetched))
    rng = np.random.default_rng(11)
    cam_img = np.arange(6, dtype=np.int32)
    fp = np.concatenate([sc.feat_point[i] for i in cam_img]).astype(np.int32)
    n_pts = sc.n_points
    args = [cam_img, fp, rng.random(n_pts) < 0.05, np.round(rng.uniform(0, 4, n_pts), 1), rng.integers(2, 6, n_pts), np.arange(6, 10), [0, 1, 0, 3]]
    a = ctx.localize_candidates(st_c, *args, point_xyz=sc.point_gt)
    b = ctx.localize_candidates(st_h, *args, point_xyz=sc.point_gt, keypoints=np.concatenate(kps))
    keys = ("rank", "corr_off", "corr_feat", "corr_point", "vis_off", "vis_cam")
    assert len(a["rank"]) >= 1 and a["corr_off"][-1] > 100
    for k in keys + ("pts_w", "pts_2d"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    want = localize_ref([len(k) for k in kps], pairs, moff, np.concatenate(fetched), *args)
    for k in keys:
        np.testing.assert_array_equal(a[k], want[k], err_msg=k)
    st_c.close(); st_h.close()


def test_slam_gps_run_equals_the_calls_by_hand(ctx, world, tmp_path):
    """slam.slam_gps_run = slam.feature_matching + build_tracks + gpsreg.slam_gps_register: every record equals the chain made
    by hand from the same calls, the cost falls, and the files written on the way read back as the restatement's."""
    w, pairs, kps = world, world["pairs"], world["kps"]
    opts = lambda: capi.default_options(max_num_iterations=ITER)
    fold = str(tmp_path / "out")
    ch, res, rec, reg = slam.slam_gps_run(ctx, w["ds"], N_CAMS, w["toff"], w["tcam"], w["txy"], w["R"], w["c"], w["model"], w["moc"], w["gps"],
                                          resize_ratio=1.0, fold=fold, fransac=dict(seed=SEED), options=opts())
    hand = capi.Chain(w["res"])
    n_m, ok, F = hand.verify_slam(seed=SEED)
    nt, no = hand.build_tracks()
    reg_h = gpsreg.slam_gps_register(hand, w["R"], w["c"], w["model"], w["moc"], w["gps"], options=opts())
    # the matching record
    np.testing.assert_array_equal(rec["pairs"], pairs); np.testing.assert_array_equal(rec["F_prior"], w["Fp"]); np.testing.assert_array_equal(rec["H_prior"], w["Hp"])
    np.testing.assert_array_equal(rec["candidates"], w["cand"]); np.testing.assert_array_equal(rec["n_survivors"], w["res"].counts()[0])
    np.testing.assert_array_equal(rec["n_matches"], n_m); np.testing.assert_array_equal(rec["ok"], ok); np.testing.assert_array_equal(rec["F"], F)
    assert (rec["n_tracks"], rec["n_obs"]) == (nt, no) and ch.slam
    g = np.zeros((N_CAMS, N_CAMS), np.int64)
    g[pairs[:, 0], pairs[:, 1]] = n_m
    np.testing.assert_array_equal(rec["match_graph"], g)
    # the registration record
    for k in ("scale", "err", "offset", "Rg", "tg", "weight", "gps", "cam_pose", "cam_model"):
        np.testing.assert_array_equal(reg[k], reg_h[k], err_msg=k)
    for k in ("n_accepted", "n_outliers", "n_inliers", "n_outliers_adjusted", "n_inliers_adjusted", "gps_weight_used", "n_points", "n_obs"):
        assert reg[k] == reg_h[k], k
    for k in ("termination", "num_iterations", "initial_cost", "final_cost", "num_residuals"):
        assert reg["summary"][k] == reg_h["summary"][k], k
    np.testing.assert_array_equal(reg["summary"]["iterations"]["cost"], reg_h["summary"]["iterations"]["cost"])
    for a, b in zip(ch.fetch_points(), hand.fetch_points()):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(ch.fetch_accuracy(), hand.fetch_accuracy()):
        np.testing.assert_array_equal(a, b)
    assert reg["n_points"] >= 100 and reg["summary"]["final_cost"] < reg["summary"]["initial_cost"]
    # the files: prior.txt, <i>_match, graph_matching.txt against the sequential restatement on the codes
    kept, n_r, ok_r, F_r = R.verify(pairs, [w["res"].fetch(p)[0] for p in range(len(pairs))], kps, seed=SEED)
    np.testing.assert_array_equal(n_m, n_r); np.testing.assert_array_equal(ok, ok_r); np.testing.assert_array_equal(F, F_r)
    np.testing.assert_array_equal(matchfiles.read_in_matching_graph(fold, N_CAMS), R.match_graph(N_CAMS, pairs, kept))
    for i in range(N_CAMS):
        ids, ms = matchfiles.query_match(fold, i)
        want = [(int(j), kept[p]) for p, (a, j) in enumerate(pairs) if a == i and len(kept[p])]
        assert ids == [j for j, _ in want]
        for m, (_, k) in zip(ms, want):
            np.testing.assert_array_equal(m, k)
    n, pr, F2, H2 = matchfiles.read_prior_info(os.path.join(fold, "prior.txt"))
    assert n == N_CAMS and (pr == pairs).all()
    reg["ba"].close(); reg_h["ba"].close(); ch.close(); res.close(); hand.close()


def test_host_driver_writes_the_same_match_files(ctx, world, tmp_path):
    """host/test_slam_match (SLAMGPS::FeatureMatching step 2 of the C++ mirror + WriteOutMatches / WriteOutMatchGraph) on one
    binary file of descriptors, keypoints and priors writes the bytes slam.feature_matching(fold=...) writes."""
    w, sc, kps = world, world["sc"], world["kps"]
    exe = os.path.join(ROOT, "host", "test_slam_match")
    assert os.path.exists(exe), "host/test_slam_match not built"
    py = tmp_path / "py"
    ch, res, rec = slam.feature_matching(ctx, w["ds"], N_CAMS, w["toff"], w["tcam"], w["txy"], fold=str(py))     # resize_ratio 0.5, default seed
    ch.close(); res.close()
    assert rec["n_matches"].sum() > 500
    src = tmp_path / "input.bin"
    with open(src, "wb") as f:
        np.array([N_CAMS], np.int32).tofile(f)
        for d, k in zip(sc.desc, kps):
            np.array([len(d)], np.int32).tofile(f)
            np.ascontiguousarray(d, np.float32).tofile(f)
            np.ascontiguousarray(k, np.float32).tofile(f)
        np.array([len(rec["pairs"])], np.int32).tofile(f)
        for (i, j), F, H in zip(rec["pairs"], rec["F_prior"], rec["H_prior"]):
            np.array([i, j], np.int32).tofile(f)
            np.ascontiguousarray(F, np.float64).tofile(f)
            np.ascontiguousarray(H, np.float64).tofile(f)
    host = tmp_path / "host"
    host.mkdir()
    subprocess.run([exe, str(src), str(host)], check=True, timeout=600)
    names = sorted(os.listdir(py))
    assert sorted(os.listdir(host) + ["prior.txt"]) == names and "graph_matching.txt" in names and len(names) > 10
    for n in names:
        if n != "prior.txt":
            assert (host / n).read_bytes() == (py / n).read_bytes(), n
