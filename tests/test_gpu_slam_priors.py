"""msfm_slam_priors = SLAMGPS::FeatureMatching step 1 (slam_gps.cc:323-423): bit-identical to composing the public calls
(gather the window pairs' shared points, msfm_fundamental_ransac_batch, msfm_homography_ransac_batch, the binary32 gates),
every verdict planted, and steps 1 + 2 end to end through msfm_match_pairs_slam with priors from this call."""
import os
import subprocess

import numpy as np
import pytest

from metricsfm_amd import _abi as A
from metricsfm_amd import capi, matchfiles, scene
from tests.slam_scene import planted_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CAMS = 16


@pytest.fixture(scope="module")
def planted():
    return planted_scene(N_CAMS)


def compose(ctx, n_cams, toff, tcam, txy, win=5, th_same=20, the=2.0, thd=5.0, rf=0.5, hf=0.9,
            seed_f=0x4D53464D46, seed_h=0x4D53464D48):
    """Step 1 from the public calls, as the contract states it: candidates in (i, j) order, the RANSACs over the list of
    those with >= th_same shared points, gates in binary32."""
    cam_pts = [[] for _ in range(n_cams)]
    for t in range(len(toff) - 1):
        for o in range(toff[t], toff[t + 1]):
            cam_pts[tcam[o]].append((t, o))
    rows, parts, cand = [], [], []
    for i in range(n_cams):
        for j in range(max(i - win, 0), min(i + win, n_cams)):
            if j == i:
                continue
            a, b = dict(cam_pts[i]), dict(cam_pts[j])
            sh = sorted(set(a) & set(b))
            rows.append([i, j, len(sh), -1, -1, 1])
            if len(sh) >= th_same:
                cand.append(len(rows) - 1)
                parts.append((txy[[a[p] for p in sh]].astype(np.float32), txy[[b[p] for p in sh]].astype(np.float32)))
    off = np.zeros(len(parts) + 1, np.int32)
    off[1:] = np.cumsum([len(p) for p, _ in parts])
    p1 = np.concatenate([p for p, _ in parts])
    p2 = np.concatenate([q for _, q in parts])
    F, _, nf, _ = ctx.fundamental_ransac(off, p1, p2, threshold=float(np.float32(the)), confidence=0.99, max_iterations=2000, min_points=8,
                                         min_inliers=0, seed=seed_f)
    H, _, nh, _ = ctx.homography_ransac(off, p1, p2, threshold=float(np.float32(thd)), seed=seed_h)
    kept = []
    for c, k in enumerate(cand):
        N = off[c + 1] - off[c]
        rows[k][3] = nf[c]
        if np.float32(nf[c]) < np.float32(N) * np.float32(rf) or nf[c] < 30:
            rows[k][5] = 2
            continue
        rows[k][4] = nh[c]
        if np.float32(nh[c]) > np.float32(nf[c]) * np.float32(hf):
            rows[k][5] = 3
            continue
        rows[k][5] = 0
        kept.append((rows[k][0], rows[k][1], F[c], H[c]))
    return np.array(rows, np.int32), kept


@pytest.mark.gpu
def test_equals_the_composition_of_public_calls(ctx, planted):
    sc, toff, tcam, txy = planted
    pairs, F, H, cand = ctx.slam_priors(N_CAMS, toff, tcam, txy)
    rows, kept = compose(ctx, N_CAMS, toff, tcam, txy)
    np.testing.assert_array_equal(cand, rows)
    assert len(pairs) == len(kept)
    for p, (i, j, f, h) in enumerate(kept):
        assert tuple(pairs[p]) == (i, j)
        np.testing.assert_array_equal(F[p], f)
        np.testing.assert_array_equal(H[p], h)
    assert set(cand[:, 5].tolist()) == {0, 1, 2, 3}, np.bincount(cand[:, 5])
    # the window: offsets -win .. win - 1 ((i + 5, i) is a candidate slot, (i, i + 5) is not)
    slots = [(int(i), int(j)) for i, j in cand[:, :2]]
    assert (5, 0) in slots and (0, 5) not in slots and (10, 5) in slots and (5, 10) not in slots
    assert len(slots) == sum(min(i + 5, N_CAMS) - max(i - 5, 0) - 1 for i in range(N_CAMS))
    assert slots == sorted(slots)
    assert (H[:, 2, 2] == 1.0).all()


def _f32_boundaries(n_shared, nf, nh):
    """Thresholds on a kept candidate's counts, by binary32 arithmetic: rf_keep is the largest t with N * t <= n_f (the F
    gate `n_f < N * t` keeps the pair) and rf_drop the next float up (it rejects); hf_keep is the smallest t with
    n_f * t >= n_h (the H gate `n_h > n_f * t` keeps it) and hf_drop the next float down (it rejects)."""
    N, f, h, one, zero = np.float32(n_shared), np.float32(nf), np.float32(nh), np.float32(1), np.float32(0)
    t = f / N
    while N * t > f:
        t = np.nextafter(t, zero)
    while N * np.nextafter(t, one) <= f:
        t = np.nextafter(t, one)
    rf_keep, rf_drop = t, np.nextafter(t, one)
    u = h / f
    while f * u < h:
        u = np.nextafter(u, one)
    while f * np.nextafter(u, zero) >= h:
        u = np.nextafter(u, zero)
    hf_keep, hf_drop = u, np.nextafter(u, zero)
    assert not (f < N * rf_keep) and f < N * rf_drop and not (h > f * hf_keep) and h > f * hf_drop
    return rf_keep, rf_drop, hf_keep, hf_drop


@pytest.mark.gpu
def test_binary32_gate_boundaries(ctx, planted):
    """Thresholds exactly on a kept candidate's counts: `count_f < N * th_ratio_f` and `count_h > count_f * th_h_f_ratio`
    are evaluated in binary32 (slam_gps.cc:318-319 are float).  At the boundary the pair is kept, one ulp past it the F
    gate (verdict 2) or the H gate (verdict 3) rejects it, and every row equals the composition of the public calls."""
    sc, toff, tcam, txy = planted
    _, _, _, cand = ctx.slam_priors(N_CAMS, toff, tcam, txy)
    kept = cand[(cand[:, 5] == 0) & (cand[:, 3] >= 30)]
    r = kept[np.argmax(kept[:, 2])]
    rf_keep, rf_drop, hf_keep, hf_drop = _f32_boundaries(r[2], r[3], r[4])
    for rf, hf, want in ((rf_keep, hf_keep, 0), (rf_drop, hf_keep, 2), (rf_keep, hf_drop, 3)):
        pairs, F, H, c2 = ctx.slam_priors(N_CAMS, toff, tcam, txy, th_ratio_f=float(rf), th_h_f_ratio=float(hf))
        rows, _ = compose(ctx, N_CAMS, toff, tcam, txy, rf=rf, hf=hf)
        np.testing.assert_array_equal(c2, rows)
        k = np.nonzero((c2[:, 0] == r[0]) & (c2[:, 1] == r[1]))[0][0]
        assert tuple(c2[k, 2:4]) == tuple(r[2:4])
        assert c2[k, 4] == (-1 if want == 2 else r[4])   # H does not run where the F gate rejects
        assert c2[k, 5] == want, (rf, hf, c2[k])
        assert len(pairs) == (rows[:, 5] == 0).sum()


@pytest.mark.gpu
def test_steps_one_and_two_end_to_end(ctx, planted):
    """The kept pairs / F / H of this call go straight into msfm_match_pairs_slam on the scene's features: the survivors are
    true correspondences (the bar of test_match_pairs_slam_gates), and no prior comes from the ground truth."""
    sc, toff, tcam, txy = planted
    pairs, F, H, cand = ctx.slam_priors(N_CAMS, toff, tcam, txy)
    assert len(pairs) >= 10
    scene.add_features(sc, 900)
    ds = ctx.descset(sc.desc, keypoints=sc.kp_xy)
    res = ds.match_pairs_slam(pairs.astype(np.int32), F, H, th_epipolar=2.0, th_distance=5.0)
    na, ng = res.counts()
    good, total = 0, 0
    for p, (i, j) in enumerate(pairs):
        code = res.fetch(p)[0]
        ok = code >= 0
        fi, fj = sc.feat_point[i][code[ok]], sc.feat_point[j][np.nonzero(ok)[0]]
        good += int(((fi == fj) & (fi >= 0)).sum())
        total += int(ok.sum())
        assert ok.sum() == na[p]
    assert total > 500 and good / total > 0.9, (good, total)
    res.close()
    ds.close()


@pytest.mark.gpu
def test_invalid_input_is_refused(ctx, planted):
    sc, toff, tcam, txy = planted
    # thresholds the public calls refuse: msfm_fundamental_ransac_batch takes no F threshold <= 0 or NaN,
    # msfm_homography_ransac_batch no NaN
    for kw in ({"win_size": 0}, {"th_same_pts": 14}, {"th_epipolar": 0.0}, {"th_epipolar": -2.0}, {"th_epipolar": float("nan")},
               {"th_distance": float("nan")}):
        with pytest.raises(capi.MsfmError) as e:
            ctx.slam_priors(N_CAMS, toff, tcam, txy, **kw)
        assert e.value.code == A.MSFM_E_INVAL
    for c in (N_CAMS, -1):
        bad = tcam.copy()
        bad[5] = c
        with pytest.raises(capi.MsfmError) as e:
            ctx.slam_priors(N_CAMS, toff, bad, txy)
        assert e.value.code == A.MSFM_E_INVAL
    t = next(t for t in range(len(toff) - 1) if toff[t + 1] - toff[t] >= 2)
    dup = tcam.copy()
    dup[toff[t] + 1] = dup[toff[t]]   # two observations of point t in one camera
    with pytest.raises(capi.MsfmError) as e:
        ctx.slam_priors(N_CAMS, toff, dup, txy)
    assert e.value.code == A.MSFM_E_INVAL
    # a point with a single observation is allowed; so are cameras without any
    pairs, F, H, cand = ctx.slam_priors(4, [0, 1, 3], [2, 0, 1], [[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]])
    assert len(pairs) == 0 and (cand[:, 5] == 1).all() and len(cand) == 12


@pytest.mark.gpu
def test_host_driver_writes_the_same_prior_file(ctx, planted, tmp_path):
    """host/test_slam_priors (SLAMGPS::FeatureMatchingPriors + WriteOutPriorInfo) on a binary track file writes the
    prior.txt of the Python path (Context.slam_priors + matchfiles.write_prior_info)."""
    sc, toff, tcam, txy = planted
    exe = os.path.join(ROOT, "host", "test_slam_priors")
    assert os.path.exists(exe), "host/test_slam_priors not built"
    trk = tmp_path / "points.bin"
    with open(trk, "wb") as f:
        np.array([N_CAMS, len(toff) - 1], np.int32).tofile(f)
        for t in range(len(toff) - 1):
            s = slice(toff[t], toff[t + 1])
            np.array([toff[t + 1] - toff[t]], np.int32).tofile(f)
            rec = np.zeros(toff[t + 1] - toff[t], dtype=[("cam", "<i4"), ("x", "<f8"), ("y", "<f8")])
            rec["cam"], rec["x"], rec["y"] = tcam[s], txy[s, 0], txy[s, 1]
            rec.tofile(f)
    # default resize_ratio 0.5 (SLAMGPS::SLAMGPS, slam_gps.cc:55): thresholds 2.0 / 0.5 = 4 px and 5.0 / 0.5 = 10 px (:316-317);
    # then resize_ratio 1 given on the command line: the library defaults 2 px and 5 px
    texts = []
    for args, th in (([], (4.0, 10.0)), (["1"], (2.0, 5.0))):
        out = tmp_path / ("prior_host_%d.txt" % len(args))
        subprocess.run([exe, str(trk), str(out)] + args, check=True, timeout=600)
        pairs, F, H, cand = ctx.slam_priors(N_CAMS, toff, tcam, txy, th_epipolar=th[0], th_distance=th[1])
        py = tmp_path / ("prior_py_%d.txt" % len(args))
        matchfiles.write_prior_info(str(py), N_CAMS, pairs, F, H)
        assert out.read_text() == py.read_text(), args
        n, pr, F2, H2 = matchfiles.read_prior_info(str(out))
        assert n == N_CAMS and (pr == pairs).all()
        texts.append((out.read_text(), cand))
    # the thresholds reach the estimators: the F inlier counts move with them
    assert (texts[0][1][:, 3] != texts[1][1][:, 3]).any()
