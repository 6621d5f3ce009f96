"""msfm_match_store + msfm_localize_candidates (IncrementalSfM::FindImageToLocalize, sfm_incremental.cc:440-562) against the dict
walk of tests/localize_ref.py: integer work and a total sort order, so every array must be identical."""
import numpy as np
import pytest

from metricsfm_amd import _abi as A
from metricsfm_amd import capi, localize, scene
from tests import localize_data as D
from tests.localize_ref import localize_ref

pytestmark = pytest.mark.gpu

LDS_MAX = 4096   # LOC_LDS_MAX of csrc/localize.hip: the longest segment the LDS sort takes


def _same(got, want, keys=D.ARRAYS):
    for k in keys:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


@pytest.fixture(scope="module")
def ring():
    c = D.ring_round()
    c["ref"] = localize_ref(*D.store_args(c), *D.problem_args(c), point_xyz=c["point_xyz"], keypoints=c["keypoints"])
    return c


def test_ring_round_is_identical_to_the_walk(ctx, ring):
    st = ctx.match_store(*D.store_args(ring))
    got = ctx.localize_candidates(st, *D.problem_args(ring), point_xyz=ring["point_xyz"], keypoints=ring["keypoints"])
    _same(got, ring["ref"], D.ARRAYS + ("pts_w", "pts_2d"))
    assert len(got["rank"]) == 4 and got["corr_off"][-1] > 400
    # the numpy gather, spelled out once more on the library's own index arrays
    np.testing.assert_array_equal(got["pts_w"], ring["point_xyz"][got["corr_point"]])
    img = np.repeat(ring["cand_img"][got["rank"]], np.diff(got["corr_off"]))
    np.testing.assert_array_equal(got["pts_2d"], ring["keypoints"][img * 200 + got["corr_feat"]].astype(np.float64))
    # what crossed to the device does not grow with the matches: the per-call arrays, the four candidates' keypoints and a few
    # integers per walked pair
    per_call = sum(ring[k].nbytes for k in ("feat_point", "pt_bad", "pt_mse", "pt_views", "point_xyz")) + 4 * 200 * 2 * 4
    assert got["h2d_bytes"] < per_call + 4096 < ring["matches"].nbytes
    # without point_xyz: the same index arrays, no points
    bare = ctx.localize_candidates(st, *D.problem_args(ring))
    _same(bare, ring["ref"])
    assert "pts_w" not in bare
    st.close()


@pytest.mark.parametrize("name", sorted(D.QUIRKS))
def test_quirk_through_the_library(ctx, name):
    c = D.QUIRKS[name]
    st = ctx.match_store(*D.store_args(c))
    _same(ctx.localize_candidates(st, *D.problem_args(c)), c["expect"])
    st.close()


def test_both_sort_paths(ctx, monkeypatch):
    """Candidate image 1 has LDS_MAX + 37 correspondences (rocPRIM's segmented sort), image 2 has 20 (the LDS sort); with the
    switch that sends everything through rocPRIM the arrays stay the same.  mse values repeat, so ties are sorted on both paths."""
    n = LDS_MAX + 37
    rng = np.random.default_rng(3)
    ident = np.column_stack([np.arange(n), rng.permutation(n)]).astype(np.int32)
    few = np.column_stack([rng.permutation(20), rng.integers(0, n, 20)]).astype(np.int32)
    c = dict(n_features=np.array([n, n, 20], np.int32), pairs=np.array([[1, 0], [2, 0]], np.int32), match_off=np.array([0, n, n + 20], np.int32),
             matches=np.concatenate([ident, few]), cam_img=np.array([0], np.int32), feat_point=rng.permutation(n).astype(np.int32),
             pt_bad=np.zeros(n, np.uint8), pt_mse=rng.integers(0, 50, n) * 0.25, pt_views=rng.integers(2, 5, n).astype(np.int32),
             cand_img=np.array([1, 2], np.int32), fail_times=np.zeros(2, np.int32))
    want = localize_ref(*D.store_args(c), *D.problem_args(c))
    assert list(np.diff(want["corr_off"])) == [n, 20]
    st = ctx.match_store(*D.store_args(c))
    got = ctx.localize_candidates(st, *D.problem_args(c))
    _same(got, want)
    monkeypatch.setenv("MSFM_LOCALIZE_LDS_MAX", "0")
    forced = ctx.localize_candidates(st, *D.problem_args(c))
    monkeypatch.delenv("MSFM_LOCALIZE_LDS_MAX")
    _same(forced, got)
    st.close()


def test_store_from_chain_equals_store_from_its_matches(ctx):
    """Config 1 with 1500 requested features (the smallest chain scene of tests/test_gpu_chain.py): the store copied out of the
    verified chain and a store made from the fetched matches + the same keypoints give the same answer."""
    sc = scene.add_features(scene.config_scene(1), 1500)
    kps = [np.ascontiguousarray(k, np.float32) for k in sc.kp_xy]
    pairs = scene.all_pairs(sc.n_cams)
    ds = ctx.descset(sc.desc, keypoints=kps)
    res = ds.match_pairs(pairs, 0.6, 0.85)
    ch = capi.Chain(res)
    with pytest.raises(capi.MsfmError) as e:
        capi.MatchStore.from_chain(ch)                 # before verify
    assert e.value.code == A.MSFM_E_INVAL
    n_m, ok, _ = ch.verify(3.0, seed=5)
    st_c = capi.MatchStore.from_chain(ch)
    fetched = [ch.fetch_matches(p) for p in range(len(pairs))]
    moff = np.concatenate([[0], np.cumsum(n_m)]).astype(np.int32)
    ch.close(); res.close(); ds.close()                # the store keeps its own copies
    st_h = ctx.match_store([len(k) for k in kps], pairs, moff, np.concatenate(fetched))
    rng = np.random.default_rng(11)
    cam_img = np.arange(6, dtype=np.int32)
    fp = np.concatenate([sc.feat_point[i] for i in cam_img]).astype(np.int32)
    n_pts = sc.n_points
    args = [cam_img, fp, rng.random(n_pts) < 0.05, np.round(rng.uniform(0, 4, n_pts), 1), rng.integers(2, 6, n_pts), np.arange(6, 10), [0, 1, 0, 3]]
    a = ctx.localize_candidates(st_c, *args, point_xyz=sc.point_gt)
    b = ctx.localize_candidates(st_h, *args, point_xyz=sc.point_gt, keypoints=np.concatenate(kps))
    assert len(a["rank"]) == 4 and a["corr_off"][-1] > 1000
    _same(a, b, D.ARRAYS + ("pts_w", "pts_2d"))
    _same(a, localize_ref([len(k) for k in kps], pairs, moff, np.concatenate(fetched), *args))
    st_c.close(); st_h.close()


def test_bad_input_is_refused_and_the_context_stays_usable(ctx):
    c = D.QUIRKS["duplicates_first_wins_all_counted"]
    good = ctx.match_store(*D.store_args(c))

    def still_works():
        _same(ctx.localize_candidates(good, *D.problem_args(c)), c["expect"])

    def refused(fn, *words):
        with pytest.raises(capi.MsfmError) as e:
            fn()
        assert e.value.code == A.MSFM_E_INVAL
        assert all(w in str(e.value) for w in words), str(e.value)
        still_works()

    nf, pairs, moff, m = D.store_args(c)
    refused(lambda: ctx.match_store(nf, pairs[::-1], moff, m), "ascending")                      # unsorted pairs
    refused(lambda: ctx.match_store(nf, np.array([[2, 0], [2, 0]], np.int32), moff, m), "ascending")   # a pair twice
    m_bad = m.copy(); m_bad[3, 1] = nf[0]                                                       # pair (2, 0): a feature of image 0 at n_features[0]
    refused(lambda: ctx.match_store(nf, pairs, moff, m_bad), "match 3")
    m_neg = m.copy(); m_neg[6, 0] = -1
    refused(lambda: ctx.match_store(nf, pairs, moff, m_neg), "match 6")
    cam_img, fp, bad, mse, views, cand, fail = D.problem_args(c)
    fp_bad = fp.copy(); fp_bad[12] = D.N_POINTS                                                 # camera 1, feature 2
    refused(lambda: ctx.localize_candidates(good, cam_img, fp_bad, bad, mse, views, cand, fail), "camera 1", "feature 2")
    refused(lambda: ctx.localize_candidates(good, cam_img, fp, bad, mse, views, [1, 2], fail), "registered")   # a registered image as candidate
    refused(lambda: ctx.localize_candidates(good, cam_img, fp, bad, mse, views, [3, 2], fail), "ascending")
    refused(lambda: ctx.localize_candidates(good, cam_img, fp, bad, mse, views, cand, fail, point_xyz=np.zeros((D.N_POINTS, 3))), "keypoints")
    good.close()


def test_a_candidate_does_not_depend_on_the_batch(ctx, ring):
    st = ctx.match_store(*D.store_args(ring))
    cam_img, fp, bad, mse, views, cand, fail = D.problem_args(ring)
    ref = ring["ref"]
    for k in range(len(cand)):
        one = ctx.localize_candidates(st, cam_img, fp, bad, mse, views, cand[k:k + 1], fail[k:k + 1], point_xyz=ring["point_xyz"],
                                      keypoints=ring["keypoints"])
        r = int(np.nonzero(ref["rank"] == k)[0][0])
        assert list(one["rank"]) == [0]
        for name, off, w in (("corr_feat", "corr_off", 1), ("corr_point", "corr_off", 1), ("vis_cam", "vis_off", 1), ("pts_w", "corr_off", 3),
                             ("pts_2d", "corr_off", 2)):
            np.testing.assert_array_equal(one[name], ref[name][ref[off][r]:ref[off][r + 1]], err_msg=name)
    st.close()


def test_one_round_feeds_epnp(ctx):
    """find_images_to_localize -> epnp_ransac on the returned corr_off / pts_w / pts_2d as they are: exact points, 0.5 px noise on
    the keypoints, so every candidate localises below th_mse_localization = 5.0 (basic_structs.h:186, sfm_incremental.cc:648;
    the bound host/test_sfm.cc holds its localisation to)."""
    c = D.ring_round(wrong=0.0, exact=True)
    sc = c["scene"]
    st = ctx.match_store(*D.store_args(c))
    n = sc.n_cams
    match_count = np.zeros((n, n), np.int32)
    match_count[c["pairs"][:, 0], c["pairs"][:, 1]] = np.diff(c["match_off"])
    fail = np.zeros(n, np.int32); fail[7] = 2
    ids, corres, visible, r = localize.find_images_to_localize(ctx, st, match_count, c["cam_img"], c["feat_point"], c["pt_bad"], c["pt_mse"],
                                                               c["pt_views"], fail, point_xyz=c["point_xyz"], keypoints=c["keypoints"], arrays=True)
    assert ids == [6, 8, 9, 7]                          # 200 / 5 three times (lower image id first), then 200 / 7
    assert all(len(x) == 200 for x in corres) and all(list(v) == [0, 1, 2, 3, 4, 5] for v in visible)
    for i, x in zip(ids, corres):
        np.testing.assert_array_equal(x[:, 0], x[:, 1])   # feature f of a ring image is point f
        mse = c["pt_mse"][x[:, 1]] + 3.0 * (c["pt_views"][x[:, 1]] <= 2)
        assert (np.diff(mse) >= 0).all()
    _, _, _, avg, _ = ctx.epnp_ransac(r["corr_off"], r["pts_w"], r["pts_2d"], scene.FOCAL)
    print("avg_error per candidate:", avg)
    assert len(avg) == 4 and (avg < 5.0).all(), avg
    st.close()
