"""msfm_new_points - IncrementalSfM::GenerateNew3DPoints (sfm_incremental.cc:755-915) for a list of new cameras on the resident
match store - against the sequential restatement tests/newpoints_ref.cpp: every fetched array identical, bit for bit.
(tests/test_newpoints_ref.py holds the restatement to the oracle's literal loop on the same cases, with the margins asserted.)"""
import os

import numpy as np
import pytest

from metricsfm_amd import _abi as A
from metricsfm_amd import capi, newpoints, scene, tracks
from tests import newpoints_data as D
from tests import newpoints_ref as NR
from tests.newpoints_data import SEED_CLAIMS, SEED_DEGENERATE, SEED_WALK

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden", "newpoints_golden.npz")


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return NR.build_ref(tmp_path_factory.mktemp("newpoints_ref"))


@pytest.fixture(scope="module")
def walk(L):
    c = D.walk_case(SEED_WALK)
    c["ref"] = NR.new_points(L, *D.ref_args(c))
    c["ref0"] = NR.new_points(L, *D.ref_args(D.sub(c, [0])))
    return c


def same(got, want, keys=NR.FETCHED):
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, w.dtype, g.shape, w.shape)
        np.testing.assert_array_equal(g, w, err_msg=k)


def run(ctx, c, st=None, **opts):
    own = st is None
    st = ctx.match_store(*D.store_args(c)) if own else st
    try:
        return ctx.new_points(st, *D.call_args(c), keypoints=c["keypoints"], **opts)
    finally:
        if own:
            st.close()


def test_walk(ctx, walk):
    got = run(ctx, D.sub(walk, [0]))
    same(got, walk["ref0"])
    print("per entry:", got["n_matches"].tolist(), got["large"].tolist(), got["n_candidates"].tolist(), got["n_accepted"].tolist())
    assert got["n_matches"].tolist() == D.WALK_N_MATCHES and got["large"].tolist() == D.WALK_LARGE
    assert got["n_candidates"].tolist() == D.WALK_N_CANDIDATES and got["n_accepted"].tolist() == D.WALK_N_ACCEPTED
    keys = got["mse"].astype(np.int64)
    assert (np.diff(keys) >= 0).all() and len(np.unique(keys)) >= 3 and np.bincount(keys).max() > 1
    walk_pos = got["vis_entry"].astype(np.int64) * 1000 + got["pt_match"]
    assert all((np.diff(walk_pos[keys == v]) > 0).all() for v in np.unique(keys))          # ties keep the walk order
    # match 256 of the pair of 257 repeats match 3: both are points, with the same coordinates
    e = np.nonzero((got["vis_entry"] == 4) & np.isin(got["pt_match"], (3, 256)))[0]
    assert len(e) == 2 and (got["X"][e[0]] == got["X"][e[1]]).all() and got["takes1"][e].tolist() == [1, 0]


def test_claims(ctx, L):
    c = D.claims_case(SEED_CLAIMS)
    got = run(ctx, c)
    same(got, NR.new_points(L, *D.ref_args(c)))
    keys = got["mse"].astype(np.int64)
    sel = np.nonzero(got["feat1"] == c["shared_f1"])[0]
    assert len(sel) == 3 and sorted(got["vis_entry"][sel].tolist()) == [0, 1, 2]         # all three accepted
    assert got["takes1"][sel].tolist() == [1, 0, 0] and keys[sel].tolist() == [0, 0, 2]   # exactly one, on the lowest key
    assert got["vis_entry"][sel].tolist() == [1, 2, 0]                                    # the tie to the earlier entry; not the walk-first
    sel = np.nonzero((got["feat2"] == c["shared_f2"]) & (got["cam2"] == c["shared_f2_cam"]))[0]
    assert len(sel) == 2 and got["takes2"][sel].tolist() == [1, 0] and keys[sel].tolist() == [0, 2]
    assert got["pt_match"][sel[0]] > got["pt_match"][sel[1]]                              # the sorted-first is the walk-second
    other = np.ones(len(keys), bool)
    other[sel] = False
    assert got["takes2"][other].all()


def test_degenerate(ctx, L):
    c = D.degenerate_case(SEED_DEGENERATE)
    st = ctx.match_store(*D.store_args(c))
    got = run(ctx, c, st)
    same(got, NR.new_points(L, *D.ref_args(c)))
    assert got["n_matches"].tolist() == D.DEGENERATE_N_MATCHES and got["n_accepted"].tolist() == D.DEGENERATE_N_ACCEPTED
    got = run(ctx, c, st, th_mse_reprojection=400.0)
    same(got, NR.new_points(L, *D.ref_args(c), th_mse_reprojection=400.0))
    assert got["n_accepted"].tolist() == D.DEGENERATE_N_ACCEPTED_400
    assert (got["mse"][-12:] == 100000.0).all() and (got["vis_entry"][-12:] == 1).all() and (got["mse"][:-12] < 9.0).all()
    # an empty visible list, and no new camera at all
    e = dict(c, vis_off=np.array([0, 0], np.int32), vis_cam=np.zeros(0, np.int32))
    got = run(ctx, e, st)
    assert got["pt_off"].tolist() == [0, 0] and len(got["X"]) == 0 and len(got["n_matches"]) == 0 and got["h2d_bytes"] == 0
    e = dict(e, new_cam=np.zeros(0, np.int32), vis_off=np.array([0], np.int32))
    got = run(ctx, e, st)
    assert got["pt_off"].tolist() == [0] and len(got["mse"]) == 0
    st.close()


def test_independence(ctx, walk):
    """Three new cameras in one call equal three single calls, row for row."""
    st = ctx.match_store(*D.store_args(walk))
    whole = run(ctx, walk, st)
    same(whole, walk["ref"])
    assert (np.diff(whole["pt_off"]) > 0).all()
    for k in range(3):
        one = run(ctx, D.sub(walk, [k]), st)
        b, e = whole["pt_off"][k], whole["pt_off"][k + 1]
        assert one["pt_off"].tolist() == [0, e - b]                    # ids start at n_points for each
        for key in NR.POINT_KEYS:
            np.testing.assert_array_equal(one[key], whole[key][b:e], err_msg="%s of new camera %d" % (key, k))
        vb, ve = walk["vis_off"][k], walk["vis_off"][k + 1]
        for key in NR.ENTRY_KEYS:
            np.testing.assert_array_equal(one[key], whole[key][vb:ve], err_msg="%s of new camera %d" % (key, k))
    st.close()


def test_golden_fixture(ctx):
    """The committed answer of the restatement (tests/golden/make_newpoints_golden.py): library and restatement cannot drift together."""
    g = np.load(GOLD)
    c = {k: g[k] for k in D.INPUTS}
    got = run(ctx, c, **D.GOLDEN_OPTS)
    for k in NR.FETCHED:
        np.testing.assert_array_equal(np.asarray(got[k]), g["want_" + k], err_msg=k)
    assert np.diff(g["want_pt_off"]).tolist() == [66, 17] and g["want_large"].tolist() == [0, 0, 0, 1, 0, 0, 0]


def test_traffic(ctx, walk):
    """What crosses PCIe is bounded by the involved cameras' features: per camera its feat_point row (4 bytes a feature), its
    keypoint rows (8) and its pose (18 doubles); per visible entry 11 integers and two offsets.  Matches of pairs the walk does
    not touch change nothing.  The per-entry term is not a feature count: it is the 52 bytes a visible entry costs whatever
    its cameras hold (and once more for the closing offsets: 364 bytes here), added so that the bound stays an exact account of the upload; the part that guards
    against match-proportional traffic, the same byte count with 600 000 unrelated matches in the store, is an equality."""
    c = D.sub(walk, [0])
    involved = sorted(set(c["vis_cam"].tolist()) | set(c["new_cam"].tolist()))
    nf = c["n_features"][c["cam_img"][involved]]
    bound = int((12 * nf + 144).sum()) + 13 * 4 * (len(c["vis_cam"]) + 1)
    a = run(ctx, c)
    big = D.with_unrelated(c, 300000)
    b = run(ctx, big)
    print("h2d bytes:", a["h2d_bytes"], "bound:", bound, "matches in the store:", len(c["matches"]), len(big["matches"]))
    assert 0 < a["h2d_bytes"] <= bound and b["h2d_bytes"] == a["h2d_bytes"]
    same(b, a)


def test_errors(ctx, walk):
    c = D.sub(walk, [0])
    st = ctx.match_store(*D.store_args(c))
    nan = float("nan")

    def bad(words, keypoints=c["keypoints"], **kw):
        args = dict(zip(("cam_img", "feat_point", "n_points", "cam_R", "cam_t", "cam_c", "cam_fk", "new_cam", "vis_off", "vis_cam"), D.call_args(c)))
        opts = {k: kw.pop(k) for k in list(kw) if k not in args}
        args.update(kw)
        with pytest.raises(capi.MsfmError) as e:
            ctx.new_points(st, keypoints=keypoints, **args, **opts)
        assert e.value.code == A.MSFM_E_INVAL
        assert all(w in str(e.value) for w in words), str(e.value)
        same(run(ctx, c, st), walk["ref0"])                              # the context stays usable

    n = 65536
    bad(["n_new", "65535"], new_cam=np.zeros(n, np.int32), vis_off=np.zeros(n + 1, np.int32), vis_cam=np.zeros(0, np.int32))
    bad(["new_cam", "outside"], new_cam=[7])
    bad(["new_cam", "outside"], new_cam=[-1])
    bad(["vis_cam", "outside"], vis_cam=[0, 1, 2, 7, 4, 5])
    img = c["cam_img"].copy(); img[6] = 9
    bad(["cam_img", "no image"], cam_img=img)
    img = c["cam_img"].copy(); img[6] = img[2]
    bad(["two cameras"], cam_img=img, feat_point=np.full(int(c["n_features"][img].sum()), -1, np.int32))
    bad(["keypoints"], keypoints=None)
    for k in ("th_mse_reprojection", "th_angle_small", "th_angle_large"):
        bad(["NaN"], **{k: nan})
    bad(["th_mse_reprojection"], th_mse_reprojection=-1.0)
    bad(["th_mse_reprojection"], th_mse_reprojection=46340.0)
    bad(["th_matches_large"], th_matches_large=-1)
    st.close()


def test_agreement_with_the_existing_path(ctx, walk):
    """tracks.generate_new_points (Python walk, two contracted msfm_triangulate_midpoint_batch calls): same order, values to 1e-9."""
    c = D.sub(walk, [0])
    X, mse, cam2, f1, f2 = tracks.generate_new_points(ctx, *D.legacy_args(c, 0))
    st = ctx.match_store(*D.store_args(c))
    state = dict(cam_img=c["cam_img"], feat_point=c["feat_point"], pt_mse=np.zeros(D.N_POINTS), cam_R=c["cam_R"], cam_t=c["cam_t"], cam_c=c["cam_c"],
                 cam_fk=c["cam_fk"])
    r = newpoints.generate_new_points(ctx, st, state, 0, D.WALK_VISIBLE, keypoints=c["keypoints"])
    st.close()
    np.testing.assert_array_equal(r.cam2, cam2)
    np.testing.assert_array_equal(r.feat1, f1)
    np.testing.assert_array_equal(r.feat2, f2)
    np.testing.assert_allclose(r.X, X, rtol=1e-9, atol=0)
    np.testing.assert_allclose(r.mse, mse, rtol=1e-9, atol=0)
    np.testing.assert_array_equal(r.X, walk["ref0"]["X"])


def test_apply_new_points(ctx, walk):
    """apply_new_points: ids behind the existing points, inserts only where they took, and a second round finds nothing new."""
    c = D.sub(walk, [0])
    st = ctx.match_store(*D.store_args(c))
    state = dict(n_features=c["n_features"], cam_img=c["cam_img"], feat_point=c["feat_point"].copy(), cam_R=c["cam_R"], cam_t=c["cam_t"],
                 cam_c=c["cam_c"], cam_fk=c["cam_fk"], point_xyz=np.zeros((D.N_POINTS, 3)), pt_bad=np.zeros(D.N_POINTS, np.uint8),
                 pt_mse=np.zeros(D.N_POINTS), pt_views=np.full(D.N_POINTS, 3, np.int32))
    r = newpoints.generate_new_points(ctx, st, state, 0, D.WALK_VISIBLE, keypoints=c["keypoints"])
    before = state["feat_point"].copy()
    ids = newpoints.apply_new_points(state, r, new_cam=0)
    n = len(r.mse)
    assert ids.tolist() == list(range(D.N_POINTS, D.N_POINTS + n)) and len(state["pt_mse"]) == D.N_POINTS + n
    assert (state["pt_views"][-n:] == 2).all() and not state["pt_bad"][-n:].any() and (state["point_xyz"][-n:] == r.X).all()
    changed = np.nonzero(state["feat_point"] != before)[0]
    assert (before[changed] == -1).all() and len(changed) == int(r.takes1.sum()) + int(r.takes2.sum())
    cam_fo = np.concatenate([[0], np.cumsum(c["n_features"][c["cam_img"]])])
    first = {}
    for i in range(n):                                                   # std::map::insert in sorted order
        first.setdefault((0, int(r.feat1[i])), ids[i])
        first.setdefault((int(r.cam2[i]), int(r.feat2[i])), ids[i])
    assert all(state["feat_point"][cam_fo[cam] + f] == p for (cam, f), p in first.items())
    again = newpoints.generate_new_points(ctx, st, state, 0, D.WALK_VISIBLE, keypoints=c["keypoints"])
    assert len(again.mse) == 0
    st.close()


def test_store_from_chain_equals_store_from_its_matches(ctx):
    """Config 1 with 1500 requested features (as tests/test_gpu_seed.py): the store copied out of the verified chain, which holds
    the keypoints, and a store made from the fetched matches plus `keypoints` give equal sets."""
    sc = scene.add_features(scene.config_scene(1), 1500)
    kps = [np.ascontiguousarray(k, np.float32) for k in sc.kp_xy]
    pairs = scene.all_pairs(sc.n_cams)
    ds = ctx.descset(sc.desc, keypoints=kps)
    res = ds.match_pairs(pairs, 0.6, 0.85)
    ch = capi.Chain(res)
    n_m, ok, _ = ch.verify(3.0, seed=5)
    st_c = capi.MatchStore.from_chain(ch)
    fetched = [ch.fetch_matches(p) for p in range(len(pairs))]
    moff = np.concatenate([[0], np.cumsum(n_m)]).astype(np.int32)
    ch.close(); res.close(); ds.close()
    st_h = ctx.match_store([len(k) for k in kps], pairs, moff, np.concatenate(fetched))
    n = sc.n_cams
    R, t, cc, fk = scene.cameras_for_tracks(sc)
    fp = np.concatenate([np.where(p % 3 == 0, p, -1) for p in sc.feat_point]).astype(np.int32)   # a third of the points exist already
    args = (np.arange(n, dtype=np.int32), fp, sc.n_points, R, t, cc, fk, [n - 1, 0], [0, n, n + 3], list(range(n)) + [n - 1, 1, 2])
    a = ctx.new_points(st_c, *args)
    b = ctx.new_points(st_h, *args, keypoints=np.concatenate(kps))
    same(a, b)
    print("points:", np.diff(a["pt_off"]).tolist(), "matches per entry:", a["n_matches"].tolist())
    assert np.diff(a["pt_off"]).min() > 0 and a["n_matches"].max() > 100
    with pytest.raises(capi.MsfmError) as e:
        ctx.new_points(st_h, *args)                                      # neither the argument nor a chain's keypoints
    assert e.value.code == A.MSFM_E_INVAL and "keypoints" in str(e.value)
    st_c.close(); st_h.close()
