"""msfm_seed_hypotheses - the loop body of IncrementalSfM::FindSeedPairThenReconstruct (sfm_incremental.cc:235-390) for a list
of hypotheses on the resident match store - against the sequential restatement tests/seed_ref.cpp with the poses of
oracle.relpose_5pt / tests/relposef_ref.cpp: every fetched array identical, bit for bit."""
import os

import numpy as np
import pytest

from metricsfm_amd import _abi as A
from metricsfm_amd import capi, scene, seed
from tests import relposef_data as RF
from tests import seed_data as D
from tests import seed_ref as SR

pytestmark = pytest.mark.gpu
KEYS = SR.FETCHED + ("winner",)
GOLD = os.path.join(os.path.dirname(__file__), "golden", "seed_golden.npz")


@pytest.fixture(scope="module")
def refs(tmp_path_factory, oracle):
    d = tmp_path_factory.mktemp("seed_ref")
    return oracle, RF.build_ref(d), SR.build_ref(d)


@pytest.fixture(scope="module")
def mixed(refs):
    c = D.build_case(D.MIXED, 5)
    c["ref"] = D.expected(*refs, c)
    return c


@pytest.fixture(scope="module")
def gates(refs):
    c = D.build_case(D.GATES, 23)
    c["ref"] = D.expected(*refs, c)
    return c


def same(got, want, keys=KEYS):
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, w.dtype, g.shape, w.shape)
        np.testing.assert_array_equal(g, w, err_msg=k)


def run(ctx, c, st, rows=None, **opts):
    rows = slice(None) if rows is None else rows
    return ctx.seed_hypotheses(st, c["hyp_img"][rows], c["cam_fk"][rows], c["same_model"][rows], keypoints=c["keypoints"], **opts)


def test_mixed_batch_is_identical(ctx, mixed):
    st = ctx.match_store(*D.store_args(mixed))
    got = run(ctx, mixed, st)
    st.close()
    want = mixed["ref"]
    print("points per hypothesis:", np.diff(got["pt_off"]).tolist(), "pose_ok:", got["pose_ok"].tolist(), "winner:", got["winner"])
    same(got, want)
    assert want["n_matches"].tolist() == D.MIXED_COUNTS
    assert want["arm"].tolist() == [5, 5, 5, 5, 5, 8, 8, 8, 8, 5, 8, 8, 5, 5]
    assert want["pose_ok"].tolist() == [0, 0, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1]
    pts = np.diff(want["pt_off"])
    assert pts[9] == 301 and pts[10] > 1000 and pts[11] > 200 and pts[12] == 1500 and want["winner"] == 9
    # the focal rule (:324-332): a known f beside an unknown one is replaced too; one shared model gets the mean for both
    assert want["f"][7, 0] != D.F and want["f"][10, 1] != 4200.0 and want["f"][11, 0] == want["f"][11, 1] and want["f"][8, 0] == want["f"][8, 1]
    # a feature in two matches stays in both: match 300 repeats match 3
    b = want["pt_off"][9]
    np.testing.assert_array_equal(want["X"][b + 300], want["X"][b + 3])


def test_golden_fixture(ctx):
    """The committed answer of the restatement (tests/seed_data.py::write_golden): library and restatement cannot drift together."""
    g = np.load(GOLD)
    st = ctx.match_store(g["n_features"], g["pairs"], g["match_off"], g["matches"])
    got = ctx.seed_hypotheses(st, g["hyp_img"], g["cam_fk"], g["same_model"], keypoints=g["keypoints"])
    st.close()
    for k in KEYS:
        np.testing.assert_array_equal(np.asarray(got[k]), g["want_" + k], err_msg=k)
    assert g["want_pose_ok"].all() and g["want_winner"] == 4


def test_gates(ctx, gates):
    st = ctx.match_store(*D.store_args(gates))
    got = run(ctx, gates, st)
    same(got, gates["ref"])
    assert np.diff(got["pt_off"]).tolist() == D.GATES_POINTS          # (tests/test_seed_ref.py holds the restatement to the same)
    assert got["pass"].tolist() == D.GATES_PASS and got["winner"] == 2
    assert run(ctx, gates, st, [0, 1, 3])["winner"] == -1
    second = run(ctx, gates, st, [3, 4])
    assert second["pass"].tolist() == [0, 1] and second["winner"] == 1
    st.close()


def test_other_options(ctx, refs, mixed):
    """Looser gates accept points of the eight-point hypotheses whose rotation is large; other sample counts and seeds."""
    o = dict(th_mse_reprojection=400.0, th_angle_small=0.01, th_seedpair_structures=3, ransac_times_5pt=37, ransac_times_8pt=50,
             seed_5pt=11, seed_8pt=12)
    rows = [2, 6, 7, 8, 10, 13]
    st = ctx.match_store(*D.store_args(mixed))
    got = run(ctx, mixed, st, rows, **o)
    st.close()
    want = D.expected(*refs, mixed, mixed["hyp_img"][rows], mixed["cam_fk"][rows], mixed["same_model"][rows], **o)
    same(got, want)
    assert (np.diff(want["pt_off"])[[1, 2, 3]] > 0).all() and want["winner"] >= 0


def test_index_rule(ctx, mixed):
    """Hypothesis h of the batch equals the last hypothesis of a call whose first h entries name absent pairs."""
    st = ctx.match_store(*D.store_args(mixed))
    whole = mixed["ref"]
    for h in range(len(mixed["hyp_img"])):
        hyp = np.array([D.absent_pair(mixed)] * h + [tuple(mixed["hyp_img"][h])], np.int32)
        one = ctx.seed_hypotheses(st, hyp, mixed["cam_fk"][:h + 1], mixed["same_model"][:h + 1], keypoints=mixed["keypoints"])
        assert one["n_matches"][:h].tolist() == [0] * h and not one["pose_ok"][:h].any() and one["pt_off"][h] == 0
        for k in ("arm", "pose_ok", "pass", "n_matches", "f", "R", "t", "c"):
            np.testing.assert_array_equal(one[k][h], whole[k][h], err_msg="%s of hypothesis %d" % (k, h))
        b, e = whole["pt_off"][h], whole["pt_off"][h + 1]
        for k in ("pt_match", "X", "mse"):
            np.testing.assert_array_equal(one[k], whole[k][b:e], err_msg="%s of hypothesis %d" % (k, h))
        assert one["winner"] == (h if whole["pass"][h] else -1)
    st.close()


def test_store_from_chain_equals_store_from_its_matches(ctx):
    """Config 1 with 1500 requested features (as tests/test_gpu_localize.py): the store copied out of the verified chain, which
    holds the keypoints, and a store made from the fetched matches plus `keypoints` give equal sets."""
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
    graph = np.zeros((n, n), np.int32)
    graph[np.asarray(pairs)[:, 0], np.asarray(pairs)[:, 1]] = n_m
    hyp = seed.sort_image_pairs(graph, np.zeros(n, bool))[:8]
    assert len(hyp) == 8
    fk = np.zeros((8, 2, 3)); fk[:4, :, 0] = scene.FOCAL                     # four hypotheses on each arm
    same_model = np.array([1, 0] * 4, np.uint8)
    a = ctx.seed_hypotheses(st_c, hyp, fk, same_model)
    b = ctx.seed_hypotheses(st_h, hyp, fk, same_model, keypoints=np.concatenate(kps))
    same(a, b)
    assert a["n_matches"].min() > 100 and a["pose_ok"][:4].all()
    with pytest.raises(capi.MsfmError) as e:
        ctx.seed_hypotheses(st_h, hyp, fk, same_model)                      # neither the argument nor a chain's keypoints
    assert e.value.code == A.MSFM_E_INVAL and "keypoints" in str(e.value)
    st_c.close(); st_h.close()


def test_pose_is_the_existing_exports(ctx, refs, mixed):
    """pose_ok / R / t equal ctx.relpose_5pt / ctx.relpose_8pt on host-gathered arrays, the other arm's problems empty."""
    st = ctx.match_store(*D.store_args(mixed))
    got = run(ctx, mixed, st)
    st.close()
    nm, p1, p2 = SR.gather(refs[2], *D.store_args(mixed), mixed["keypoints"], mixed["hyp_img"])
    fk = mixed["cam_fk"]
    arm = np.where((fk[:, 0, 0] != 0) & (fk[:, 1, 0] != 0), 5, 8)
    b = D.arm_batches(arm, nm, p1, p2)
    five = ctx.relpose_5pt(*b[5], fk[:, 0, 0], fk[:, 1, 0])
    eight = ctx.relpose_8pt(*b[8])
    pose_ok, R, t, f8 = D.merge_poses(arm, five, eight)
    np.testing.assert_array_equal(got["pose_ok"], pose_ok)
    live = pose_ok == 1
    np.testing.assert_array_equal(got["R"][live], R[live])
    np.testing.assert_array_equal(got["t"][live], t[live])
    assert not got["R"][~live].any() and not got["t"][~live].any() and not got["c"][~live].any()
    for h in np.nonzero(live & (arm == 8))[0]:
        want = [(f8[h, 0] + f8[h, 1]) / 2.0] * 2 if mixed["same_model"][h] else list(f8[h])
        assert got["f"][h].tolist() == want


def test_points_agree_with_triangulate_midpoint(ctx, mixed):
    """X of the accepted points against msfm_triangulate_midpoint_batch on the same two-view tracks: that kernel is compiled
    with fused multiply-adds, this one is not - 1e-9, the bound tests/test_gpu_tri.py holds it to against its oracle."""
    st = ctx.match_store(*D.store_args(mixed))
    got = run(ctx, mixed, st)
    st.close()
    args, th, tm = D.two_view_tracks(mixed, got)
    X, mse, ok = ctx.triangulate_midpoint(A.TrackArrays(*args), D.OPTS["th_mse_reprojection"], D.OPTS["th_angle_small"])
    keep = ok == 1
    np.testing.assert_array_equal(np.bincount(th[keep], minlength=len(mixed["hyp_img"])), np.diff(got["pt_off"]))
    np.testing.assert_array_equal(tm[keep], got["pt_match"])
    np.testing.assert_allclose(got["X"], X[keep], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(got["mse"], mse[keep], rtol=1e-7, atol=1e-9)


def test_transfer_does_not_grow_with_the_store(ctx, gates):
    """The same hypotheses on a store that holds 200000 more matches (between the two spare images) send the same bytes."""
    nf, pairs, moff, m = D.store_args(gates)
    spare = D.absent_pair(gates)
    big = 200000
    st_small = ctx.match_store(nf, pairs, moff, m)
    st_big = ctx.match_store(nf, np.concatenate([pairs, [spare]]), np.concatenate([moff, [moff[-1] + big]]),
                             np.concatenate([m, np.zeros((big, 2), np.int32)]))
    a, b = run(ctx, gates, st_small), run(ctx, gates, st_big)
    st_small.close(); st_big.close()
    same(a, b)
    kp_bytes = int(nf[np.unique(gates["hyp_img"])].sum()) * 2 * 4
    assert a["h2d_bytes"] == b["h2d_bytes"]
    assert kp_bytes < a["h2d_bytes"] < kp_bytes + 4096 < big * 8


def test_two_calls_give_identical_bytes(ctx, mixed):
    st = ctx.match_store(*D.store_args(mixed))
    a, b = run(ctx, mixed, st), run(ctx, mixed, st)
    st.close()
    for k in KEYS:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


def test_launches_are_timed(ctx, gates):
    st = ctx.match_store(*D.store_args(gates))
    ctx.profile_reset()
    ctx.profile(True)
    try:
        run(ctx, gates, st)
        stats = ctx.profile_get()
    finally:
        ctx.profile(False)
        ctx.profile_reset()
    st.close()
    for name in ("seed_gather", "pose_e5_hyp", "pose_e5_score", "pose_e5_select", "seed_camera", "seed_triangulate", "seed_compact"):
        assert stats[name]["launches"] == 1, (name, stats)
    assert "pose_f8_hyp" not in stats                                       # no eight-point hypothesis: that arm is not launched


def test_bad_input_is_refused_and_the_context_stays_usable(ctx, gates):
    st = ctx.match_store(*D.store_args(gates))
    hyp, fk, sm, kp = gates["hyp_img"], gates["cam_fk"], gates["same_model"], gates["keypoints"]
    n_img = len(gates["n_features"])

    def refused(*words, **kw):
        args = dict(hyp_img=hyp, cam_fk=fk, same_model=sm, keypoints=kp)
        opts = {k: kw.pop(k) for k in list(kw) if k not in args}
        args.update(kw)
        with pytest.raises(capi.MsfmError) as e:
            ctx.seed_hypotheses(st, **args, **opts)
        assert e.value.code == A.MSFM_E_INVAL
        assert all(w in str(e.value) for w in words), str(e.value)
        same(run(ctx, gates, st), gates["ref"])

    def with_hyp(h, pair):
        out = hyp.copy(); out[h] = pair
        return out

    def with_f(h, cam, v):
        out = fk.copy(); out[h, cam, 0] = v
        return out

    refused("hypothesis 1", hyp_img=with_hyp(1, (2, n_img)))
    refused("hypothesis 2", hyp_img=with_hyp(2, (-1, 3)))
    refused("itself", hyp_img=with_hyp(0, (4, 4)))
    refused("keypoints", keypoints=None)
    refused("focal", cam_fk=with_f(3, 1, -1.0))
    refused("focal", cam_fk=with_f(0, 0, np.nan))
    refused("ransac_times", ransac_times_5pt=0)
    refused("ransac_times", ransac_times_8pt=65537)
    refused("threshold", th_mse_reprojection=np.nan)
    refused("threshold", th_angle_small=np.nan)
    refused("threshold", th_seedpair_structures=-1)
    too_many = 65536
    refused("n_hyp", hyp_img=np.tile(hyp[:1], (too_many, 1)), cam_fk=np.tile(fk[:1], (too_many, 1, 1)), same_model=np.zeros(too_many, np.uint8))
    empty = ctx.seed_hypotheses(st, np.zeros((0, 2), np.int32), np.zeros((0, 2, 3)), np.zeros(0, np.uint8), keypoints=kp)
    assert empty["winner"] == -1 and empty["pt_off"].tolist() == [0] and len(empty["arm"]) == 0
    st.close()


def test_find_seed_pair_walks_the_ranked_list_in_chunks(ctx, gates):
    """find_seed_pair on the gates store: image pairs ranked by SortImagePairs, chunks of k; the chunking changes a hypothesis'
    sample key, not what these exact pairs reconstruct.  The winner's arrays make a BaArrays."""
    nf, pairs, moff, m = D.store_args(gates)
    st = ctx.match_store(nf, pairs, moff, m)
    n = len(nf)
    graph = np.zeros((n, n), np.int32)
    graph[pairs[:, 0], pairs[:, 1]] = np.diff(moff)
    order = seed.sort_image_pairs(graph, np.zeros(n, bool)).tolist()
    passing = [tuple(p) for p, ok in zip(gates["hyp_img"].tolist(), D.GATES_PASS) if ok]
    first = min(order.index(list(p)) for p in passing)
    by_pair = {tuple(p): m[moff[k]:moff[k + 1]] for k, p in enumerate(pairs.tolist())}
    for k in (1, 2, 64):
        r = seed.find_seed_pair(ctx, st, graph, np.zeros(n, bool), np.full(n, D.F), np.arange(n), k=k, keypoints=gates["keypoints"],
                                pair_matches=lambda a, b: by_pair[(a, b)])
        assert r["images"] == tuple(order[first]) and r["n_visited"] == first + 1
        P = len(r["point"])
        assert P in (20, 25) and r["obs_xy"].shape == (2 * P, 2) and r["obs_cam"].tolist() == [0, 1] * P
        ba = A.BaArrays(r["cam_pose"], r["cam_model"], r["cam_model_of_cam"], r["point"], r["obs_cam"], r["obs_pt"], r["obs_xy"])
        assert ba.struct.n_obs == 2 * P and ba.struct.n_models == 2
    processed = np.zeros(n, bool)
    processed[[p[0] for p in passing]] = True
    assert seed.find_seed_pair(ctx, st, graph, processed, np.full(n, D.F), np.arange(n), keypoints=gates["keypoints"]) is None
    st.close()
