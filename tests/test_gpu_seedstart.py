"""Starting a model on the device: msfm_recon_create_from_seed on the winner a msfm_seed_set keeps resident, msfm_recon_normalize /
msfm_recon_set_cameras, and incremental.start_model / reconstruct through both backends.  Every comparison is array for array
and bit for bit: against the host assembly of the same seed (seed.find_seed_pair with the match callback +
tests/seedstart_ref.py::state_from_seed), against the literal loops of seedstart_ref.normalize, and against the flat
adjust.adjust_round + apply_round on the same arrays."""
import numpy as np
import pytest

from metricsfm_amd import _abi as A
from metricsfm_amd import adjust, capi, incremental
from tests import relposef_data as RF
from tests import resident_data as RD
from tests import seed_data as D
from tests import seed_ref as SR
from tests import seedstart_data as SD
from tests import seedstart_ref as REF

pytestmark = pytest.mark.gpu
SUMMARY = ("termination", "num_iterations", "num_successful_steps", "num_unsuccessful_steps", "initial_cost", "final_cost", "num_residuals",
           "num_reduced_params")
COUNTS = ("count_outliers", "count_new_add", "count_outliers_new_add")
FULL4 = dict(full_options=dict(max_num_iterations=4))


def same(got, want, keys=RD.FETCHED):
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, w.dtype, g.shape, w.shape)
        np.testing.assert_array_equal(g, w, err_msg=k)


def same_solves(got, want):
    same(got, want, ("solved",))
    for k in COUNTS:
        assert got[k] == want[k], (k, got[k], want[k])
    for g, w in zip(got["summary"], want["summary"]):
        assert (g is None) == (w is None)
        if g is not None:
            for k in SUMMARY:
                assert g[k] == w[k], (k, g[k], w[k])
            np.testing.assert_array_equal(g["iterations"], w["iterations"])


def refused(code, fn, *a, **kw):
    with pytest.raises(capi.MsfmError) as e:
        fn(*a, **kw)
    assert e.value.code == code, e.value
    return str(e.value)


@pytest.fixture(scope="module")
def seeds(ctx):
    """name -> (case, store, the host-assembled seed of the parent's route, its flat state), made once."""
    made = {}

    def get(name):
        if name not in made:
            c = SD.seed_case(name)
            st = ctx.match_store(*D.store_args(c))
            host = SD.find(ctx, st, c, pair_matches=lambda a, b: c["by_pair"][(a, b)])
            assert host is not None and host["n_visited"] == 2 and host["images"] == tuple(c["hyp_img"][1])
            made[name] = (c, st, host, REF.state_from_seed(host, c["n_features"]))
        return made[name]
    yield get
    for _, st, _, _ in made.values():
        st.close()


def resident(ctx, c, st, **kw):
    """The resident route: find_seed_pair(keep=True) -> Recon.from_seed; the set is closed behind the call."""
    kept = SD.find(ctx, st, c, keep=True)
    assert "obs_feature" not in kept
    with kept["set"] as s:
        q = capi.Recon.from_seed(ctx, st, s, kept["cam_pose"], kept["cam_model"], kept["cam_model_of_cam"], keypoints=c["keypoints"], **kw)
    return kept, q


@pytest.mark.parametrize("name", list(SD.SEED_CASES))
def test_state_from_seed(ctx, seeds, name):
    c, st, host, want = seeds(name)
    kept, q = resident(ctx, c, st)
    try:
        for k in ("point", "mse", "pt_match", "cam_pose", "cam_model", "cam_model_of_cam"):
            np.testing.assert_array_equal(kept[k], host[k], err_msg=k)
        P = len(host["point"])
        z = q.size()
        assert (z["n_cams"], z["n_points"], z["n_obs"]) == (2, P, 2 * P) and z["n_models"] == len(host["cam_model"])
        assert z["h2d_bytes"] == c["keypoints"].nbytes            # a host-made store: the keypoints, as msfm_recon_create; nothing per point
        got = q.fetch()
        same(got, want)
        assert got["pt_views"].tolist() == [2] * P and got["pt_new_added"].all() and got["pt_mutable"].all() and not got["pt_bad"].any()
        if name == "dup":
            ptm = host["pt_match"].tolist()
            assert 3 in ptm and 300 in ptm                        # (tests/test_seedstart_ref.py: the restatement accepts both)
            lo, hi = ptm.index(3), ptm.index(300)
            assert got["obs_feat"][2 * lo] == got["obs_feat"][2 * hi] == 3 and got["feat_point"][3] == lo < hi
            assert (got["obs_point"] == hi).sum() == 2 and (got["obs_point"] == lo).sum() == 2
            f2 = got["obs_feat"][2 * lo + 1]
            assert got["obs_feat"][2 * hi + 1] == f2 and got["feat_point"][c["n_features"][got["cam_img"][0]] + f2] == lo
        if name == "eight":
            assert len(got["cam_model"]) == 2 and got["cam_fk"][:, 1:].any() and P > 1000
        if name == "shared":
            assert len(got["cam_model"]) == 1 and got["cam_fk"][0, 0] == got["cam_fk"][1, 0]
    finally:
        q.close()


def test_dup_case_accepts_both_matches_of_feature_3(tmp_path, oracle):
    """The condition of the repeated-feature case, from the restatement's own answer."""
    c = SD.seed_case("dup")
    want = D.expected(oracle, RF.build_ref(tmp_path), SR.build_ref(tmp_path), c)
    assert want["winner"] == 1 and {3, 300} <= set(want["pt_match"][want["pt_off"][1]:].tolist())


@pytest.fixture(scope="module")
def planted(ctx):
    """P -> (store, case) of RD.commit_case(P): a host-made state of P points."""
    made = {}

    def get(P):
        if P not in made:
            c = RD.commit_case(P)
            made[P] = (ctx.match_store(*c["store"]), c)
        return made[P]
    yield get
    for st, _ in made.values():
        st.close()


@pytest.mark.parametrize("with_noise", [False, True])
@pytest.mark.parametrize("P", [1, 63, 257, 1500])
def test_normalize_is_the_ordered_sum(ctx, planted, P, with_noise):
    """msfm_recon_normalize against the literal loop on clouds whose sums depend on their order (tests/test_seedstart_ref.py
    shows that a pairwise sum gives other bits).  One point has mad = 0: scale = 100 / 0, which the loop returns as inf and the
    library refuses with MSFM_E_NUMERIC, the state untouched."""
    st, c = planted(P)
    state = dict(c["state"], point_xyz=SD.planted_points(P))
    noise = np.random.default_rng(100 + P).standard_normal((P, 3)) if with_noise else None
    q = ctx.recon(st, state, c["cam_pose"], c["cam_model"], c["cam_model_of_cam"], keypoints=c["keypoints"])
    flat = dict(state, cam_pose=c["cam_pose"], cam_model=c["cam_model"], cam_model_of_cam=np.asarray(c["cam_model_of_cam"], np.int32))
    try:
        before = q.size()["h2d_bytes"]
        mid, scale, out = REF.normalize(state["point_xyz"], noise)
        if P == 1:
            assert scale == float("inf")
            assert "not finite" in refused(A.MSFM_E_NUMERIC, q.normalize, noise)
            same(q.fetch(), flat)
            return
        g_mid, g_scale = q.normalize(noise)
        np.testing.assert_array_equal(g_mid, mid)
        assert g_scale == scale
        assert q.size()["h2d_bytes"] - before == (24 * P if with_noise else 0)
        same(q.fetch(), dict(flat, point_xyz=out))
    finally:
        q.close()


@pytest.mark.parametrize("name", ["gates", "dup"])
def test_initial_adjustment(ctx, seeds, name):
    """from_seed, normalize with noise, set_cameras, adjust(full, outliers) against the restatement's normalise + perturb and the
    flat adjust_round + apply_round on the same arrays: state, summaries and iteration rows."""
    c, st, host, want0 = seeds(name)
    P = len(host["point"])
    rng = np.random.default_rng(11)
    noise_p, noise_c = rng.standard_normal((P, 3)), rng.standard_normal((2, 2, 3))
    # flat
    state = {k: np.array(v) for k, v in want0.items() if k not in ("cam_pose", "cam_model", "cam_model_of_cam")}
    state["n_features"] = np.array(c["n_features"])
    mid, scale, state["point_xyz"] = REF.normalize(state["point_xyz"], noise_p)
    pose, state["cam_R"], state["cam_t"], state["cam_c"] = incremental.normalize_cameras(host["cam_pose"], host["cam_c"], mid, scale, noise_c)
    want = adjust.adjust_round(ctx, st, state, pose, host["cam_model"], host["cam_model_of_cam"], -1, [], partial=False, full=True, keypoints=c["keypoints"],
                               **FULL4)
    pose, model = adjust.apply_round(state, want)
    # resident
    kept, q = resident(ctx, c, st)
    try:
        g_mid, g_scale = q.normalize(noise_p)
        np.testing.assert_array_equal(g_mid, mid)
        assert g_scale == scale
        q.set_cameras(*incremental.normalize_cameras(kept["cam_pose"], kept["cam_c"], g_mid, g_scale, noise_c))
        got = q.adjust(-1, [], partial=False, full=True, outliers=True, **FULL4)
        same_solves(got, want)
        assert want["solved"][1] == 1 and want["summary"][1]["num_iterations"] >= 1
        same(q.fetch(), dict(state, cam_pose=pose, cam_model=model, cam_model_of_cam=np.asarray(host["cam_model_of_cam"], np.int32)))
    finally:
        q.close()


def test_refusals_leave_everything_usable(ctx, seeds):
    c, st, host, want = seeds("gates")
    n = len(c["n_features"])
    kept = SD.find(ctx, st, c, keep=True)
    args = (kept["cam_pose"], kept["cam_model"], kept["cam_model_of_cam"])
    other = ctx.match_store(*D.store_args(c))
    loser = ctx.seed_hypotheses(st, c["hyp_img"][:1], c["cam_fk"][:1], c["same_model"][:1], keypoints=c["keypoints"], keep=True)
    try:
        inval = A.MSFM_E_INVAL
        assert loser["winner"] == -1
        assert "no winner" in refused(inval, capi.Recon.from_seed, ctx, st, loser["set"], *args, keypoints=c["keypoints"])
        assert "another store" in refused(inval, capi.Recon.from_seed, ctx, other, kept["set"], *args, keypoints=c["keypoints"])
        three = np.tile(kept["cam_model"][:1], (3, 1))
        assert "n_models" in refused(inval, capi.Recon.from_seed, ctx, st, kept["set"], kept["cam_pose"], three, [0, 1], keypoints=c["keypoints"])
        assert "n_models" in refused(inval, capi.Recon.from_seed, ctx, st, kept["set"], kept["cam_pose"], np.zeros((0, 3)), [0, 0], keypoints=c["keypoints"])
        assert "cam_model_of_cam[1]" in refused(inval, capi.Recon.from_seed, ctx, st, kept["set"], kept["cam_pose"], kept["cam_model"], [0, 2],
                                                keypoints=c["keypoints"])
        assert "cam_model_of_cam[0]" in refused(inval, capi.Recon.from_seed, ctx, st, kept["set"], kept["cam_pose"], kept["cam_model"], [-1, 0],
                                                keypoints=c["keypoints"])
        assert "no keypoints of image" in refused(inval, capi.Recon.from_seed, ctx, st, kept["set"], *args)
        # the set and the context still answer
        q = capi.Recon.from_seed(ctx, st, kept["set"], *args, keypoints=c["keypoints"])
        try:
            same(q.fetch(), want)
            # all points equal: mad = 0
            flat = dict(want, point_xyz=np.tile([1.0, 2.0, 3.0], (len(want["pt_mse"]), 1)))
            e = ctx.recon(st, dict(flat, n_features=c["n_features"]), flat["cam_pose"], flat["cam_model"], flat["cam_model_of_cam"], keypoints=c["keypoints"])
            try:
                assert "not finite" in refused(A.MSFM_E_NUMERIC, e.normalize)
                same(e.fetch(), flat)
            finally:
                e.close()
            # a state without points
            empty = dict(want, **{k: np.asarray(want[k])[:0] for k in ("obs_point", "obs_cam", "obs_feat", "point_xyz", "pt_bad", "pt_mse", "pt_views",
                                                                       "pt_mutable", "pt_new_added")})
            empty["feat_point"] = np.full(len(want["feat_point"]), -1, np.int32)
            z = ctx.recon(st, dict(empty, n_features=c["n_features"]), empty["cam_pose"], empty["cam_model"], empty["cam_model_of_cam"],
                          keypoints=c["keypoints"])
            try:
                assert "no point" in refused(inval, z.normalize)
                same(z.fetch(), empty)
            finally:
                z.close()
            mid, scale = q.normalize()                            # the next valid call succeeds
            r_mid, r_scale, out = REF.normalize(want["point_xyz"])
            assert scale == r_scale
            same(q.fetch(), dict(want, point_xyz=out))
        finally:
            q.close()
    finally:
        kept["set"].close(); loser["set"].close(); other.close()
    assert n == len(st.n_features)


def test_traffic_does_not_scale_with_the_points(ctx):
    """from_seed on a chain-made store sends the same bytes for a seed of about 300 and of about 1500 points."""
    sent, points = [], []
    for n in (300, 1500):
        st, _, n_m, _, close = SD.chain_pairs(ctx, [dict(n=n, kw=dict(outlier_frac=0.0))], 31)
        graph = np.array([[0, n_m[0]], [0, 0]], np.int32)
        kept = incremental.seedpair.find_seed_pair(ctx, st, graph, np.zeros(2, bool), np.full(2, D.F), np.arange(2), keep=True)
        assert kept is not None
        with kept["set"] as s:
            q = capi.Recon.from_seed(ctx, st, s, kept["cam_pose"], kept["cam_model"], kept["cam_model_of_cam"])
        z = q.size()
        sent.append(z["h2d_bytes"]); points.append(z["n_points"])
        got = q.fetch()
        np.testing.assert_array_equal(got["point_xyz"], kept["point"])
        q.close(); close()
    print("points", points, "bytes", sent)
    assert points[0] > 250 and points[1] > 1250 and sent[0] == sent[1] < 4096


@pytest.fixture(scope="module")
def models(ctx):
    """incremental.reconstruct through both backends on the two strips; the state after the seed and after every round is kept."""
    c = SD.strips_case()
    out = {}
    for cls in (incremental.FlatBackend, incremental.ResidentBackend):
        st = ctx.match_store(*c["store"])
        book = incremental.Book(**c["book"])
        states = []
        ms = incremental.reconstruct(cls, ctx, st, book, noise_seed=5, keypoints=c["keypoints"], pair_matches=lambda a, b: c["by_pair"][(a, b)],
                                     on_round=lambda m, b: states.append((m, b.fetch())))
        out[cls.__name__] = (ms, states, book)
        st.close()
    return out


def test_whole_models(models):
    (flat, f_states, f_book), (res, r_states, r_book) = models["FlatBackend"], models["ResidentBackend"]
    assert len(flat) == len(res) == 2
    assert len(f_states) == len(r_states)
    for (mf, sf), (mr, sr) in zip(f_states, r_states):
        assert mf == mr
        same(sr, sf)
    for a, b in zip(res, flat):
        assert a["seed"]["images"] == b["seed"]["images"] and a["seed"]["n_points"] == b["seed"]["n_points"] and a["seed"]["scale"] == b["seed"]["scale"]
        np.testing.assert_array_equal(a["seed"]["mid"], b["seed"]["mid"])
        same_solves(a["seed"], b["seed"])
        assert len(a["rounds"]) == len(b["rounds"])
        for g, w in zip(a["rounds"], b["rounds"]):
            for k in ("image", "failed_images", "image_ids", "visible", "n_new", "full") + COUNTS:
                if k in w or k in g:
                    assert g[k] == w[k], (k, g[k], w[k])
            if w["image"] >= 0:
                same(g, w, ("R", "t"))
                same_solves(g, w)
        same(a["state"], b["state"])
    np.testing.assert_array_equal(r_book.processed, f_book.processed)
    # what keeps the comparison from passing empty
    imgs = [set(m["state"]["cam_img"].tolist()) for m in flat]
    print("models:", [sorted(s) for s in imgs], "rounds:", [[r["image"] for r in m["rounds"]] for m in flat])
    assert not (imgs[0] & imgs[1]) and all(len(s) >= 4 for s in imgs)
    assert any(r.get("full") and r["solved"][1] for m in flat for r in m["rounds"])
    for m in flat:
        first = m["rounds"][0]
        strip = m["seed"]["images"][0] // SD.STRIP_IMAGES
        assert first["image"] >= 0 and all(i // SD.STRIP_IMAGES == strip for i in first["image_ids"])
    assert not flat[1]["seed"]["fail_times"].any() and not res[1]["seed"]["fail_times"].any()      # ClearModel
