"""msfm_recon - a model's flat state resident on the device - against the flat calls it replaces: after every resident call
`Recon.fetch()` must equal the dict the flat functions leave, array for array, dtype and shape included, and the call's record
(counts, solved, summaries iteration row for iteration row, the assembled problems) must equal the flat call's.  No tolerance:
the kernels and their inputs are the same."""
import itertools

import numpy as np
import pytest

from metricsfm_amd import _abi as A
from metricsfm_amd import adjust, capi, incremental, newpoints, scene
from tests import newpoints_data as ND
from tests import resident_data as RD
from tests import round_data as D

pytestmark = pytest.mark.gpu
SUMMARY = ("termination", "num_iterations", "num_successful_steps", "num_unsuccessful_steps", "initial_cost", "final_cost", "num_residuals",
           "num_reduced_params")
PROBLEM = ("kept", "obs_cam", "obs_pt", "obs_xy", "pt_weight", "cam_mutable", "pt_mutable")
RECORD = ("cam_pose", "cam_model", "cam_R", "cam_t", "cam_c", "cam_fk", "adjust_cams", "adjust_pts", "solved")
QUICK = dict(partial_options=dict(max_num_iterations=3), full_options=dict(max_num_iterations=3))


@pytest.fixture(scope="module")
def main():
    return D.main_case()


def same(got, want, keys):
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, w.dtype, g.shape, w.shape)
        np.testing.assert_array_equal(g, w, err_msg=k)


def same_record(got, want, keep_problem):
    same(got, want, RECORD)
    for k in ("count_outliers", "count_new_add", "count_outliers_new_add"):
        assert got[k] == want[k], (k, got[k], want[k])
    for g, w in zip(got["summary"], want["summary"]):
        assert (g is None) == (w is None)
        if g is not None:
            for k in SUMMARY:
                assert g[k] == w[k], (k, g[k], w[k])
            np.testing.assert_array_equal(g["iterations"], w["iterations"])
    if keep_problem:
        for g, w in zip(got["problem"], want["problem"]):
            same(g, w, PROBLEM)


class Pair:
    """The same state twice: a flat dict with its parameter blocks, and a Recon made from it."""

    def __init__(self, ctx, c, **kw):
        self.ctx, self.c = ctx, c
        self.store = ctx.match_store(*D.store_args(c))
        self.state = RD.flat_state(c)
        self.pose, self.model = np.array(c["cam_pose"]), np.array(c["cam_model"])
        self.recon = ctx.recon(self.store, self.state, self.pose, self.model, c["cam_model_of_cam"], keypoints=c["keypoints"], **kw)

    def flat(self):
        return dict(self.state, cam_pose=self.pose, cam_model=self.model, cam_model_of_cam=np.asarray(self.c["cam_model_of_cam"], np.int32))

    def check(self):
        same(self.recon.fetch(), self.flat(), RD.FETCHED)

    def adjust(self, new_cam, visible, **kw):
        """The round's adjustment through both; returns (flat record, resident record)."""
        want = adjust.adjust_round(self.ctx, self.store, self.state, self.pose, self.model, self.c["cam_model_of_cam"], new_cam, visible,
                                   keypoints=self.c["keypoints"], **kw)
        self.pose, self.model = adjust.apply_round(self.state, want)
        got = self.recon.adjust(new_cam, visible, **kw)
        return want, got

    def close(self):
        self.recon.close()
        self.store.close()


def test_create_fetch_size(ctx, main):
    p = Pair(ctx, main, reserve_points=1000, reserve_obs=7)
    try:
        p.check()
        z = p.recon.size()
        n, no = len(main["pt_bad"]), len(main["obs_point"])
        assert (z["n_cams"], z["n_models"], z["n_points"], z["n_obs"]) == (8, 2, n, no)
        assert z["cap_points"] == 1000 > n and z["cap_obs"] == no > 7
        st = p.state
        sent = sum(st[k].nbytes for k in ("feat_point", "obs_point", "obs_cam", "obs_feat", "point_xyz", "pt_bad", "pt_mse", "pt_views", "pt_mutable",
                                          "pt_new_added")) + main["keypoints"].nbytes + 4 * (8 + 1)
        assert z["h2d_bytes"] == sent
    finally:
        p.close()


@pytest.mark.parametrize("stages", list(itertools.product([False, True], repeat=3)), ids=lambda s: "".join("pfo"[k] if s[k] else "-" for k in range(3)))
def test_adjust_stages(ctx, main, stages):
    """Every subset of partial / full / outliers on one state with keep_problem, then a second adjustment on what the first
    left (the full one with the outliers), each against adjust_round + apply_round."""
    partial, full, outliers = stages
    p = Pair(ctx, main)
    try:
        want, got = p.adjust(main["new_cam"], main["visible"], partial=partial, full=full, outliers=outliers, keep_problem=1, **QUICK)
        same_record(got, want, True)
        p.check()
        assert got["solved"].tolist() == [int(partial), int(full)]
        assert (got["count_outliers"] > 0) == outliers
        if partial:     # (the three iterations of a full stage alone are all rejected on this state: only the partial stage is known to move it)
            assert (p.state["point_xyz"] != main["point_xyz"]).any()
        want, got = p.adjust(main["new_cam"], main["visible"], partial=False, full=True, outliers=True, **QUICK)
        same_record(got, want, False)
        p.check()
        assert "point_xyz" not in got and got["h2d_bytes"] < want["h2d_bytes"]
    finally:
        p.close()


SKIPPED = {"all_bad": lambda: D.sized_case(40, all_bad=True), "empty": D.empty_case, "no_rows": D.points_without_rows_case}


@pytest.mark.parametrize("name", list(SKIPPED))
def test_adjust_stage_skipped(ctx, name):
    c = SKIPPED[name]()
    p = Pair(ctx, c)
    try:
        p.check()
        want, got = p.adjust(c["new_cam"], c["visible"], partial=True, full=True, outliers=True, keep_problem=1, **QUICK)
        same_record(got, want, True)
        assert got["solved"].tolist() == [0, 0]
        p.check()
    finally:
        p.close()


def test_traffic_does_not_scale_with_the_state(ctx, main):
    """5 000 more points with two rows each on cameras that are neither free nor visible: the resident adjustment sends the
    same bytes for both states; the flat call's h2d_bytes grows by at least the new points' arrays, so the counter counts."""
    K = 5000
    small, big = Pair(ctx, main), Pair(ctx, RD.with_unrelated(main, K))
    try:
        sent = []
        for p in (small, big):
            before = p.recon.size()["h2d_bytes"]
            want, got = p.adjust(main["new_cam"], main["visible"], partial=True, full=False, outliers=True, **QUICK)
            same_record(got, want, False)
            p.check()
            after = p.recon.size()["h2d_bytes"]
            assert after - before == got["h2d_bytes"] > 0
            sent.append((after - before, want["h2d_bytes"]))
        assert sent[0][0] == sent[1][0]
        assert sent[1][1] - sent[0][1] >= K * (24 + 8 + 1 + 1 + 1) + 2 * K * 12
        assert big.recon.size()["h2d_bytes"] - small.recon.size()["h2d_bytes"] >= K * (24 + 8 + 1 + 1 + 1) + 2 * K * 12   # (at creation)
    finally:
        small.close()
        big.close()
    # the new points: the same walk on a state of 1 000 and of 6 000 points
    c = ND.sub(ND.walk_case(ND.SEED_WALK), [0])
    small, big = NewPointsPair(ctx, c), NewPointsPair(ctx, dict(c, n_points=np.int32(ND.N_POINTS + K)))
    try:
        sent = []
        for p in (small, big):
            before = p.recon.size()["h2d_bytes"]
            want, got = p.new_points()
            p.check()
            assert p.recon.size()["h2d_bytes"] - before == got["h2d_bytes"] > 0
            sent.append(got["h2d_bytes"])
        assert sent[0] == sent[1] < want["h2d_bytes"]
    finally:
        small.close()
        big.close()


def refused(fn, *a, **kw):
    with pytest.raises(capi.MsfmError) as e:
        fn(*a, **kw)
    assert e.value.code == A.MSFM_E_INVAL, e.value
    return str(e.value)


def test_refusals_leave_the_state(ctx, main):
    c = main
    n_cams, n_points = len(c["cam_img"]), len(c["pt_bad"])
    p = Pair(ctx, c)
    try:
        assert "new_cam" in refused(p.recon.adjust, n_cams, c["visible"])
        p.check()
        assert "visible[1]" in refused(p.recon.adjust, c["new_cam"], [7, n_cams])
        p.check()
        assert "visible[0]" in refused(p.recon.adjust, c["new_cam"], [-1])
        p.check()
        assert "do_partial without new_cam" in refused(p.recon.adjust, -1, c["visible"])
        p.check()
        for th in (np.nan, -1.0):
            assert "th_mse_outliers" in refused(p.recon.adjust, c["new_cam"], c["visible"], th_mse_outliers=th)
            p.check()
        assert "weight" in refused(p.recon.adjust, c["new_cam"], c["visible"], weight_partial=np.nan)
        p.check()
        # a state that is refused at creation: an image listed twice, a feat_point entry >= n_points, a row outside its array
        def create(**edit):
            st = dict(p.state)
            for k, (at, value) in edit.items():
                st[k] = np.array(st[k])
                st[k][at] = value
            ctx.recon(p.store, st, c["cam_pose"], c["cam_model"], c["cam_model_of_cam"], keypoints=c["keypoints"]).close()
        twice = dict(p.state, cam_img=np.array(c["cam_img"]))
        twice["cam_img"][1] = c["cam_img"][0]
        twice["feat_point"] = np.full(int(c["n_features"][twice["cam_img"]].sum()), -1, np.int32)
        assert "two cameras" in refused(ctx.recon, p.store, twice, c["cam_pose"], c["cam_model"], c["cam_model_of_cam"], keypoints=c["keypoints"])
        fo = np.concatenate([[0], np.cumsum(c["n_features"][c["cam_img"]])])
        assert "feat_point of camera 3, feature 2" in refused(create, feat_point=(fo[3] + 2, n_points))
        assert "observation 17" in refused(create, obs_cam=(17, n_cams))
        assert "observation 17" in refused(create, obs_point=(17, -1))
        assert "no keypoints of image" in refused(ctx.recon, p.store, p.state, c["cam_pose"], c["cam_model"], c["cam_model_of_cam"])
        create()
        # the object and the context still answer: a good round matches the flat one
        want, got = p.adjust(c["new_cam"], c["visible"], partial=True, outliers=True, keep_problem=1, **QUICK)
        same_record(got, want, True)
        p.check()
    finally:
        p.close()


NEW_POINTS = ("pt_off", "cam2", "feat1", "feat2", "vis_entry", "pt_match", "X", "mse", "takes1", "takes2", "n_matches", "large", "n_candidates",
              "n_accepted")


class NewPointsPair:
    """A newpoints_data case as a flat state and as a Recon over the same store."""

    def __init__(self, ctx, c, **kw):
        self.ctx, self.c = ctx, c
        self.store = ctx.match_store(*ND.store_args(c))
        self.state, self.pose, self.model, self.moc = RD.newpoints_state(c)
        self.recon = ctx.recon(self.store, self.state, self.pose, self.model, self.moc, keypoints=c["keypoints"], **kw)

    def check(self):
        same(self.recon.fetch(), dict(self.state, cam_pose=self.pose, cam_model=self.model, cam_model_of_cam=self.moc), RD.FETCHED)

    def new_points(self, k=0, **opts):
        """New camera k of the case through both: generate_new_points + apply_new_points, and Recon.new_points.  Returns the
        flat call's dict and the resident one's."""
        c = self.c
        new_cam, visible = int(c["new_cam"][k]), c["vis_cam"][c["vis_off"][k]:c["vis_off"][k + 1]]
        want = self.ctx.new_points(self.store, self.state["cam_img"], self.state["feat_point"], len(self.state["pt_mse"]), self.state["cam_R"],
                                   self.state["cam_t"], self.state["cam_c"], self.state["cam_fk"], [new_cam], [0, len(visible)], visible,
                                   keypoints=c["keypoints"], **opts)
        newpoints.apply_new_points(self.state, newpoints.NewPoints(*(want[k] for k in newpoints.NewPoints._fields)), new_cam)
        got = self.recon.new_points(new_cam, visible, stats=True, **opts)
        same(got, want, NEW_POINTS)
        assert got["n_new"] == len(want["mse"])
        return want, got

    def close(self):
        self.recon.close()
        self.store.close()


@pytest.mark.parametrize("n", [0, 1, 256, 257])
def test_new_points_sizes(ctx, n):
    p = NewPointsPair(ctx, RD.two_camera_case(n))
    try:
        want, got = p.new_points()
        assert got["n_new"] == n and want["takes1"].all() and want["takes2"].all()
        p.check()
        z = p.recon.size()
        assert (z["n_points"], z["n_obs"]) == (ND.N_POINTS + n, 2 * n)
        assert p.recon.new_points(0, [1]) == 0     # every match is triangulated now; without stats only the count comes back
        p.check()
    finally:
        p.close()


def test_new_points_claims_and_lists(ctx):
    """Several points that name one slot (claims_case: takes1 / takes2 = 0 for the later ones), then the walk case: a visible
    list with the camera itself, and one with a camera listed twice - each new camera appended behind the one before."""
    c = ND.claims_case(ND.SEED_CLAIMS)
    p = NewPointsPair(ctx, c)
    try:
        want, _ = p.new_points()
        assert (want["takes1"] == 0).any() and (want["takes2"] == 0).any() and want["takes1"].any()
        p.check()
    finally:
        p.close()
    c = ND.walk_case(ND.SEED_WALK)
    assert c["vis_cam"][c["vis_off"][0]] == c["new_cam"][0] and c["vis_cam"][c["vis_off"][2]:c["vis_off"][3]].tolist() == [3, 0, 0]
    p = NewPointsPair(ctx, c)
    try:
        for k in range(3):
            want, got = p.new_points(k)
            assert got["n_new"] > 0
            p.check()
        # the rows that were appended carry real observations: the outlier stage of the adjustment reads them
        want = adjust.adjust_round(ctx, p.store, p.state, p.pose, p.model, p.moc, -1, [], keypoints=c["keypoints"], partial=False, full=False)
        p.pose, p.model = adjust.apply_round(p.state, want)
        got = p.recon.adjust(-1, [], partial=False, full=False)
        same_record(got, want, False)
        assert np.isfinite(p.state["pt_mse"][ND.N_POINTS:]).all()
        p.check()
    finally:
        p.close()


def test_growth_crosses_capacity(ctx):
    """The same appends with room reserved for all of them and with none: one run grows its arrays (twice the need), the other
    does not, and both leave the flat functions' state."""
    c = ND.walk_case(ND.SEED_WALK)
    tight, roomy = NewPointsPair(ctx, c, reserve_points=ND.N_POINTS + 100, reserve_obs=200), NewPointsPair(ctx, c, reserve_points=4000, reserve_obs=8000)
    try:
        caps = []
        for p in (tight, roomy):
            before = p.recon.size()
            want, got = p.new_points(0)
            after = p.recon.size()
            p.check()
            caps.append((before["cap_points"], before["cap_obs"], after["cap_points"], after["cap_obs"], got["n_new"]))
        n = caps[0][4]
        assert n == sum(ND.WALK_N_ACCEPTED) > 100
        assert caps[0] == (ND.N_POINTS + 100, 200, 2 * (ND.N_POINTS + n), 4 * n, n)
        assert caps[1] == (4000, 8000, 4000, 8000, n)
        same(tight.recon.fetch(), roomy.recon.fetch(), RD.FETCHED)
    finally:
        tight.close()
        roomy.close()


def test_new_points_refusals_leave_the_state(ctx):
    c = ND.sub(ND.walk_case(ND.SEED_WALK), [0])
    p = NewPointsPair(ctx, c)
    try:
        n_cams = len(c["cam_img"])
        assert "new_cam[0]" in refused(p.recon.new_points, n_cams, [1])
        assert "vis_cam[1]" in refused(p.recon.new_points, 0, [1, n_cams])
        assert "NaN" in refused(p.recon.new_points, 0, [2], th_angle_small=float("nan"))
        assert "th_mse_reprojection" in refused(p.recon.new_points, 0, [2], th_mse_reprojection=-1.0)
        p.check()
        p.new_points()
        p.check()
    finally:
        p.close()


def test_store_from_chain(ctx, chain_stores):
    """One round - localize, commit, new points, adjustment - on a store made from a chain, with the keypoints in the store and
    none passed, against the host-made store of the same matches with `keypoints`, and against the flat backend.  The chain is
    the one of tests/test_gpu_newpoints.py: config 1 with 1500 requested features; images 0-8 are registered with two thirds of
    the points, image 9 is the candidate."""
    sc, st_c, st_h, nf, kp, match_count = chain_stores
    n_reg = sc.n_cams - 1
    c = RD.scene_model(sc, n_reg, nf, sc.feat_point, kp, np.arange(sc.n_points) % 3 != 0, match_count)
    c["book"].update(round_opts=dict(partial_options=dict(max_num_iterations=4)))
    args = (c["state"], c["cam_pose"], c["cam_model"], c["cam_model_of_cam"])
    flat = incremental.FlatBackend(ctx, st_h, *args, keypoints=c["keypoints"])
    chain = incremental.ResidentBackend(ctx, st_c, *args)
    host = incremental.ResidentBackend(ctx, st_h, *args, keypoints=c["keypoints"])
    try:
        assert "no keypoints of image" in refused(incremental.ResidentBackend, ctx, st_h, *args)      # neither the argument nor a chain's
        want = incremental.run_round(flat, incremental.Book(**c["book"]))
        assert want["image"] == n_reg and want["n_new"] > 100 and len(want["visible"]) == n_reg + 1 and want["solved"][0] == 1
        for res in (chain, host):
            same_round(incremental.run_round(res, incremental.Book(**c["book"])), want)
            same(res.fetch(), flat.fetch(), RD.FETCHED)
    finally:
        chain.close(); host.close()


@pytest.fixture(scope="module")
def chain_stores(ctx):
    sc = scene.add_features(scene.config_scene(1), 1500)
    kps = [np.ascontiguousarray(k, np.float32) for k in sc.kp_xy]
    pairs = scene.all_pairs(sc.n_cams)
    ds = ctx.descset(sc.desc, keypoints=kps)
    res = ds.match_pairs(pairs, 0.6, 0.85)
    ch = capi.Chain(res)
    n_m, _, _ = ch.verify(3.0, seed=5)
    st_c = capi.MatchStore.from_chain(ch)
    fetched = [ch.fetch_matches(q) for q in range(len(pairs))]
    moff = np.concatenate([[0], np.cumsum(n_m)]).astype(np.int32)
    ch.close(); res.close(); ds.close()
    nf = np.array([len(k) for k in kps], np.int32)
    st_h = ctx.match_store(nf, pairs, moff, np.concatenate(fetched))
    match_count = np.zeros((sc.n_cams, sc.n_cams), np.int32)
    match_count[pairs[:, 0], pairs[:, 1]] = n_m
    yield sc, st_c, st_h, nf, np.concatenate(kps), match_count
    st_c.close(); st_h.close()


ROUND_KEYS = ("image", "failed_images", "image_ids", "visible", "n_new", "full", "count_outliers", "count_new_add", "count_outliers_new_add")


def backends(ctx, c, **reserve):
    store = ctx.match_store(*c["store"])
    args = (ctx, store, c["state"], c["cam_pose"], c["cam_model"], c["cam_model_of_cam"])
    flat = incremental.FlatBackend(*args, keypoints=c["keypoints"])
    res = incremental.ResidentBackend(*args, keypoints=c["keypoints"], **reserve)
    return store, flat, res, incremental.Book(**c["book"]), incremental.Book(**c["book"])


def same_round(got, want):
    for k in ROUND_KEYS:
        if k in want or k in got:
            assert got[k] == want[k], (k, got[k], want[k])
    if want["image"] < 0:
        return
    for k in ("f", "avg_error", "n_inliers"):
        assert got[k] == want[k], (k, got[k], want[k])
    same(got, want, ("R", "t", "solved"))
    for g, w in zip(got["summary"], want["summary"]):
        assert (g is None) == (w is None)
        if g is not None:
            for k in SUMMARY:
                assert g[k] == w[k], (k, g[k], w[k])
            np.testing.assert_array_equal(g["iterations"], w["iterations"])


def run_both(ctx, c, n_rounds, **reserve):
    """n_rounds through both backends, state and record compared after every round.  Returns the flat records, per round the
    flat backend's winner states and takes flags, the final fetched state and the capacities seen."""
    store, flat, res, book_f, book_r = backends(ctx, c, **reserve)
    try:
        recs, extra, caps = [], [], [res.recon.size()]
        for _ in range(n_rounds):
            want = incremental.run_round(flat, book_f)
            got = incremental.run_round(res, book_r)
            same_round(got, want)
            same(res.fetch(), flat.fetch(), RD.FETCHED)
            np.testing.assert_array_equal(book_r.fail_times, book_f.fail_times)
            recs.append(want)
            caps.append(res.recon.size())
            if want["image"] >= 0:
                r = flat.last_new_points
                extra.append(dict(states=set(np.unique(flat._loc["corr_state"]).tolist()), arm_f=float(book_f.image_f[want["image"]]),
                                  untaken=int((np.asarray(r.takes1) == 0).sum() + (np.asarray(r.takes2) == 0).sum())))
            print({k: want.get(k) for k in ROUND_KEYS}, extra[-1] if want["image"] >= 0 else None)
        return recs, extra, res.fetch(), caps
    finally:
        res.close()
        store.close()


@pytest.fixture(scope="module")
def rounds(ctx):
    return run_both(ctx, RD.rounds_case(), 6)


def test_rounds_match_the_flat_state(rounds):
    """6 rounds of RD.rounds_case() through both backends (the comparison after every round is inside run_both), and the seven
    conditions on the flat backend's own records, so that the comparison cannot pass vacuously."""
    recs, extra, _, _ = rounds
    done = [r for r in recs if r["image"] >= 0]
    assert len(done) >= 5                                                              # 1
    assert any(r["failed_images"] for r in done)                                       # 2: a failed try ahead of a winner
    assert any(e["arm_f"] == 0.0 for e in extra)                                       # 3: a winner on the sweep arm
    assert any({1, 2, 3} <= e["states"] for e in extra)                                # 4
    assert any(e["untaken"] > 0 for e in extra)                                        # 5
    assert any(r["full"] and r["solved"][1] for r in done)                             # 6
    assert any(r["count_outliers"] > 0 for r in done) and any(r["count_outliers"] == 0 for r in done)   # 7


def test_growth_crosses_capacity_in_a_round(ctx, rounds):
    """The same rounds with capacities that a new_points append outgrows, and with room for everything: the final state of the
    first run both times; the capacities change in the one run and not in the other."""
    _, _, final, _ = rounds
    c = RD.rounds_case()
    n, no = len(c["state"]["pt_bad"]), len(c["state"]["obs_point"])
    _, _, tight, caps_t = run_both(ctx, c, 6, reserve_points=n + 10, reserve_obs=no + 250)
    _, _, roomy, caps_r = run_both(ctx, c, 6, reserve_points=20000, reserve_obs=40000)
    same(tight, final, RD.FETCHED)
    same(roomy, final, RD.FETCHED)
    assert len({z["cap_points"] for z in caps_t}) > 1 and len({z["cap_obs"] for z in caps_t}) > 1
    assert {z["cap_points"] for z in caps_r} == {20000} and {z["cap_obs"] for z in caps_r} == {40000}


@pytest.mark.parametrize("n,all_added", [(255, False), (256, False), (257, False), (513, False), (300, True)])
def test_commit_sizes(ctx, n, all_added):
    """A winner row of n correspondences (the block edges of the scan), and one in which no correspondence is state 2 (every
    point is new-added: nothing is appended and the new feat_point row is all -1), against apply_localized_image."""
    c = RD.commit_case(n, all_added)
    store, flat, res, book_f, book_r = backends(ctx, c)
    try:
        cand = np.array([3], np.int32)
        want = flat.localize(book_f, cand)
        got = res.localize(book_r, cand)
        assert want["image"] == 3 == got["image"] and got["n_corr"] == n == len(want["corr_state"])
        pose6 = np.concatenate([scene.R_to_angle_axis(want["R"]).reshape(3), want["t"]])
        assert flat.commit_camera(pose6, 0, None) == res.commit_camera(pose6, 0, None) == [3, 0, 1, 2]
        same(res.fetch(), flat.fetch(), RD.FETCHED)
        n2 = int((want["corr_state"] == 2).sum())
        assert res.recon.size()["n_obs"] == 3 * n + n2 and (n2 == 0) == all_added
        if all_added:      # the pt_bad store of state 1 beside an empty scan
            assert (flat.state["feat_point"][3 * n:] == -1).all() and (want["corr_state"] == 1).any()
        else:
            assert (want["corr_state"] == 1).any() and n2 > n // 4
    finally:
        res.close()
        store.close()


def test_commit_and_localize_refusals_leave_the_state(ctx):
    c = RD.commit_case(64)
    store, flat, res, book_f, book_r = backends(ctx, c)
    try:
        rec = res.recon
        pose6 = np.zeros(6)
        check = lambda: same(rec.fetch(), flat.fetch(), RD.FETCHED)   # noqa: E731
        assert "no pending" in refused(rec.commit_camera, pose6, 0)
        assert "registered already" in refused(rec.localize, [2, 3], [0, 0], [c["book"]["image_f"][0]] * 2)
        check()
        before = rec.size()["h2d_bytes"]
        got = res.localize(book_r, np.array([3], np.int32))
        assert got["image"] == 3 and rec.size()["h2d_bytes"] > before
        assert "model = 2" in refused(rec.commit_camera, pose6, 2)
        assert "cam_model3" in refused(rec.commit_camera, pose6, 1)
        check()
        want = flat.localize(book_f, np.array([3], np.int32))
        pose6 = np.concatenate([scene.R_to_angle_axis(want["R"]).reshape(3), want["t"]])
        assert flat.commit_camera(pose6, 1, [want["f"], 0.0, 0.0]) == res.commit_camera(pose6, 1, [want["f"], 0.0, 0.0])
        check()
        assert "no pending" in refused(rec.commit_camera, pose6, 0)      # a second commit of the same winner
        check()
    finally:
        res.close()
        store.close()


def test_round_traffic_does_not_scale_with_the_state(ctx):
    """A whole round - localize, commit_camera, new_points, adjust - on the rounds case and on the same case with 5 000 more points
    (two rows each on cameras 0 and 1, held by no camera): every call sends the same bytes for both states."""
    K = 5000
    c = RD.rounds_case()
    big = dict(c, state=dict(c["state"]))
    extra = RD.with_unrelated(dict(c["state"], pt_new_added=c["state"]["pt_new_added"]), K)
    for k in ("point_xyz", "pt_bad", "pt_mse", "pt_mutable", "pt_new_added", "obs_point", "obs_cam", "obs_feat"):
        big["state"][k] = extra[k]
    big["state"]["pt_views"] = np.concatenate([c["state"]["pt_views"], np.full(K, 2, np.int32)])
    sent = []
    for case in (c, big):
        store, flat, res, book_f, book_r = backends(ctx, case)
        try:
            rec, steps, before = res.recon, [], res.recon.size()["h2d_bytes"]

            def lap():
                nonlocal before
                now = rec.size()["h2d_bytes"]
                steps.append(now - before)
                before = now
            cam_img = res.cam_img()
            processed = np.zeros(len(book_r.fail_times), bool)
            processed[cam_img] = True
            from metricsfm_amd import localize
            cand = localize.candidate_images(book_r.match_count, processed, book_r.fail_times)
            loc = res.localize(book_r, cand); lap()
            pose6 = np.concatenate([scene.R_to_angle_axis(loc["R"]).reshape(3), loc["t"]])
            visible = res.commit_camera(pose6, 0, None); lap()
            res.new_points(book_r, visible[0], visible); lap()
            res.adjust(book_r, visible[0], visible, False); lap()
            assert steps[0] > 0 and steps[1] == 0 and steps[2] > 0 and steps[3] > 0
            sent.append((loc["image"], steps))
        finally:
            res.close()
            store.close()
    assert sent[0] == sent[1], sent
