"""msfm_localize_poses (the try loop of sfm_incremental.cc:143-164 around IncrementalSfM::LocalizeImage, :565-729) on the resident
correspondence set, against the two public pose calls on the fetched set, against the sequential restatement of
tests/localizepose_ref.py over the oracle, and against the patterns tests/localizepose_data.py records.  The pose kernels are
the ones behind `ctx.epnp_ransac` / `ctx.epnpf_sweep` and the rest is integer work, so every array must be identical."""
import numpy as np
import pytest

from metricsfm_amd import _abi as A
from metricsfm_amd import capi
from tests import localize_data as D
from tests import localizepose_data as PD
from tests import localizepose_ref as PR
from tests.golden import make_localizepose_golden as G

pytestmark = pytest.mark.gpu


def _same(got, want, keys=PD.ROW_ARRAYS + PD.CORR_ARRAYS + PD.SCALARS):
    for k in keys:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def _set(ctx, c, cand=None):
    st = ctx.match_store(*D.store_args(c))
    cam_img, fp, bad, mse, views, cand_img, fail = D.problem_args(c)
    if cand is not None:
        cand_img, fail = cand_img[cand], fail[cand]
    s = ctx.localize_set(st, cam_img, fp, bad, mse, views, cand_img, fail, point_xyz=c["point_xyz"], keypoints=c["keypoints"])
    st.close()                                   # the set keeps what it needs
    return s


@pytest.fixture(scope="module")
def ring(ctx):
    c = PD.ring_case()
    s = _set(ctx, c)
    loc = s.fetch()
    for k in D.ARRAYS + ("pts_w", "pts_2d"):      # the search itself: tests/test_gpu_localize.py; here only that the case is the case
        np.testing.assert_array_equal(loc[k], c["loc"][k], err_msg=k)
    yield c, s, loc
    s.close()


def test_known_focal_rows_equal_epnp_ransac_and_the_restatement(ctx, ring, oracle):
    c, s, loc = ring
    got = s.poses(c["f"], pt_new_added=c["pt_new_added"])
    R, t, err, avg, best = ctx.epnp_ransac(loc["corr_off"], loc["pts_w"], loc["pts_2d"], c["f"])
    for name, want in (("R", R), ("t", t), ("errors", err), ("avg_error", avg), ("best_iter", best)):
        np.testing.assert_array_equal(got[name], want, err_msg=name)
    _same(got, PD.reference("known"))
    E = PD.EXPECT["known"]
    assert list(got["tried"]) == [1, 1, 1, 1] and list(got["arm"]) == [1, 1, 1, 1] and list(got["pass"]) == E["passes"]
    assert got["winner"] == E["winner"] and got["next_row"] == E["next_row"] and got["n_tried"] == 4
    assert list(got["n_inliers"]) == E["n_inliers"] and list(got["n_outliers"]) == E["n_outliers"]
    assert PD.state_count(got, loc, 3) == E["state3"] and min(E["state3"][1:]) > 0          # state 3 occurs
    assert PD.state_count(got, loc, 0) == [203, 0, 0, 0]                                    # the failed row has no states


def test_sweep_rows_equal_epnpf_sweep(ctx, ring):
    c, s, loc = ring
    got = s.poses(0.0, row_f_init=c["f"], pt_new_added=c["pt_new_added"], sweep=PD.SWEEP)
    f, R, t, err, avg, bstep, biter = ctx.epnpf_sweep(loc["corr_off"], loc["pts_w"], loc["pts_2d"], c["f"], **PD.SWEEP)
    for name, want in (("f", f), ("R", R), ("t", t), ("errors", err), ("avg_error", avg), ("best_step", bstep), ("best_iter", biter)):
        np.testing.assert_array_equal(got[name], want, err_msg=name)
    assert list(got["arm"]) == [2, 2, 2, 2] and list(got["pass"]) == list((~(avg > 5.0)).astype(np.uint8))


def test_a_mixed_call_equals_both_and_the_restatement(ctx, ring, oracle):
    c, s, loc = ring
    row_f = PD.ROW_F["mixed"](c)
    got = s.poses(row_f, row_f_init=c["f"], pt_new_added=c["pt_new_added"], sweep=PD.SWEEP)
    k = ctx.epnp_ransac(loc["corr_off"], loc["pts_w"], loc["pts_2d"], c["f"])
    w = ctx.epnpf_sweep(loc["corr_off"], loc["pts_w"], loc["pts_2d"], c["f"], **PD.SWEEP)
    off = loc["corr_off"]
    for r in range(4):
        R, t, err, avg, bi = (w[1], w[2], w[3], w[4], w[6]) if row_f[r] == 0 else k
        np.testing.assert_array_equal(got["R"][r], R[r]); np.testing.assert_array_equal(got["t"][r], t[r])
        np.testing.assert_array_equal(got["errors"][off[r]:off[r + 1]], err[off[r]:off[r + 1]])
        assert got["avg_error"][r] == avg[r] and got["best_iter"][r] == bi[r]
        assert got["f"][r] == (w[0][r] if row_f[r] == 0 else c["f"]) and got["best_step"][r] == (w[5][r] if row_f[r] == 0 else -1)
    _same(got, PD.reference("mixed"))
    E = PD.EXPECT["mixed"]
    assert list(got["arm"]) == E["arm"] and list(got["pass"]) == E["passes"] and got["winner"] == E["winner"]
    assert list(got["best_step"]) == E["best_step"] and list(got["n_inliers"]) == E["n_inliers"] and list(got["n_outliers"]) == E["n_outliers"]


def test_thresholds(ctx, ring):
    c, s, loc = ring
    full = s.poses(c["f"], pt_new_added=c["pt_new_added"])
    low = s.poses(c["f"], pt_new_added=c["pt_new_added"], th_mse_localization=1.0)      # below every average (1.12 .. 6.77)
    assert low["winner"] == -1 and not low["pass"].any() and not low["corr_state"].any() and not low["n_inliers"].any()
    _same(low, full, ("tried", "R", "t", "errors", "avg_error", "best_iter"))
    # 203 correspondences per row: 204 leaves every row untried, and all zeros come back
    none = s.poses(c["f"], n_points=200, th_min_2d3d_corres=204)
    assert none["n_tried"] == 0 and none["winner"] == -1 and none["next_row"] == -1
    assert not any(np.asarray(none[k]).any() for k in PD.ROW_ARRAYS + PD.CORR_ARRAYS)


def test_a_row_below_th_min_is_left_untried(ctx):
    # images 8 and 9 only, image 9 with the first 150 matches of pair (9, 0) alone: rows of 203 and 150 correspondences
    c = dict(PD.ring_case())
    keep = [p for p, (i, j) in enumerate(c["pairs"]) if not (i == 9 and j != 0)]
    lens = np.diff(c["match_off"])
    lens[[p for p in keep if tuple(c["pairs"][p]) == (9, 0)]] = 150
    c["matches"] = np.concatenate([c["matches"][c["match_off"][p]:c["match_off"][p] + lens[p]] for p in keep])
    c["pairs"], c["match_off"] = c["pairs"][keep], np.concatenate([[0], np.cumsum(lens[keep])]).astype(np.int32)
    s = _set(ctx, c, cand=[2, 3])
    loc = s.fetch()
    n = np.diff(loc["corr_off"])
    assert list(loc["rank"]) == [0, 1] and list(n) == [203, 150]
    got = s.poses(c["f"], n_points=200, th_min_2d3d_corres=int(n[1]) + 1)
    assert list(got["tried"]) == [1, 0] and got["next_row"] == -1 and not got["R"][1].any() and got["avg_error"][1] == 0.0
    assert not got["errors"][loc["corr_off"][1]:].any()
    got = s.poses(c["f"], n_points=200, th_min_2d3d_corres=int(n[1]))
    assert list(got["tried"]) == [1, 1] and got["avg_error"][1] > 0.0
    s.close()


def test_chunks_of_one_try_reproduce_the_single_call(ctx, ring):
    c, s, loc = ring
    row_f = PD.ROW_F["mixed"](c)
    full = s.poses(row_f, row_f_init=c["f"], pt_new_added=c["pt_new_added"], sweep=PD.SWEEP)
    off, row, seen = loc["corr_off"], 0, []
    while row >= 0:
        one = s.poses(row_f, row_f_init=c["f"], pt_new_added=c["pt_new_added"], sweep=PD.SWEEP, first_row=row, max_tries=1)
        assert one["n_tried"] == 1 and list(np.nonzero(one["tried"])[0]) == [row]
        assert one["winner"] == (row if full["pass"][row] else -1)
        for k in PD.ROW_ARRAYS:
            np.testing.assert_array_equal(one[k][row], full[k][row], err_msg=k)
            assert not np.delete(one[k], row, axis=0).any(), k                     # untried rows return zeros
        for k in PD.CORR_ARRAYS:
            np.testing.assert_array_equal(one[k][off[row]:off[row + 1]], full[k][off[row]:off[row + 1]], err_msg=k)
        seen.append(row)
        row = one["next_row"]
    assert seen == [0, 1, 2, 3]
    two = s.poses(row_f, row_f_init=c["f"], n_points=200, sweep=PD.SWEEP, first_row=1, max_tries=2)
    assert list(two["tried"]) == [0, 1, 1, 0] and two["next_row"] == 3 and two["winner"] == 2


def test_a_row_alone_in_the_search_keeps_its_rules_not_its_samples(ctx, ring, oracle):
    """Image 8 searched alone is row 0 instead of row 1.  Its correspondences are the same (tests/test_gpu_localize.py), but the
    row index is the sampler index, so other samples are drawn and pose, errors and with them the states may differ from row 1 of
    the full call.  What holds: it is problem 0 of `ctx.epnp_ransac` on its own set, and the states follow from that pose by the
    same rules - the restatement at row 0."""
    c, s, loc = ring
    one = _set(ctx, c, cand=[2])
    l1 = one.fetch()
    off = loc["corr_off"]
    np.testing.assert_array_equal(l1["corr_point"], loc["corr_point"][off[1]:off[2]])
    np.testing.assert_array_equal(l1["pts_2d"], loc["pts_2d"][off[1]:off[2]])
    got = one.poses(c["f"], pt_new_added=c["pt_new_added"])
    one.close()
    R, t, err, avg, best = ctx.epnp_ransac(l1["corr_off"], l1["pts_w"], l1["pts_2d"], c["f"])
    np.testing.assert_array_equal(got["R"], R); np.testing.assert_array_equal(got["errors"], err)
    known, swept = PR.oracle_solvers(oracle)
    _same(got, PR.localize_poses_ref(l1, c["f"], None, 200, c["pt_new_added"], known, swept))


def test_pt_new_added_null_is_all_zeros(ctx, ring, oracle):
    c, s, loc = ring
    a = s.poses(c["f"], n_points=200)
    b = s.poses(c["f"], pt_new_added=np.zeros(200, np.uint8))
    _same(a, b)
    _same(a, PD.reference("not_added"))
    assert list(a["n_inliers"]) == PD.EXPECT["not_added"]["n_inliers"] and PD.state_count(a, loc, 3) == PD.EXPECT["not_added"]["state3"]


def test_a_row_spans_several_workgroups(ctx, oracle):
    c, E = PD.big_case(), PD.EXPECT_BIG
    s = _set(ctx, c)
    loc = s.fetch()
    assert list(np.diff(loc["corr_off"])) == E["n_corr"]
    got = s.poses(c["f"], pt_new_added=c["pt_new_added"])
    s.close()
    _same(got, PD.reference("big"))
    assert list(got["pass"]) == E["passes"] and got["winner"] == E["winner"] and list(got["n_inliers"]) == E["n_inliers"]
    assert list(got["n_outliers"]) == E["n_outliers"] and PD.state_count(got, loc, 3) == E["state3"]


def test_degenerate_and_refused_input(ctx, ring):
    c, s, loc = ring
    st = ctx.match_store(*D.store_args(c))
    cam_img, fp, bad, mse, views, cand_img, fail = D.problem_args(c)
    empty = ctx.localize_set(st, cam_img, fp, bad, mse, views, cand_img[:0], fail[:0], point_xyz=c["point_xyz"], keypoints=c["keypoints"])
    got = empty.poses([], n_points=200)
    assert got["n_tried"] == 0 and got["winner"] == -1 and got["next_row"] == -1 and len(got["tried"]) == 0 and len(got["errors"]) == 0
    empty.close()
    bare = ctx.localize_set(st, cam_img, fp, bad, mse, views, cand_img, fail)
    st.close()

    def refused(fn, *words):
        with pytest.raises(capi.MsfmError) as e:
            fn()
        assert e.value.code == A.MSFM_E_INVAL
        assert all(w in str(e.value) for w in words), str(e.value)

    refused(lambda: bare.poses(c["f"], n_points=200), "point_xyz")
    bare.close()
    top = int(loc["corr_point"].max())
    refused(lambda: s.poses(c["f"], n_points=top), "n_points", "point %d" % top)
    refused(lambda: s.poses(c["f"], n_points=200, first_row=-1), "first_row")
    refused(lambda: s.poses(c["f"], n_points=200, max_tries=-1), "max_tries")
    refused(lambda: s.poses(c["f"], n_points=200, max_iter=0), "max_iter")
    refused(lambda: s.poses(c["f"], n_points=200, max_iter=65537), "max_iter")
    refused(lambda: s.poses(c["f"], n_points=200, sweep=dict(f_ratio_step=0.0)), "f_ratio_step")
    refused(lambda: s.poses(c["f"], n_points=200, sweep=dict(f_ratio_max=0.5)), "f_ratio_max")
    refused(lambda: s.poses(c["f"], n_points=200, sweep=dict(max_iter=0)), "max_iter")
    refused(lambda: s.poses(c["f"], n_points=200, sweep=dict(f_ratio_step=1e-9)), "step count")
    refused(lambda: s.poses(-1.0, n_points=200), "row_f")
    refused(lambda: s.poses(0.0, n_points=200), "row_f_init")
    _same(s.poses(c["f"], n_points=top + 1), s.poses(c["f"], n_points=200))          # the context stays usable; spare points change nothing


def test_a_set_keeps_its_context(oracle):
    """A set is a child of its context: closing the context first keeps it until the set has gone."""
    c = PD.ring_case()
    own = capi.Context(0)
    s = _set(own, c)
    own.close()
    got = s.fetch()
    np.testing.assert_array_equal(got["corr_point"], c["loc"]["corr_point"])
    s.close()                                     # last child: the context is released here


def test_committed_answer(ctx, ring):
    c, s, loc = ring
    g = G.load()
    got = s.poses(PD.ROW_F["mixed"](c), row_f_init=c["f"], pt_new_added=c["pt_new_added"], sweep=PD.SWEEP)
    for k in PD.ROW_ARRAYS + PD.CORR_ARRAYS:
        np.testing.assert_array_equal(got[k], g["mixed_" + k], err_msg=k)
    assert [got[k] for k in PD.SCALARS] == list(g["mixed_scalars"])
    got = s.poses(c["f"], pt_new_added=c["pt_new_added"])
    for k in PD.ROW_ARRAYS + PD.CORR_ARRAYS:
        np.testing.assert_array_equal(got[k], g["known_" + k], err_msg=k)
    assert [got[k] for k in PD.SCALARS] == list(g["known_scalars"])
