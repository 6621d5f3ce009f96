"""The CPU side of msfm_localize_poses (no GPU): the rules of tests/localizepose_ref.py - the yardstick of
tests/test_gpu_localizepose.py - pinned on hand-made error arrays, and the patterns tests/localizepose_data.py records verified
through the oracle."""
import numpy as np

from tests import localizepose_data as PD
from tests.localizepose_ref import localize_poses_ref


def _loc(counts, points):
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    n = int(off[-1])
    return dict(corr_off=off, corr_point=np.asarray(points, np.int32), pts_w=np.zeros((n, 3)), pts_2d=np.zeros((n, 2)))


def _fixed(errors, avgs):
    """Solvers that hand back the given per-row errors and averages."""
    def known(r, X, x, f):
        return np.eye(3) * (r + 1), np.full(3, float(r)), np.asarray(errors[r], float)[:len(X)], avgs[r], 7

    def swept(r, X, x, f_init):
        return 1.5 * f_init, np.eye(3) * (r + 1), np.full(3, float(r)), np.asarray(errors[r], float)[:len(X)], avgs[r], 2, 9
    return known, swept


def test_equal_to_the_average_is_an_inlier_and_nan_goes_on():
    # :713 is `error > avg`: 2.0 at avg 2.0 stays; a NaN error is no outlier; a NaN average passes the gate (:648) and makes
    # no outlier
    loc = _loc([4, 3], [0, 1, 2, 3, 4, 5, 6])
    nan = float("nan")
    r = localize_poses_ref(loc, 100.0, None, 7, None, *_fixed([[2.0, 2.0000001, nan, 1.0], [9.0, 1000.0, 0.0]], [2.0, nan]), th_min_2d3d_corres=0)
    assert list(r["corr_state"]) == [2, 1, 2, 2, 2, 2, 2]
    assert list(r["pass"]) == [1, 1] and r["winner"] == 0
    assert list(r["n_inliers"]) == [3, 3] and list(r["n_outliers"]) == [1, 0]
    # the gate: avg == th passes, the next double above does not
    r = localize_poses_ref(loc, 100.0, None, 7, None, *_fixed([[0.0] * 4, [0.0] * 3], [5.0, np.nextafter(5.0, 6.0)]), th_min_2d3d_corres=0)
    assert list(r["pass"]) == [1, 0] and list(r["corr_state"]) == [2] * 4 + [0] * 3


def test_a_point_named_twice_and_points_added_before():
    # point 3 twice among the inliers: the first takes it, the second finds is_new_added_ set; the outlier in between that names it
    # too marks it bad and does not set the flag; point 5 came in with the flag; each row starts from the input flags again
    loc = _loc([5, 2, 1], [3, 3, 3, 5, 4, 3, 5, 3])
    added = np.zeros(6, np.uint8); added[5] = 1
    r = localize_poses_ref(loc, 100.0, None, 6, added, *_fixed([[9.0, 1.0, 1.0, 1.0, 1.0], [1.0, 1.0], [1.0]], [4.0, 4.0, 4.0]), th_min_2d3d_corres=0)
    assert list(r["corr_state"]) == [1, 2, 3, 3, 2, 0, 0, 0]
    assert list(r["tried"]) == [1, 0, 0]          # 2 and 1 correspondences: below 3 (:567) whatever th_min says
    assert list(r["n_inliers"]) == [2, 0, 0] and list(r["n_outliers"]) == [1, 0, 0]
    assert not added[3]                            # the input is not written
    r = localize_poses_ref(_loc([3, 3], [3, 3, 5, 3, 5, 5]), 100.0, None, 6, added, *_fixed([[1.0] * 3, [1.0] * 3], [4.0, 4.0]), th_min_2d3d_corres=0)
    assert list(r["corr_state"]) == [2, 3, 3, 2, 3, 3]


def test_which_rows_are_tried():
    loc = _loc([25, 19, 20, 2, 30, 21], np.zeros(117, np.int32))
    solvers = _fixed([[9.0] * 30] * 6, [6.0] * 6)
    r = localize_poses_ref(loc, [100.0, 100.0, 0.0, 100.0, 100.0, 0.0], 50.0, 1, None, *solvers)
    assert list(r["tried"]) == [1, 0, 1, 0, 1, 1] and list(r["arm"]) == [1, 0, 2, 0, 1, 2] and r["next_row"] == -1 and r["winner"] == -1
    assert list(r["f"]) == [100.0, 0.0, 75.0, 0.0, 100.0, 75.0] and list(r["best_step"]) == [-1, 0, 2, 0, -1, 2]
    assert not r["R"][1].any() and not r["R"][3].any() and r["avg_error"][1] == 0.0
    r = localize_poses_ref(loc, 100.0, None, 1, None, *solvers, max_tries=2)
    assert list(r["tried"]) == [1, 0, 1, 0, 0, 0] and r["next_row"] == 4 and r["n_tried"] == 2
    r = localize_poses_ref(loc, 100.0, None, 1, None, *solvers, first_row=1, max_tries=2)
    assert list(r["tried"]) == [0, 0, 1, 0, 1, 0] and r["next_row"] == 5
    r = localize_poses_ref(loc, 100.0, None, 1, None, *solvers, first_row=5, max_tries=0)
    assert list(r["tried"]) == [0, 0, 0, 0, 0, 1] and r["next_row"] == -1
    r = localize_poses_ref(loc, 100.0, None, 1, None, *solvers, th_min_2d3d_corres=26, max_tries=1)
    assert list(r["tried"]) == [0, 0, 0, 0, 1, 0] and r["next_row"] == -1      # row 5 has 21
    r = localize_poses_ref(loc, 100.0, None, 1, None, *solvers, th_min_2d3d_corres=0, max_tries=0)
    assert list(r["tried"]) == [1, 1, 1, 0, 1, 1]                              # 2 correspondences: never


def test_recorded_patterns_of_the_ring_round(oracle):
    c, E = PD.ring_case(), PD.EXPECT
    loc = c["loc"]
    assert [int(c["cand_img"][k]) for k in loc["rank"]] == E["images"] and list(np.diff(loc["corr_off"])) == E["n_corr"]
    assert list(c["dup_feats"]) == E["dup_feats"]
    k = PD.reference("known")
    assert list(k["pass"]) == E["known"]["passes"] and k["winner"] == E["known"]["winner"] and k["next_row"] == E["known"]["next_row"]
    assert list(k["n_inliers"]) == E["known"]["n_inliers"] and list(k["n_outliers"]) == E["known"]["n_outliers"]
    assert PD.state_count(k, loc, 3) == E["known"]["state3"] and PD.state_count(k, loc, 2) == E["known"]["n_inliers"]
    assert k["avg_error"][0] > 5.0 and (k["avg_error"][1:] < 5.0).all()
    # a copy of an inlier feature is the second inlier that names its point
    off = loc["corr_off"]
    for r in (1, 2, 3):
        feat, st = loc["corr_feat"][off[r]:off[r + 1]], k["corr_state"][off[r]:off[r + 1]]
        for e, f in enumerate(E["dup_feats"]):
            a, b = int(np.nonzero(feat == f)[0][0]), int(np.nonzero(feat == 200 + e)[0][0])
            assert b > a and (st[a], st[b]) in ((2, 3), (1, 1)), (r, f)
    m = PD.reference("mixed")
    for key, name in (("arm", "arm"), ("pass", "passes"), ("best_step", "best_step"), ("n_inliers", "n_inliers"), ("n_outliers", "n_outliers")):
        assert list(m[key]) == E["mixed"][name], key
    assert m["winner"] == E["mixed"]["winner"]
    na = PD.reference("not_added")
    assert list(na["n_inliers"]) == E["not_added"]["n_inliers"] and PD.state_count(na, loc, 3) == E["not_added"]["state3"]
    np.testing.assert_array_equal(na["errors"], k["errors"])


def test_recorded_patterns_of_the_big_row(oracle):
    c, E = PD.big_case(), PD.EXPECT_BIG
    b = PD.reference("big")
    assert list(np.diff(c["loc"]["corr_off"])) == E["n_corr"] and list(b["pass"]) == E["passes"] and b["winner"] == E["winner"]
    assert list(b["n_inliers"]) == E["n_inliers"] and list(b["n_outliers"]) == E["n_outliers"] and PD.state_count(b, c["loc"], 3) == E["state3"]


def test_committed_answer_still_reproduces(oracle):
    from tests.golden import make_localizepose_golden as G
    g, now = G.load(), G.answers()
    assert sorted(g) == sorted(now)
    for k in now:
        np.testing.assert_array_equal(g[k], now[k], err_msg=k)
