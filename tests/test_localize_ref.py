"""tests/localize_ref.py - the dict walk the GPU search is compared with - against expectations written out by hand: one case
of a few matches per quirk of IncrementalSfM::FindImageToLocalize (sfm_incremental.cc:440-562), and `candidate_images`
(:423-438)."""
import numpy as np
import pytest

from metricsfm_amd.localize import candidate_images
from tests import localize_data as D
from tests.localize_ref import localize_ref


@pytest.mark.parametrize("name", sorted(D.QUIRKS))
def test_quirk(name):
    c = D.QUIRKS[name]
    got = localize_ref(*D.store_args(c), *D.problem_args(c))
    for k in D.ARRAYS:
        np.testing.assert_array_equal(got[k], c["expect"][k], err_msg=k)


def test_points_and_keypoints_follow_the_sorted_order():
    c = D.QUIRKS["two_views_add_three"]
    xyz = np.arange(3 * D.N_POINTS, dtype=np.float64).reshape(-1, 3)
    kp = np.arange(2 * sum(D.N_FEATURES), dtype=np.float32).reshape(-1, 2) * 0.5
    got = localize_ref(*D.store_args(c), *D.problem_args(c), point_xyz=xyz, keypoints=kp)
    np.testing.assert_array_equal(got["pts_w"], xyz[[1, 2, 3, 4, 5, 0]])
    first = sum(D.N_FEATURES[:2])                       # image 2's keypoints start behind those of images 0 and 1
    np.testing.assert_array_equal(got["pts_2d"], kp[first + np.array([1, 2, 3, 4, 5, 0])].astype(np.float64))


def test_ring_round_has_what_the_gpu_test_relies_on():
    """Repeated features, features without a point, bad points, ties in the sort key and a tie in the score all occur."""
    c = D.ring_round()
    r = localize_ref(*D.store_args(c), *D.problem_args(c))
    assert len(r["rank"]) == 4 and (np.diff(r["corr_off"]) > 100).all() and (np.diff(r["vis_off"]) == 6).all()
    i = int(c["cand_img"][r["rank"][0]])
    row = np.nonzero(c["pairs"][:, 0] == i)[0][0]
    f_i = c["matches"][c["match_off"][row]:c["match_off"][row + 1], 0]
    assert len(np.unique(f_i)) == len(f_i)             # (a wrong match replaces the second feature: the first stays unique per pair ...)
    f_all = c["matches"][c["match_off"][row]:c["match_off"][row + 6], 0]
    assert len(np.unique(f_all)) < len(f_all)          # (... and repeats across the pairs of the candidate)
    mse = c["pt_mse"][r["corr_point"]] + 3.0 * (c["pt_views"][r["corr_point"]] <= 2)
    seg = mse[r["corr_off"][0]:r["corr_off"][1]]
    assert (np.diff(seg) >= 0).all() and (np.diff(seg) == 0).sum() >= 5
    assert (c["feat_point"] < 0).mean() > 0.05 and c["pt_bad"].sum() >= 5 and not c["pt_bad"][r["corr_point"]].any()


def test_candidate_images_reads_the_registered_rows():
    n = 5
    mc = np.zeros((n, n), np.int32)
    mc[0, 2] = 7          # registered 0 -> 2: candidate
    mc[3, 1] = 9          # 3 -> registered 1 only in the other direction: not a candidate (:428 reads row id_img of the camera)
    mc[1, 4] = 4          # 4 has failed too often
    mc[1, 0] = 5          # registered already
    processed = np.array([1, 1, 0, 0, 0], bool)
    fail = np.array([0, 0, 4, 0, 5])
    np.testing.assert_array_equal(candidate_images(mc, processed, fail, 5), [2])
    np.testing.assert_array_equal(candidate_images(mc, processed, fail, 6), [2, 4])
    np.testing.assert_array_equal(candidate_images(mc, np.zeros(n, bool), fail, 5), [])
