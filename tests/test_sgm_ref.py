"""The two restatements of the dense-stereo definitions (tests/sgm_ref.cpp, tests/sgm_ref.py) against each other, against a planted
disparity, against rows that can be checked by hand, and on every stated quirk.  No device."""
import numpy as np
import pytest

from tests import sgm_data as X
from tests import sgm_ref as R


@pytest.mark.parametrize("name", X.SMALLEST)
def test_restatements_agree(name):
    D = X.CASES[name][0]
    left, right = X.case_pair(name)
    cpp = X.expected(name)
    py = R.run(left, right, D, baseline=X.BASELINE, focal=X.FOCAL, **X.DEFAULTS)
    for plane, _ in X.PLANES:
        assert np.array_equal(cpp[plane], py[plane]), plane


def test_restatements_agree_with_census():
    """The two smallest cases have at most one census row: a case with a census interior, oblique paths of every length and a
    consistency margin as well."""
    left, right = X.case_pair("odd64")
    cpp = X.expected("odd64")
    py = R.run(left, right, 64, baseline=X.BASELINE, focal=X.FOCAL, **X.DEFAULTS)
    for plane, _ in X.PLANES:
        assert np.array_equal(cpp[plane], py[plane]), plane
    assert cpp["census_left"].any() and cpp["disparity"].any() and cpp["depth"].any()


def test_planted_disparity_is_recovered():
    """A noise-free pair, left = right shifted by 9 in the upper and by 23 in the lower half.  Counted: x >= D, more than 8 px from
    the boundary between the halves, inside the consistency grid.  (Pixels inside the median's and the census' border are part
    of the count; 140 x 60 leaves them well below 5 %.)"""
    D, w, h = 64, 140, 60
    left, right, planted = X.planted_pair(w, h, 11, 9, 23)
    got = X.run_ref_cpp(left, right, D, volumes=False)["disparity"]
    yy, xx = np.mgrid[0:h, 0:w]
    counted = (xx >= D) & (np.abs(yy - (h // 2 - 0.5)) > 8) & (xx < 16 * (w // 16)) & (yy < 16 * (h // 16))
    share = (got[counted] == planted[counted]).mean()
    print("planted disparity recovered on %.1f %% of %d pixels" % (100 * share, counted.sum()))
    assert counted.sum() > 1000 and share >= 0.95


def test_constant_image():
    img = np.full((20, 70), 77, np.uint8)
    for got in (X.run_ref_cpp(img, img, 64), R.run(img, img, 64, **X.DEFAULTS)):
        assert not got["census_left"].any() and not got["census_right"].any()
        assert not got["path_cost"].any() and not got["disparity"].any() and not got["raw_right"].any()


def test_single_row_recurrence_by_hand():
    """Path 0 on one row, D = 4, P1 = 2, P2 = 5, with a hand-made C.
      x = 0: L = C                                   = (3, 0, 4, 6)
      x = 1: m = 0; d = 0: min(3, 0 + 2, 5) = 2;  d = 1: min(0, 3 + 2, 4 + 2, 5) = 0;  d = 2: min(4, 0 + 2, 6 + 2, 5) = 2;
             d = 3: min(6, 4 + 2, 5) = 5;  L = C + (2, 0, 2, 5) = (1, 7, 1, 0) + (2, 0, 2, 5) = (3, 7, 3, 5)
      x = 2: m = 3; d = 0: min(0, 4 + 2, 5) = 0;  d = 1: min(4, 0 + 2, 0 + 2, 5) = 2;  d = 2: min(0, 4 + 2, 2 + 2, 5) = 0;
             d = 3: min(2, 0 + 2, 5) = 2;  L = (5, 5, 5, 0) + (0, 2, 0, 2) = (5, 7, 5, 2)
    and path 1 walks the same row from its other end."""
    C = np.array([[[3, 0, 4, 6], [1, 7, 1, 0], [5, 5, 5, 0]]], np.int64)
    L = R.path_cost(C, 0, 2, 5)
    assert L[0].tolist() == [[3, 0, 4, 6], [3, 7, 3, 5], [5, 7, 5, 2]]
    back = R.path_cost(C[:, ::-1], 1, 2, 5)
    assert np.array_equal(back[:, ::-1], L)
    # a vertical path on one row has no predecessor anywhere
    assert np.array_equal(R.path_cost(C, 2, 2, 5), C)


def _winner_rows(S_row, uniqueness=0.96):
    """both restatements' rule on one pixel's sums: the numpy one directly, the C++ one through its shared decision"""
    S = np.asarray(S_row, np.int64)[None, None, :]
    return int(R.winners(S, uniqueness)[0][0, 0])


def test_quirk_ties_go_to_the_lower_disparity():
    S = np.full(64, 50)
    S[[20, 21]] = 7                     # two equal minima side by side: the lower one, not the last one met
    assert _winner_rows(S) == 20
    S = np.full(64, 50)
    S[[20, 40]] = 7                     # equal minima far apart: 7 * 0.96 < 7 and |40 - 20| > 1, so invalid ...
    assert _winner_rows(S) == 0
    assert _winner_rows(S, 1.0) == 20   # ... and at uniqueness 1 the product reaches c0: the lower one


def _check(med_left, med_right, left):
    return R.consistency(np.asarray(med_left, np.uint16), np.asarray(med_right, np.uint16), np.asarray(left, np.uint8))


def test_quirks_of_the_consistency_check():
    h, w = 16, 37                       # grid: x < 32, y < 16
    left = np.full((h, w), 9, np.uint8)
    ml = np.full((h, w), 5, np.uint16)
    mr = np.full((h, w), 5, np.uint16)
    out = _check(ml, mr, left)
    assert (out == 5).all()
    # k = x - d < 0 keeps the pixel (x = 0 .. 4 at d = 5), although no right pixel confirms it
    assert (out[:, :5] == 5).all()
    # a left pixel of value 0 is invalid, whatever the disparities say
    left0 = left.copy()
    left0[3, 10] = 0
    assert _check(ml, mr, left0)[3, 10] == 0 and _check(ml, mr, left0)[3, 11] == 5
    # the right plane disagrees everywhere: inside the grid everything with a partner goes, the margin x >= 32 keeps the
    # median's value, and so does k < 0
    out = _check(ml, np.full((h, w), 9, np.uint16), left)
    assert not out[:, 5:32].any() and (out[:, 32:] == 5).all() and (out[:, :5] == 5).all()
    # rows beyond 16 * (h / 16) as well
    out = _check(np.full((h + 3, w), 5, np.uint16), np.full((h + 3, w), 9, np.uint16), np.full((h + 3, w), 9, np.uint8))
    assert not out[:16, 5:32].any() and (out[16:] == 5).all()
    # a difference of 1 is consistent, d = 0 is not valid
    assert (_check(ml, np.full((h, w), 6, np.uint16), left) == 5).all()
    assert not _check(np.zeros((h, w), np.uint16), np.zeros((h, w), np.uint16), left).any()


def test_quirk_median_border_is_zero():
    p = np.full((6, 7), 9, np.uint16)
    m = R.median3(p)
    assert (m[1:-1, 1:-1] == 9).all()
    assert not m[0].any() and not m[-1].any() and not m[:, 0].any() and not m[:, -1].any()
    # and in the full chain of both restatements, on a case whose raw plane is not zero on the border
    e = X.expected("odd64")
    assert e["raw_left"][0].any() or e["raw_left"][:, -1].any()
    for plane in ("median_left", "median_right"):
        assert not e[plane][0].any() and not e[plane][-1].any() and not e[plane][:, 0].any() and not e[plane][:, -1].any()


def test_quirks_hold_in_the_cpp_restatement():
    """The same quirks through tests/sgm_ref.cpp, on a pair made for them: a constant pair has S = 0 for every d, a tie over all
    disparities, so the raw winners are 0 = the lowest; with the left image 0 in one pixel nothing changes in a constant pair, so the
    zero-pixel and margin rules are read from a textured case instead."""
    img = np.full((20, 70), 77, np.uint8)
    got = X.run_ref_cpp(img, img, 64)
    assert not got["raw_left"].any()
    left, right = X.case_pair("odd64")
    e = X.expected("odd64")
    D, w, h, _ = X.CASES["odd64"]
    zero = left == 0
    gw, gh = 16 * (w // 16), 16 * (h // 16)
    inside = np.zeros((h, w), bool)
    inside[:gh, :gw] = True
    assert zero[inside].any() and not e["disparity"][zero & inside].any()
    assert np.array_equal(e["disparity"][~inside], e["median_left"][~inside].astype(np.uint8)) and e["median_left"][~inside].any()
    # k < 0 keeps: a pixel inside the grid with x < d, a non-zero left value and a positive median keeps the median's value
    xx = np.arange(w)[None, :]
    keeps = inside & (xx - e["median_left"].astype(np.int64) < 0) & ~zero & (e["median_left"] > 0)
    assert keeps.any() and np.array_equal(e["disparity"][keeps], e["median_left"][keeps].astype(np.uint8))
