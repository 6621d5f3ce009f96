"""The CPU restatement of cv::findHomography(RANSAC) (tests/hransac_ref.cpp) that the GPU homography RANSAC is compared
with bit for bit, checked on its own against the geometry, and the feature/prior.txt format of SLAMGPS step 1
(slam_gps.cc:1821-1885).  No GPU."""
import numpy as np
import pytest

from metricsfm_amd import matchfiles
from tests import hransac_data as D


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return D.build_ref(tmp_path_factory.mktemp("hransac_ref"))


def test_exact_H_from_four_points(ref):
    rng = np.random.default_rng(5)
    Ht = D.random_H(rng)
    x1 = np.array([[-400, -300], [420, -280], [380, 310], [-350, 290]], np.float64)
    x2 = D.apply_H(Ht, x1)
    H, inl, nin, ok = D.ref_hransac(ref, [0, 4], x1, x2)
    assert ok[0] == 1 and nin[0] == 4 and inl.tolist() == [1, 1, 1, 1] and H[0, 2, 2] == 1.0
    # the points are rounded to binary32 first: the fit is exact for the rounded points
    np.testing.assert_allclose(D.apply_H(H[0], x1.astype(np.float32)), x2.astype(np.float32), rtol=0, atol=1e-9 * 1e3)


def test_planar_truth_to_1e9(ref):
    """Noise-free planar data with 30 % outliers, points and their images exactly representable: H to 1e-9 of the truth,
    the mask = the true inliers, with and without the polish."""
    Ht = np.array([[1.25, 0.0, 16.0], [0.0, 0.75, -8.0], [0.0, 0.0, 1.0]])
    g = np.array([(x, y) for x in range(-512, 513, 64) for y in range(-384, 385, 64)], np.float64)
    rng = np.random.default_rng(2)
    x1, x2 = g.copy(), D.apply_H(Ht, g)
    n_out = int(0.3 * len(g))
    idx = rng.choice(len(g), n_out, replace=False)
    x2[idx] += rng.uniform(50, 200, (n_out, 2)) * rng.choice([-1, 1], (n_out, 2))
    good = np.ones(len(g), bool)
    good[idx] = False
    for polish in (0, 1):
        H, inl, nin, ok = D.ref_hransac(ref, [0, len(g)], x1, x2, polish=polish)
        assert ok[0] == 1
        np.testing.assert_array_equal(inl.astype(bool), good)
        assert nin[0] == good.sum()
        assert np.abs(H[0] - Ht).max() <= 1e-9, (polish, H[0] - Ht)


def test_planar_with_perspective_and_outliers(ref):
    rng = np.random.default_rng(11)
    x1, x2, Ht, good = D.make_pair(rng, 500, 0.3, planar=True, noise=0.0)
    for polish in (0, 1):
        H, inl, nin, ok = D.ref_hransac(ref, [0, 500], x1, x2, polish=polish)
        assert ok[0] == 1
        np.testing.assert_array_equal(inl.astype(bool), good)
        d = D.apply_H(H[0], x1[good].astype(np.float64)) - D.apply_H(Ht, x1[good].astype(np.float64))
        assert np.abs(d).max() < 1e-3   # binary32 rounding of the inputs is all that is left


@pytest.mark.parametrize("kind", ["collinear", "identical"])
def test_degenerate_sets_fail_with_mask_of_ones(ref, kind):
    n = 40
    if kind == "collinear":
        t = np.linspace(-300, 300, n)
        x1 = np.column_stack([t, 0.5 * t + 3])
        x2 = np.column_stack([2 * t, -t + 7])
    else:
        x1 = np.tile([[12.5, -3.25]], (n, 1))
        x2 = np.tile([[7.0, 1.0]], (n, 1))
    H, inl, nin, ok = D.ref_hransac(ref, [0, n], x1, x2)
    assert ok[0] == 0 and (H[0] == 0).all()
    assert (inl == 1).all() and nin[0] == n


def test_small_sets(ref):
    rng = np.random.default_rng(3)
    Ht = D.random_H(rng)
    x1 = rng.uniform(-500, 500, (4, 2))
    x2 = D.apply_H(Ht, x1)
    off, p1, p2 = D.batch([(x1[:0], x2[:0]), (x1[:3], x2[:3]), (x1, x2)])
    H, inl, nin, ok = D.ref_hransac(ref, off, p1, p2)
    assert ok.tolist() == [0, 0, 1] and nin.tolist() == [0, 0, 4]
    assert inl.tolist() == [0, 0, 0, 1, 1, 1, 1]
    assert (H[:2] == 0).all() and H[2, 2, 2] == 1.0
    np.testing.assert_allclose(H[2], Ht, rtol=1e-4, atol=1e-7)


def test_polish_never_increases_the_inlier_error(ref):
    rng = np.random.default_rng(17)
    for trial in range(6):
        x1, x2, _, _ = D.make_pair(rng, 300, 0.25, planar=trial % 2 == 0, noise=1.0)
        H0, inl0, n0, ok0 = D.ref_hransac(ref, [0, 300], x1, x2, polish=0, threshold=5.0)
        H1, inl1, n1, ok1 = D.ref_hransac(ref, [0, 300], x1, x2, polish=1, threshold=5.0)
        assert ok0[0] == ok1[0] == 1
        np.testing.assert_array_equal(inl0, inl1)   # the mask is the RANSAC mask, not recomputed after the polish
        m = inl0.astype(bool)
        e0 = ((D.apply_H(H0[0], x1[m].astype(np.float64)) - x2[m]) ** 2).sum()
        e1 = ((D.apply_H(H1[0], x1[m].astype(np.float64)) - x2[m]) ** 2).sum()
        assert e1 <= e0 * (1 + 1e-12), (trial, e0, e1)


def test_update_num_iters_with_four_model_points(ref):
    assert ref.hr_update_num_iters(0.995, 0.5, 4, 2000) == round(np.log(0.005) / np.log(1 - 0.5 ** 4))
    assert ref.hr_update_num_iters(0.995, 0.85, 4, 2000) == 2000


def test_prior_file_round_trip(tmp_path):
    rng = np.random.default_rng(4)
    pairs = np.array([(0, 1), (0, 3), (2, 0), (2, 1), (4, 3)], np.int32)
    F = rng.normal(0, 1e-3, (5, 3, 3))
    H = rng.normal(0, 1, (5, 3, 3))
    F[:, 2, 2] = 1.0
    H[:, 2, 2] = 1.0
    p = tmp_path / "prior.txt"
    matchfiles.write_prior_info(str(p), 5, pairs, F, H)
    n, pr, F2, H2 = matchfiles.read_prior_info(str(p))
    assert n == 5
    np.testing.assert_array_equal(pr, pairs)
    np.testing.assert_allclose(F2, F, rtol=0, atol=5e-13)
    np.testing.assert_allclose(H2, H, rtol=0, atol=5e-13)
    lines = p.read_text().split("\n")
    assert lines[0] == "5" and lines[1] == "2" and lines[2].startswith("1 ") and lines[2].endswith(" ")
    assert len(lines[2].split()) == 19 and "%.12f" % F[0, 0, 0] == lines[2].split()[1] and "%.12f" % H[0, 0, 0] == lines[2].split()[2]
    assert lines[4] == "0"   # camera 1 keeps no pair
    matchfiles.write_prior_info(str(tmp_path / "again.txt"), 5, pr, F2, H2)
    assert (tmp_path / "again.txt").read_text() == p.read_text()


def test_reads_a_reference_style_file(tmp_path):
    """A file as SLAMGPS::WriteOutPriorInfo writes it (std::fixed, setprecision(12), `id F00 H00 F01 H01 ... `)."""
    txt = ("3\n"
           "1\n"
           "2 0.000000000001 1.000000000000 -0.000012345678 0.000000000000 0.500000000000 12.250000000000 "
           "0.000000000000 0.000000000000 1.000000000000 1.000000000000 -3.000000000000 -7.125000000000 "
           "0.000000000000 0.000000000000 0.000000000000 0.000000000000 1.000000000000 1.000000000000 \n"
           "0\n"
           "0\n")
    p = tmp_path / "prior.txt"
    p.write_text(txt)
    n, pr, F, H = matchfiles.read_prior_info(str(p))
    assert n == 3 and pr.tolist() == [[0, 2]]
    np.testing.assert_array_equal(F[0], [[1e-12, -0.000012345678, 0.5], [0, 1, -3], [0, 0, 1]])
    np.testing.assert_array_equal(H[0], [[1, 0, 12.25], [0, 1, -7.125], [0, 0, 1]])
    matchfiles.write_prior_info(str(tmp_path / "w.txt"), n, pr, F, H)
    assert (tmp_path / "w.txt").read_text() == txt
