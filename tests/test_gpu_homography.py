"""msfm_homography_ransac_batch (geo.hip) = cv::findHomography(pts1, pts2, mask, RANSAC, th) of SLAMGPS::FeatureMatching
step 1 (slam_gps.cc:400-408), bit for bit against the sequential CPU restatement tests/hransac_ref.cpp: H, mask, counts, ok."""
import os

import numpy as np
import pytest

from metricsfm_amd import _abi as A
from metricsfm_amd import capi
from tests import hransac_data as D

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hransac_small.npz")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return D.build_ref(tmp_path_factory.mktemp("hransac_ref"))


def _mixed_batch(seed, frac, planar):
    rng = np.random.default_rng(seed)
    parts = []
    for n in (0, 3, 4, 5, 60, 400, 1500, 2500):   # the last two exceed one 1 024-point LDS tile of the scoring kernel
        x1, x2, _, _ = D.make_pair(rng, n, frac if n > 4 else 0.0, planar=planar, noise=0.5)
        parts.append((x1, x2))
    return D.batch(parts)


def _same(g, r):
    for a, b in zip(g, r):
        np.testing.assert_array_equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("frac", [0.0, 0.3, 0.6, 0.85])
@pytest.mark.parametrize("planar", [True, False])
def test_matches_cpu_restatement(ctx, ref, frac, planar):
    off, p1, p2 = _mixed_batch(int(frac * 100) + (0 if planar else 7), frac, planar)
    for polish in (0, 1):
        for seed in (D.SEED_H, 12345):
            g = ctx.homography_ransac(off, p1, p2, threshold=3.0, polish=polish, seed=seed)
            r = D.ref_hransac(ref, off, p1, p2, threshold=3.0, polish=polish, seed=seed)
            _same(g, r)
            H, inl, nin, ok = g
            assert ok[:2].tolist() == [0, 0] and nin[:2].tolist() == [0, 0]
            assert ok[2] == 1 and nin[2] == 4
            if planar and frac <= 0.6:
                assert ok[4:].all()
            if polish == 0:
                # the mask is the binary32 error of the returned H against threshold^2
                for p in range(len(off) - 1):
                    if not ok[p] or off[p + 1] - off[p] <= 4:
                        continue
                    s = slice(off[p], off[p + 1])
                    e = D.transfer_err32(H[p], p1[s], p2[s])
                    np.testing.assert_array_equal(inl[s], (e.astype(np.float64) <= 9.0).astype(np.uint8))


@pytest.mark.gpu
def test_all_samples_replayed_at_85_percent_outliers(ctx, ref):
    """At 85 % outliers cvRANSACUpdateNumIters never cuts the 2 000 samples: the second pass runs for these pairs."""
    rng = np.random.default_rng(85)
    parts = [D.make_pair(rng, 1200, 0.85, planar=True, noise=0.3)[:2] for _ in range(3)]
    off, p1, p2 = D.batch(parts)
    assert D.ref_hransac(ref, [0, 1200], p1[:1200], p2[:1200])[3][0] == 1
    _same(ctx.homography_ransac(off, p1, p2), D.ref_hransac(ref, off, p1, p2))
    assert ref.hr_update_num_iters(0.995, 0.86, 4, 2000) == 2000


@pytest.mark.gpu
def test_pair_result_does_not_depend_on_neighbours(ctx):
    off, p1, p2 = _mixed_batch(3, 0.3, True)
    full = ctx.homography_ransac(off, p1, p2)
    # pair 5 alone, but at sampler index 5 (the sampler index is the position in the call): pad with empty pairs
    s = slice(off[5], off[6])
    off5 = np.array([0, 0, 0, 0, 0, 0, off[6] - off[5]], np.int32)
    alone = ctx.homography_ransac(off5, p1[s], p2[s])
    np.testing.assert_array_equal(alone[0][5], full[0][5])
    np.testing.assert_array_equal(alone[1], full[1][s])
    assert alone[2][5] == full[2][5] and alone[3][5] == full[3][5]
    # and its neighbours changed: another pair at index 4 does not move pair 5
    off_b = off.copy()
    p1b, p2b = p1.copy(), p2.copy()
    p2b[off[4]:off[5]] += 13.0
    other = ctx.homography_ransac(off_b, p1b, p2b)
    np.testing.assert_array_equal(other[0][5], full[0][5])
    np.testing.assert_array_equal(other[1][s], full[1][s])


@pytest.mark.gpu
def test_degenerate_and_small_sets(ctx, ref):
    t = np.linspace(-300, 300, 40)
    col1, col2 = np.column_stack([t, 0.5 * t + 3]), np.column_stack([2 * t, -t + 7])
    same1, same2 = np.tile([[12.5, -3.25]], (30, 1)), np.tile([[7.0, 1.0]], (30, 1))
    off, p1, p2 = D.batch([(col1, col2), (same1, same2), (col1[:4], col2[:4]), (col1[:2], col2[:2])])
    g = ctx.homography_ransac(off, p1, p2)
    _same(g, D.ref_hransac(ref, off, p1, p2))
    H, inl, nin, ok = g
    assert ok.tolist() == [0, 0, 0, 0] and (H == 0).all()
    assert nin.tolist() == [40, 30, 4, 0]
    assert (inl[:74] == 1).all() and (inl[74:] == 0).all()


@pytest.mark.gpu
def test_bad_options_are_refused(ctx):
    off, p1, p2 = _mixed_batch(1, 0.3, True)
    for kw in ({"max_iterations": 0}, {"confidence": 0.0}, {"confidence": 1.0}, {"confidence": -0.5}):
        with pytest.raises(capi.MsfmError) as e:
            ctx.homography_ransac(off, p1, p2, **kw)
        assert e.value.code == A.MSFM_E_INVAL
    bad = off.copy()
    bad[3], bad[4] = bad[4], bad[3]
    with pytest.raises(capi.MsfmError) as e:
        ctx.homography_ransac(bad, p1, p2)
    assert e.value.code == A.MSFM_E_INVAL
    with pytest.raises(capi.MsfmError) as e:
        ctx.homography_ransac(off + 1, p1, p2)
    assert e.value.code == A.MSFM_E_INVAL
    # threshold <= 0 means 3.0, as in OpenCV
    _same(ctx.homography_ransac(off, p1, p2, threshold=0.0), ctx.homography_ransac(off, p1, p2, threshold=3.0))


@pytest.mark.gpu
def test_golden_fixture(ctx):
    """tests/golden/hransac_small.npz (tests/golden/make_hransac_golden.py: the CPU restatement's output) without a compiler."""
    z = np.load(GOLDEN)
    for polish in (0, 1):
        H, inl, nin, ok = ctx.homography_ransac(z["off"], z["pt1"], z["pt2"], threshold=float(z["threshold"]), polish=polish,
                                                seed=int(z["seed"]))
        np.testing.assert_array_equal(H, z["H%d" % polish])
        np.testing.assert_array_equal(inl, z["inlier%d" % polish])
        np.testing.assert_array_equal(nin, z["n_inliers%d" % polish])
        np.testing.assert_array_equal(ok, z["ok%d" % polish])
