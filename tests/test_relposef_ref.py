"""The CPU restatement of RelativePoseEstimation::RelativePoseWithoutFocalLength (tests/relposef_ref.cpp) that
msfm_relpose_8pt_batch is compared with bit for bit, checked on its own: the single-sample eight-point fit against a
numpy restatement, noise-free generic pairs against the truth, the algebraic epipole rotation against the atan2 form,
the pose-from-E tail against the five-point oracle, the reference's quirks, and the committed fixture.  No GPU."""
import os

import numpy as np
import pytest

from tests import relposef_data as D
from tests.twoview import make_relpose_batch

GOLD = os.path.join(os.path.dirname(__file__), "golden", "relposef_golden.npz")
NAMES = ("F", "f_ref", "f_cur", "E", "R", "t", "ok", "best_iter", "best_error", "n_candidates")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return D.build_ref(tmp_path_factory.mktemp("relposef_ref"))


def one(ref, a, b, **kw):
    off, pa, pb = D.batch([(a, b)])
    return [v[0] for v in D.ref_relpose_8pt(ref, off, pa, pb, **kw)]


@pytest.mark.parametrize("noise", [0.0, 0.5])
def test_single_sample_fit_against_numpy(ref, noise):
    """Eight matches drawn through the exported sampler: F (unit Frobenius norm, sign fixed) to 1e-8 of numpy's."""
    rng = np.random.default_rng(11)
    for k in range(10):
        a, b, _, _, _ = D.make_pair(rng, 200, noise=noise)
        idx = D.ref_sample8(ref, D.SEED_F8, 0, k, 200)
        assert len(set(idx.tolist())) == 8 and idx.min() >= 0 and idx.max() < 200
        good, F = D.ref_fit(ref, a[idx], b[idx])
        assert good
        err = np.abs(D.unit_F(F) - D.unit_F(D.numpy_fit(a[idx], b[idx]))).max()
        print("8-point fit, noise %.1f, sample %d: |dF| = %.3e" % (noise, k, err))
        assert err <= 1e-8


@pytest.mark.parametrize("n", [9, 12, 15])
@pytest.mark.parametrize("noise", [0.0, 0.5])
def test_all_points_fit_against_numpy(ref, n, noise):
    rng = np.random.default_rng(100 + n)
    for _ in range(5):
        a, b, _, _, _ = D.make_pair(rng, n, noise=noise)
        good, F = D.ref_fit(ref, a, b)
        assert good
        err = np.abs(D.unit_F(F) - D.unit_F(D.numpy_fit(a, b))).max()
        print("%d-point fit, noise %.1f: |dF| = %.3e" % (n, noise, err))
        assert err <= 1e-8
        # and the batch call on such a pair is that fit
        out = one(ref, a, b)
        np.testing.assert_array_equal(out[0], F)
        assert out[7] == 0 and out[9] == 1


@pytest.mark.parametrize("n", [8, 12, 200])
def test_noise_free_generic_pairs(ref, n):
    """Both focal lengths to 1e-8 relative (the margin is the Jacobi SVD against LAPACK), R to 1e-8, t parallel to the
    truth in the reference's convention (t = -R^T u: parallel to R^T t_true), every match in front of both cameras."""
    for seed in range(10):
        rng = np.random.default_rng(1000 * n + seed)
        a, b, R, t, X = D.make_pair(rng, n)
        F, f1, f2, E, Rr, tr, ok, bi, be, nc = one(ref, a, b)
        assert ok == 1 and nc == (1 if n < 16 else 200) and 0 <= bi < 200
        print("n %d seed %d: df_ref %.3e df_cur %.3e dR %.3e" % (n, seed, f1 / D.F_REF - 1, f2 / D.F_CUR - 1, np.abs(Rr - R).max()))
        assert abs(f1 / D.F_REF - 1) <= 1e-8 and abs(f2 / D.F_CUR - 1) <= 1e-8
        assert np.abs(Rr - R).max() <= 1e-8
        tn = np.linalg.norm(t)
        assert abs(np.linalg.norm(tr) - 1) <= 1e-9
        assert np.linalg.norm(np.cross(tr, R.T @ t / tn)) <= 1e-8
        # the reference hands back R^T t rather than t (the existing five-point arm documents the same): turned back,
        # it is the true translation with its sign, and the recovered pair of cameras sees every point in front
        tf = Rr @ tr
        assert tf @ t / tn >= 1 - 1e-8
        Xc = X @ Rr.T + tn * tf
        assert (X[:, 2] > 0).all() and (Xc[:, 2] > 0).all()
        xa = np.column_stack([a / f1, np.ones(n)]); xb = np.column_stack([b / f2, np.ones(n)])
        assert np.abs(np.einsum("ni,ij,nj->n", xb, E, xa)).max() <= 1e-8 * np.abs(E).max()
        ha = np.column_stack([a, np.ones(n)]); hb = np.column_stack([b, np.ones(n)])
        assert np.abs(np.einsum("ni,ij,nj->n", hb, F, ha)).max() <= 1e-8 * np.abs(F).max() * 5000


def test_algebraic_rotation_equals_atan2_form(ref):
    """c = e0 / |(e0, e1)|, s = -e1 / |(e0, e1)| is the rotation by atan2(-e1, e0): the focal lengths of the restatement
    equal a numpy evaluation of FocalLengthFromFMatrix in its atan2 / cos / sin form, on the same epipoles, to 1e-12."""
    rng = np.random.default_rng(21)
    compared = 0
    for k in range(20):
        a, b, _, _, _ = D.make_pair(rng, 12, noise=0.5 * (k % 2))
        good, F = D.ref_fit(ref, a, b)
        assert good
        ok, f1, f2, e1, e2 = D.ref_focal_from_F(ref, F)
        assert np.abs(F @ e1).max() <= 1e-9 * np.abs(F).max() and np.abs(F.T @ e2).max() <= 1e-9 * np.abs(F).max()

        def rot(e):
            th = np.arctan2(-e[1], e[0])
            return np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1.0]])
        r1, r2 = rot(e1), rot(e2)
        Fr = r2 @ F @ r1.T
        e1r, e2r = r1 @ e1, r2 @ e2
        M = np.diag(1 / np.array([e2r[2], 1, -e2r[0]])) @ Fr @ np.diag(1 / np.array([e1r[2], 1, -e1r[0]]))
        A, B, Cc, Dd = M[0, 0], M[0, 1], M[1, 0], M[1, 1]
        f1sq = (-A * Cc * e1r[0] ** 2) / (A * Cc * e1r[2] ** 2 + B * Dd)
        f2sq = (-A * B * e2r[0] ** 2) / (A * B * e2r[2] ** 2 + Cc * Dd)
        assert ok == (f1sq >= 0 and f2sq >= 0)
        if ok:
            compared += 1
            print("pair %d: %.3e %.3e" % (k, f1 / np.sqrt(f1sq) - 1, f2 / np.sqrt(f2sq) - 1))
            assert abs(f1 / np.sqrt(f1sq) - 1) <= 1e-12 and abs(f2 / np.sqrt(f2sq) - 1) <= 1e-12
    assert compared >= 10


def test_pose_from_E_equals_the_five_point_oracle(ref, oracle):
    """The decomposition and cheirality vote fed with the five-point oracle's E on pts / f: its R and t bit for bit."""
    off, a, b, _, _ = make_relpose_batch(77, [40, 200, 9], outlier_frac=0.1)
    f1, f2 = 4800.0, 4650.0
    E, R, t, ok, _ = oracle.relpose_5pt(off, a, b, f1, f2)
    assert ok.all()
    for p in range(3):
        s = slice(off[p], off[p + 1])
        Rr, tr = D.ref_pose_from_E(ref, E[p], a[s], b[s], f1, f2)
        np.testing.assert_array_equal(Rr, R[p])
        np.testing.assert_array_equal(tr, t[p])


@pytest.mark.parametrize("n", [0, 7])
def test_too_few_matches(ref, n):
    rng = np.random.default_rng(3)
    a, b, _, _, _ = D.make_pair(rng, n)
    F, f1, f2, E, R, t, ok, bi, be, nc = one(ref, a, b)
    assert ok == 0 and bi == -1 and be == 1e6 and nc == 0 and f1 == 0 and f2 == 0
    for m in (F, E, R, t):
        assert not m.any()


def test_repeated_match_is_not_a_candidate(ref):
    """A sample that holds the same match twice has a constraint matrix of rank 7: the kernel is not one-dimensional."""
    rng = np.random.default_rng(4)
    a, b, _, _, _ = D.make_pair(rng, 8)
    a[5], b[5] = a[2], b[2]
    assert not D.ref_fit(ref, a, b)[0]
    # a pair of 40 matches of which 30 are one and the same: most samples draw it twice
    a, b, _, _, _ = D.make_pair(rng, 40)
    a[10:], b[10:] = a[9], b[9]
    out = one(ref, a, b)
    dup = sum(len(set(np.minimum(D.ref_sample8(ref, D.SEED_F8, 0, it, 40), 9).tolist())) < 8 for it in range(200))
    assert dup > 0 and out[9] == 200 - dup and out[9] < 200


def test_all_errors_above_1e6_keep_the_first_candidate(ref):
    """Pixel coordinates scaled up until every Sampson sum is >= 1e6: idx_min stays 0, error_min stays 1e6."""
    rng = np.random.default_rng(5)
    a, b, _, _, _ = D.make_pair(rng, 300, noise=0.5)
    a, b = a * 1e4, b * 1e4
    F, f1, f2, E, R, t, ok, bi, be, nc = one(ref, a, b)
    assert nc == 200 and bi == 0 and be == 1e6
    idx = D.ref_sample8(ref, D.SEED_F8, 0, 0, 300)
    np.testing.assert_array_equal(F, D.ref_fit(ref, a[idx], b[idx])[1])


def test_pure_x_translation_stays_as_recorded(ref):
    """Identical orientation, translation along x: both epipoles are (1, 0, 0), the diagonal factors divide by e_z ~ 0.
    Recorded behaviour of the focal test on this scene (noise-free, 50 matches): it does not report a failure - the
    f^2 are non-negative or NaN - and what comes out is not the truth."""
    rng = np.random.default_rng(6)
    a, b, _, _, _ = D.make_pair(rng, 50, rot=np.zeros(3), centre=np.array([-30.0, 0.0, 0.0]), jitter=0.0)
    F, f1, f2, E, R, t, ok, bi, be, nc = one(ref, a, b)
    assert nc == 200 and ok == 1
    assert not (abs(f1 / D.F_REF - 1) < 1e-3 and abs(f2 / D.F_CUR - 1) < 1e-3)


def test_identical_points_terminate(ref):
    a = np.full((40, 2), 12.5)
    F, f1, f2, E, R, t, ok, bi, be, nc = one(ref, a, a.copy())
    assert nc == 0 and ok == 0 and bi == -1
    a = np.zeros((12, 2))
    out = one(ref, a, a.copy())       # the all-points SVD arm on 0 / 0
    assert out[6] in (0, 1)


def test_golden_fixture(ref):
    g = np.load(GOLD)
    out = D.ref_relpose_8pt(ref, g["off"], g["pts_ref"], g["pts_cur"], ransac_times=int(g["ransac_times"]), seed=int(g["seed"]))
    for name, v in zip(NAMES, out):
        np.testing.assert_array_equal(v, g[name], err_msg=name)
    assert g["ok"].any() and not g["ok"].all()
