"""msfm_relpose_8pt_batch - RelativePoseEstimation::RelativePoseWithoutFocalLength for a batch of seed-pair candidates - against
its sequential CPU restatement tests/relposef_ref.cpp: every output bit for bit (NaN equal to NaN), over a mixed batch, other
options, the batch split, the optional outputs, and the committed fixture."""
import os

import numpy as np
import pytest

from tests import relposef_data as D
from tests.twoview import make_relpose_batch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden", "relposef_golden.npz")
NAMES = ("F", "f_ref", "f_cur", "E", "R", "t", "ok", "best_iter", "best_error", "n_candidates")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return D.build_ref(tmp_path_factory.mktemp("relposef_ref"))


def same(got, want):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        np.testing.assert_array_equal(g, w, err_msg=name)


def test_mixed_batch_bit_for_bit(ctx, ref):
    off, a, b = D.make_mixed_batch(7)
    assert np.diff(off).tolist() == D.MIXED_SIZES
    want = D.ref_relpose_8pt(ref, off, a, b)
    got = ctx.relpose_8pt(off, a, b)
    same(got, want)
    ok, nc = got[6], got[9]
    assert ok[1] == 0 and ok[2] == 0 and nc[1] == 0 and nc[2] == 0
    assert nc[3] == 1 and nc[4] == 1 and nc[5] == 1 and nc[6] == 200 and nc[7] == 200
    assert ok[7] == 1                  # 2500 generic matches with noise alone yield focal lengths


def test_noise_free_pair_recovers_the_truth(ctx):
    rng = np.random.default_rng(8)
    a, b, R, t, _ = D.make_pair(rng, 200)
    F, f1, f2, E, Rr, tr, ok, bi, be, nc = ctx.relpose_8pt([0, 200], a, b)
    assert ok[0] == 1 and nc[0] == 200
    assert abs(f1[0] / D.F_REF - 1) <= 1e-8 and abs(f2[0] / D.F_CUR - 1) <= 1e-8
    assert np.abs(Rr[0] - R).max() <= 1e-8
    assert np.linalg.norm(np.cross(tr[0], R.T @ t / np.linalg.norm(t))) <= 1e-8


@pytest.mark.parametrize("seed,times", [(1, 37), (2, 1000)])
def test_options(ctx, ref, seed, times):
    off, a, b = D.make_mixed_batch(9, [300, 8, 16, 700, 15, 50])
    same(ctx.relpose_8pt(off, a, b, ransac_times=times, seed=seed), D.ref_relpose_8pt(ref, off, a, b, ransac_times=times, seed=seed))


def test_no_candidate_below_the_threshold(ctx, ref):
    """Unrelated points: every fit scores 1e6 or more, so the first candidate is kept and best_error stays at its start,
    whether the candidates fit one stride of the selection's 256 threads or not."""
    rng = np.random.default_rng(3)
    sizes = [300, 16, 40]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    a = rng.uniform(-2000, 2000, (off[-1], 2))
    b = rng.uniform(-2000, 2000, (off[-1], 2))
    for times in (1, 65, 300):
        want = D.ref_relpose_8pt(ref, off, a, b, ransac_times=times, seed=4)
        ok, bi, be, nc = want[6], want[7], want[8], want[9]
        assert (be == 1e6).all() and (bi == 0).all() and (nc == times).all() and (ok == 0).all(), times
        same(ctx.relpose_8pt(off, a, b, ransac_times=times, seed=4), want)


def test_golden_fixture(ctx):
    g = np.load(GOLD)
    got = ctx.relpose_8pt(g["off"], g["pts_ref"], g["pts_cur"], ransac_times=int(g["ransac_times"]), seed=int(g["seed"]))
    same(got, [g[k] for k in NAMES])


def test_batch_split_rule(ctx):
    """Sample `it` of a pair is keyed by (seed, the pair's index within the call, it, its number of matches) and by nothing
    else: pair p of a batch equals the last pair of a call whose first p pairs are empty."""
    off, a, b = D.make_mixed_batch(10, [300, 40, 16, 700, 15, 50])
    whole = ctx.relpose_8pt(off, a, b)
    for p in range(len(off) - 1):
        s = slice(off[p], off[p + 1])
        alone = ctx.relpose_8pt([0] * (p + 1) + [off[p + 1] - off[p]], a[s], b[s])
        for name, w, g in zip(NAMES, whole, alone):
            np.testing.assert_array_equal(g[p], w[p], err_msg="%s of pair %d" % (name, p))
            assert not g[:p].any() or name in ("best_iter", "best_error")
    # and with other pairs around it in another order of sizes, as long as the index stays
    off2, a2, b2 = D.batch([(a[off[k]:off[k + 1]], b[off[k]:off[k + 1]]) if k == 3 else (a[:20 + k], b[:20 + k]) for k in range(6)])
    other = ctx.relpose_8pt(off2, a2, b2)
    for name, w, g in zip(NAMES, whole, other):
        np.testing.assert_array_equal(g[3], w[3], err_msg=name)


def test_optional_outputs_and_repeatability(ctx):
    off, a, b = D.make_mixed_batch(11, [300, 7, 16, 100])
    full = ctx.relpose_8pt(off, a, b)
    again = ctx.relpose_8pt(off, a, b)
    bare = ctx.relpose_8pt(off, a, b, diagnostics=False)
    same(again, full)
    assert bare[7] is None and bare[8] is None and bare[9] is None
    for name, g, w in zip(NAMES[:7], bare, full):
        np.testing.assert_array_equal(g, w, err_msg=name)


def test_argument_checks(ctx):
    from metricsfm_amd.capi import MsfmError
    off, a, b = D.make_mixed_batch(12, [20, 30])
    for times in (0, 65537):
        with pytest.raises(MsfmError):
            ctx.relpose_8pt(off, a, b, ransac_times=times)
    with pytest.raises(MsfmError):
        ctx.relpose_8pt([0, 30, 20], a, b)
    out = ctx.relpose_8pt([0], a[:0], b[:0])
    assert all(len(v) == 0 for v in out)


def test_five_point_path_unchanged(ctx, oracle):
    """The decomposition and cheirality vote now shared with the eight-point arm: msfm_relpose_5pt_batch still equals its oracle."""
    off, a, b, _, _ = make_relpose_batch(13, [400, 4, 5, 9, 10, 1500, 60], outlier_frac=0.15)
    got = ctx.relpose_5pt(off, a, b, 4800.0, 4650.0, ransac_times=64, seed=5)
    want = oracle.relpose_5pt(off, a, b, 4800.0, 4650.0, ransac_times=64, seed=5)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)
