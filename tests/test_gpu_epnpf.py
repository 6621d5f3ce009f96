"""The batched EPnP focal sweep on the GPU (msfm_epnpf_sweep_batch; reference AbsolutePoseEstimation::AbsolutePoseWithoutFocalLength,
absolute_pose_estimation.cc:28-40 -> AbsolutePoseEPNPF::EPNPF, absolute_pose_via_epnpf.cc:34-63) against the CPU reference
composed from the oracle (tests/epnpf_ref.py) and against msfm_epnp_ransac_batch on the expanded batch.
Step i of image p is problem p * n_steps + i of that call: every comparison is exact."""
import ctypes as C
import os

import numpy as np
import pytest

from metricsfm_amd import _abi as A
from metricsfm_amd import capi
from tests import epnpf_ref
from tests.twoview import make_pnp_batch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden", "epnpf_golden.npz")
NAMES = ("f", "R", "t", "errors", "avg_error", "best_step", "best_iter", "step_error")


@pytest.fixture(scope="module")
def O(oracle):
    return oracle


def equal(g, o):
    assert len(g) == len(o) == len(NAMES)
    for a, b, k in zip(g, o, NAMES):
        np.testing.assert_array_equal(a, b, err_msg=k)   # NaNs compare equal, everything else bit for bit


def test_sweep_matches_reference_defaults_mixed_batch(ctx, O):
    sizes = [300, 0, 3, 4, 5, 60, 2500, 50]
    off, X, x, _, _ = make_pnp_batch(11, sizes, outlier_frac=0.15)
    x[off[7]:] = np.random.default_rng(12).uniform(-1500, 1500, (50, 2))   # an image no pose explains
    g = ctx.epnpf_sweep(off, X, x, 4800.0, keep_step_errors=True)
    o = epnpf_ref.epnpf_sweep(O, off, X, x, 4800.0)
    equal(g, o)
    f, R, t, err, avg, bs, bi, se = g
    assert se.shape == (8, 350)
    for p in (1, 2):   # fewer than 4 points: nothing selected
        assert bs[p] == -1 and bi[p] == -1 and f[p] == 4800.0 and avg[p] == 10000.0 and not R[p].any() and (se[p] == 1e9).all()
    for p in (0, 3, 4, 5, 6, 7):
        assert bs[p] >= 0 and bi[p] >= 0 and f[p] == (0.5 + int(bs[p]) * 0.01) * 4800.0
    # the 4-point image: every step returns the minimal solver's "no fit" (the CPU reference says so), and 100000.0 < 1000000.0 keeps step 0
    assert (se[3] == 100000.0).all() and bs[3] == 0 and bi[3] == 0 and f[3] == 2400.0
    assert bs[4] > 0 and se[4].min() < 10.0   # the 5-point image keeps a real step


@pytest.mark.parametrize("seed,iters", [(1, 37), (2, 1000)])
def test_sweep_matches_reference_options(ctx, O, seed, iters):
    off, X, x, _, _ = make_pnp_batch(20 + seed, [120, 4, 33, 700], outlier_frac=0.3, noise=1.0)
    f_init = np.array([4800.0, 4000.0, 5200.0, 2500.0])
    kw = dict(f_ratio_min=0.8, f_ratio_max=1.25, f_ratio_step=0.05, max_iter=iters, seed=5 + seed)
    g = ctx.epnpf_sweep(off, X, x, f_init, keep_step_errors=True, **kw)
    assert g[7].shape == (4, 8)   # (1.25 - 0.8) / 0.05 = 8.99...: 8 steps
    equal(g, epnpf_ref.epnpf_sweep(O, off, X, x, f_init, **kw))
    short = ctx.epnpf_sweep(off, X, x, f_init, **kw)   # the step errors are optional, nothing else changes
    assert len(short) == 7
    equal(short + (g[7],), g)


def test_sweep_is_the_plain_call_on_the_expanded_batch(ctx):
    sizes = [90, 3, 150, 5]
    off, X, x, _, _ = make_pnp_batch(31, sizes, outlier_frac=0.2)
    f_init = np.array([4800.0, 4500.0, 5100.0, 4000.0])
    lo, step, S = 0.9, 0.02, 10
    f, R, t, err, avg, bs, bi, se = ctx.epnpf_sweep(off, X, x, f_init, f_ratio_min=lo, f_ratio_max=1.1, f_ratio_step=step,
                                                    max_iter=100, seed=9, keep_step_errors=True)
    assert se.shape == (4, S)
    eoff = np.concatenate([[0], np.cumsum(np.repeat(sizes, S))]).astype(np.int32)
    eX = np.concatenate([np.tile(X[off[p]:off[p + 1]], (S, 1)) for p in range(4)])
    ex = np.concatenate([np.tile(x[off[p]:off[p + 1]], (S, 1)) for p in range(4)])
    ef = np.array([(lo + i * step) * f_init[p] for p in range(4) for i in range(S)])
    R1, t1, e1, a1, b1 = ctx.epnp_ransac(eoff, eX, ex, ef, max_iter=100, seed=9)
    for p in range(4):
        if sizes[p] < 4:
            assert bs[p] == -1 and bi[p] == -1 and f[p] == f_init[p]
            q = p * S   # any of its steps: the result of an image with fewer than 4 points
        else:
            assert bs[p] == int(np.argmin(se[p])) and se[p].min() < 1e6   # argmin returns the first minimum
            q = p * S + int(bs[p])
            assert f[p] == ef[q] and bi[p] == b1[q]
        np.testing.assert_array_equal(R[p], R1[q])
        np.testing.assert_array_equal(t[p], t1[q])
        np.testing.assert_array_equal(err[off[p]:off[p + 1]], e1[eoff[q]:eoff[q + 1]])
        assert avg[p] == a1[q]


def test_sweep_is_independent_of_the_batch_split(ctx):
    off, X, x, _, _ = make_pnp_batch(32, [80, 90, 100], outlier_frac=0.2)
    f_init = np.array([4800.0, 4000.0, 5200.0])
    whole = ctx.epnpf_sweep(off, X, x, f_init, keep_step_errors=True)
    one = ctx.epnpf_sweep(off[:2], X[:off[1]], x[:off[1]], f_init[:1], keep_step_errors=True)
    for k, w, a in zip(NAMES, whole, one):
        np.testing.assert_array_equal(w[:off[1]] if k == "errors" else w[:1], a, err_msg=k)


def test_sweep_degenerate_inputs(ctx, O):
    rng = np.random.default_rng(5)
    off = np.array([0, 30, 60, 90], np.int32)
    X = np.concatenate([np.column_stack([rng.uniform(-40, 40, 30), rng.uniform(-30, 30, 30), np.zeros(30)]),   # coplanar
                        np.tile([[1.0, 2.0, 3.0]], (30, 1)),                                                     # one point
                        np.column_stack([np.arange(30.0), 2 * np.arange(30.0), 3 * np.arange(30.0)])])           # collinear
    x = rng.uniform(-1000, 1000, (90, 2))
    kw = dict(f_ratio_min=0.5, f_ratio_max=1.5, f_ratio_step=0.05, max_iter=64)
    equal(ctx.epnpf_sweep(off, X, x, 4800.0, keep_step_errors=True, **kw), epnpf_ref.epnpf_sweep(O, off, X, x, 4800.0, **kw))


def test_sweep_known_answer(ctx):
    # exact correspondences at f = 4800 and f_init = 4800: candidate 50 is (0.5 + 50 * 0.01) * 4800 = 4800.0 exactly
    off, X, x, R, t = make_pnp_batch(7, [300, 60], outlier_frac=0, noise=0, f=4800)
    f, Rg, tg, err, avg, bs, bi, se = ctx.epnpf_sweep(off, X, x, 4800.0, keep_step_errors=True)
    assert list(bs) == [50, 50] and list(f) == [4800.0, 4800.0]
    assert (se[:, 50] < 1e-2).all() and (avg < 1e-2).all()
    assert np.abs(Rg - R).max() < 1e-4


def test_invalid_arguments_leave_the_context_usable(ctx):
    off, X, x, _, _ = make_pnp_batch(8, [40, 50], outlier_frac=0.1)
    good = ctx.epnpf_sweep(off, X, x, 4800.0, f_ratio_min=0.9, f_ratio_max=1.1, f_ratio_step=0.02, max_iter=16)
    for kw in (dict(f_ratio_step=0.0), dict(f_ratio_step=-0.01), dict(f_ratio_max=0.5), dict(f_ratio_max=0.25),
               dict(f_ratio_step=10.0),                                  # 0 steps
               dict(f_ratio_step=1e-5),                                  # 350000 steps > 65535
               dict(max_iter=0), dict(max_iter=65537)):
        with pytest.raises(capi.MsfmError) as e:
            ctx.epnpf_sweep(off, X, x, 4800.0, **kw)
        assert e.value.code == A.MSFM_E_INVAL, kw
    for bad in (np.array([1, 40, 90], np.int32), np.array([0, 50, 40], np.int32)):
        with pytest.raises(capi.MsfmError) as e:
            ctx.epnpf_sweep(bad, X, x, 4800.0)
        assert e.value.code == A.MSFM_E_INVAL
    # n_problems * n_steps must fit an int: 65535 empty images x 65535 steps
    with pytest.raises(capi.MsfmError) as e:
        ctx.epnpf_sweep(np.zeros(65536, np.int32), np.zeros((0, 3)), np.zeros((0, 2)), 4800.0, f_ratio_min=0.0, f_ratio_max=65535.5,
                        f_ratio_step=1.0)
    assert e.value.code == A.MSFM_E_INVAL
    with pytest.raises(capi.MsfmError) as e:   # the sibling's limit on the batch
        ctx.epnpf_sweep(np.zeros(65537, np.int32), np.zeros((0, 3)), np.zeros((0, 2)), 4800.0)
    assert e.value.code == A.MSFM_E_INVAL
    o = capi.epnpf_options()   # required pointers missing
    assert capi.lib().msfm_epnpf_sweep_batch(ctx._h, 2, A.ptr(off, A.c_int_p), A.ptr(X, A.c_double_p), A.ptr(x, A.c_double_p), None, C.byref(o),
                                             None, None, None, None, None, None, None, None) == A.MSFM_E_INVAL
    again = ctx.epnpf_sweep(off, X, x, 4800.0, f_ratio_min=0.9, f_ratio_max=1.1, f_ratio_step=0.02, max_iter=16)
    for a, b in zip(good, again):
        np.testing.assert_array_equal(a, b)


def test_golden_fixture(ctx):
    z = np.load(GOLD)
    g = ctx.epnpf_sweep(z["off"], z["X"], z["x"], z["f_init"], seed=int(z["seed"]), keep_step_errors=True)
    for a, k in zip(g, NAMES):
        np.testing.assert_array_equal(a, z[k], err_msg=k)
