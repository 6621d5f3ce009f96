"""The focal sweep's CPU side (no GPU): the reference composed from the oracle (tests/epnpf_ref.py), the step count of
msfm_epnpf_num_steps, and the committed fixture (the options struct against the C compiler: tests/test_abi.py)."""
import os

import numpy as np
import pytest

from metricsfm_amd import _abi as A
from metricsfm_amd import capi
from tests import epnpf_ref
from tests.golden import make_epnpf_golden as G
from tests.twoview import make_pnp_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restated_sampler_reproduces_the_kept_sample(oracle):
    # the kept sample of a plain oracle.epnp_ransac problem, solved again from sample4's indices: same pose, bit for bit
    off, X, x, _, _ = make_pnp_batch(21, [50, 9, 200], outlier_frac=0.2)
    for seed, iters in ((0x4D53464D50, 200), (77, 13)):
        R, t, _, _, best = oracle.epnp_ransac(off, X, x, 4800.0, max_iter=iters, seed=seed)
        for p in range(3):
            idx = epnpf_ref.sample4(seed, p, int(best[p]), int(off[p + 1] - off[p]))
            assert len(set(idx)) == 4
            R4, t4, _ = oracle._test_epnp4(X[off[p]:off[p + 1]][idx], x[off[p]:off[p + 1]][idx], 4800.0)
            np.testing.assert_array_equal(R4, R[p])
            np.testing.assert_array_equal(t4, t[p])


def test_reference_sweep_is_the_sequential_loop(oracle):
    # epnpf_sweep asserts the R / t cross-check on every step; here its selection against the step errors it returns
    off, X, x, _, _ = make_pnp_batch(22, [30, 2, 4, 5], outlier_frac=0.2)
    f, R, t, err, avg, bs, bi, se = epnpf_ref.epnpf_sweep(oracle, off, X, x, [4000.0, 4100.0, 4200.0, 4300.0], 0.8, 1.25, 0.05, max_iter=20)
    assert se.shape == (4, 8)
    assert bs[1] == -1 and bi[1] == -1 and f[1] == 4100.0 and avg[1] == 10000.0 and (se[1] == 1e9).all() and not R[1].any()
    for p in (0, 2, 3):
        assert bs[p] == int(np.argmin(se[p])) and se[p].min() < 1e6     # argmin = the first minimum
        assert f[p] == (0.8 + int(bs[p]) * 0.05) * [4000.0, 4100.0, 4200.0, 4300.0][p]
        # the winner's outputs are the plain call's at that focal length and problem index
        o1 = np.concatenate([np.zeros(p * 8 + int(bs[p]), np.int32), [0, off[p + 1] - off[p]]]).astype(np.int32)
        R1, t1, e1, a1, b1 = oracle.epnp_ransac(o1, X[off[p]:off[p + 1]], x[off[p]:off[p + 1]], f[p], max_iter=20)
        np.testing.assert_array_equal(R1[-1], R[p])
        np.testing.assert_array_equal(e1, err[off[p]:off[p + 1]])
        assert a1[-1] == avg[p] and b1[-1] == bi[p]


@pytest.mark.parametrize("lo,hi,step,want", [(0.5, 4.0, 0.01, 350), (0.8, 1.25, 0.05, 8), (0.9, 1.1, 0.02, 10)])
def test_step_count_is_the_binary64_expression(lo, hi, step, want):
    assert int((hi - lo) / step) == want   # absolute_pose_via_epnpf.cc:44; (1.25 - 0.8) / 0.05 is 8.999..., not 9
    assert epnpf_ref.num_steps(lo, hi, step) == want
    assert capi.epnpf_num_steps(f_ratio_min=lo, f_ratio_max=hi, f_ratio_step=step) == want


def test_defaults_and_invalid_step_counts():
    o = capi.epnpf_options()
    assert (o.f_ratio_min, o.f_ratio_max, o.f_ratio_step, o.max_iter, o.seed) == (0.5, 4.0, 0.01, 200, 0x4D53464D50)
    assert capi.epnpf_num_steps() == 350
    for kw in (dict(f_ratio_step=0.0), dict(f_ratio_step=-0.01), dict(f_ratio_step=float("nan")), dict(f_ratio_max=0.5),
               dict(f_ratio_max=0.4), dict(f_ratio_step=10.0), dict(f_ratio_step=1e-6), dict(f_ratio_max=float("inf"))):
        assert capi.epnpf_num_steps(**kw) == A.MSFM_E_INVAL, kw
    assert capi.epnpf_num_steps(f_ratio_min=0.0, f_ratio_max=65535.5, f_ratio_step=1.0) == 65535
    assert capi.epnpf_num_steps(f_ratio_min=0.0, f_ratio_max=65536.0, f_ratio_step=1.0) == A.MSFM_E_INVAL


def test_golden_fixture_reproduces_from_the_reference(oracle):
    z = np.load(os.path.join(ROOT, "tests", "golden", "epnpf_golden.npz"))
    off, X, x, f_init = G.inputs()
    for a, k in zip((off, X, x, f_init), ("off", "X", "x", "f_init")):
        np.testing.assert_array_equal(a, z[k])
    assert int(z["seed"]) == G.SEED and z["step_error"].shape == (3, 350)
    for a, k in zip(epnpf_ref.epnpf_sweep(oracle, off, X, x, f_init, seed=G.SEED), G.KEYS):
        np.testing.assert_array_equal(a, z[k])
