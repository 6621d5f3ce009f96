"""CPU tests of the step checker (tests/ba_step_check.py) that tests/test_gpu_ba_large.py applies to the GPU's linear solve:
the oracle's own step passes, the Jacobi scale it reports is the complex-step one, and small corruptions of a step fail."""
import numpy as np
import pytest

from metricsfm_amd import scene
from tests import ba_step_check as K


@pytest.fixture(scope="module")
def case(oracle):
    """40 aerial cameras with one CameraModel each (use_same_camera = false: 9 reduced columns per camera, n = 360) and
    the SLAMGPS rows; the oracle's reduced system at x0 and its own first LM step."""
    sc = scene.make_aerial_scene(40, 2400, seed=1040, n_models=40, gps_sigma=0.5)
    mk = lambda: K.step_arrays(sc)
    ref = K.reference(oracle, mk())
    r, a = K.oracle_step(oracle, mk)
    return sc, mk, ref, r, a


def test_oracle_step_passes(case):
    sc, mk, ref, r, a = case
    assert len(ref["rhs"]) == 9 * sc.n_cams
    assert r["iterations"]["step_is_successful"][1] == 1
    # iteration 0 of the solve is the reduced system's linearisation point
    assert r["iterations"]["cost"][0] == ref["cost"] and r["iterations"]["gradient_max_norm"][0] == ref["gmax"]
    eta = K.check_step(ref, K.scaled_step(ref, a), K.STEP_BAR)
    assert eta < 1e-15, eta   # measured: 2.9e-17


def test_scale_is_the_complex_step_column_scale(case):
    """Ceres' jacobian_scaling_ = 1 / (1 + |column|) from SparseLM's complex-step Jacobian (tests/independent_lm.py)."""
    from tests.independent_lm import SparseLM
    sc, mk, ref, _, _ = case
    arr = mk()
    lm = SparseLM(arr)
    _, J = lm.linearise(arr.cam_pose, arr.cam_model, arr.point)
    scale = 1.0 / (1.0 + np.sqrt(np.asarray(J.multiply(J).sum(0)).ravel()))
    n = len(ref["scale"])
    assert lm.n > n and 6 * int(lm.cu.sum()) + 3 * int(lm.mu.sum()) == n   # (SparseLM's point columns come after these)
    np.testing.assert_allclose(ref["scale"], scale[:n], rtol=1e-12)
    assert (ref["scale"] < 1.0).all() and (ref["scale"] > 0.0).all()


@pytest.mark.parametrize("block", [0, 3, 5])
def test_a_block_off_by_one_part_in_a_million_fails(case, block):
    sc, mk, ref, _, a = case
    y = K.scaled_step(ref, a)
    y[64 * block:64 * block + 64] *= 1 + 1e-6
    eta, res = K.backward_error(ref["S"], y, ref["rhs"])
    assert eta > 100 * K.STEP_BAR, eta
    # the report names the worst block: the scaled one itself, except for the intrinsics block (5, the last 40 columns),
    # whose error shows most in the cameras it couples to
    b = K.worst_block(res)[0]
    assert b == block or block == 5
    with pytest.raises(AssertionError, match="columns %d\\.\\." % (64 * b)):
        K.check_step(ref, y, K.STEP_BAR)


@pytest.mark.parametrize("pair", [(0, 1), (2, 4)])
def test_two_swapped_blocks_fail(case, pair):
    sc, mk, ref, _, a = case
    y = K.scaled_step(ref, a)
    b0, b1 = pair
    y[64 * b0:64 * b0 + 64], y[64 * b1:64 * b1 + 64] = y[64 * b1:64 * b1 + 64].copy(), y[64 * b0:64 * b0 + 64].copy()
    eta, _ = K.backward_error(ref["S"], y, ref["rhs"])
    assert eta > 100 * K.STEP_BAR, eta
    with pytest.raises(AssertionError):
        K.check_step(ref, y, K.STEP_BAR)


def test_backward_error_of_a_dense_symmetric_system():
    """The blocked symmetrisation against numpy on a matrix whose lower triangle holds garbage (never read)."""
    rng = np.random.default_rng(4)
    n = 2500
    B = rng.standard_normal((n, n))
    Sf = B @ B.T + n * np.eye(n)
    y = rng.standard_normal(n)
    rhs = Sf @ y + 1e-3 * rng.standard_normal(n)   # (a residual far above the rounding of either product)
    S = np.triu(Sf) + np.tril(rng.standard_normal((n, n)), -1)
    eta, res = K.backward_error(S, y, rhs, rows=700)
    np.testing.assert_allclose(res, Sf @ y - rhs, rtol=0, atol=1e-9 * np.abs(Sf @ y).max())
    want = np.linalg.norm(Sf @ y - rhs) / (np.linalg.norm(Sf) * np.linalg.norm(y) + np.linalg.norm(rhs))
    assert abs(eta - want) <= 1e-9 * want
