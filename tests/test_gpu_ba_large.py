"""The bundle adjustment past config 3's size, where the dense Cholesky (chol.hip) changes code paths: config 5's global
solve with GPS rows against the oracle, and a ladder of systems up to 23 k columns whose GPU step is checked against the
oracle's reduced system (tests/ba_step_check.py).  Every case asserts which factorisation and back-substitution paths ran
(msfm_ba_layout.solve_paths)."""
import numpy as np
import pytest

from metricsfm_amd import _abi as A
from metricsfm_amd import scene
from tests import ba_step_check as K

pytestmark = pytest.mark.gpu

BACK = A.MSFM_PATH_BACKSOLVE_CHAIN

_C5 = {}


def _c5():
    """BASELINE config 5 (2000 aerial cameras / 1 M points / 6 M observations, one shared CameraModel, GPS rows), as
    SLAMGPS::FullBundleAdjustment hands it over (slam_gps.cc:675-863): built once per session."""
    if "sc" not in _C5:
        _C5["sc"] = scene.config_scene(5)
    return _C5["sc"]


def _resident(ctx, monkeypatch, make, env, iters):
    from metricsfm_amd import capi
    for k in ("MSFM_CHOL_DOMAINS", "MSFM_CHOL_LAUNCHES"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    a = make()
    ba = ctx.ba(a)
    try:
        r = ba.run(capi.default_options(max_num_iterations=iters, **K.NO_STOP))
        lay = ba.layout()
        a.cam_pose[:], a.cam_model[:], a.point[:] = ba.download()
    finally:
        ba.close()
        for k in env:
            monkeypatch.delenv(k)
    return r, lay, a


def test_ba_config5_global_oracle_parity(ctx, oracle):
    """Two LM iterations of config 5's full BA (n = 6 * 2000 + 3 = 12 003) against the oracle on every host core: same
    accept / reject sequence, costs to 1e-9, parameters to 1e-7 (check_parity)."""
    import time
    from tests.test_gpu_ba import check_parity
    t0 = time.perf_counter()
    sc = _c5()
    t_scene = time.perf_counter() - t0
    r, r_ref, _ = check_parity(ctx, oracle, lambda: K.step_arrays(sc),
                               dict(max_num_iterations=2, num_threads=oracle.host_cores(), **K.NO_STOP))
    print("config 5: host scene %.1f s, oracle set-up %.1f s + 2 iterations %.1f s on %d threads" % (
        t_scene, r_ref["setup_ms"] / 1e3, r_ref["solve_ms"] / 1e3, oracle.host_cores()))
    assert r["num_reduced_params"] == 12003 and r["num_iterations"] == 2
    assert r["num_residuals"] == 2 * sc.n_obs + 3 * sc.n_cams


def test_ba_config5_global_gpu_orders_and_paths(ctx, monkeypatch):
    """Config 5's full BA on the GPU alone: the dense elimination order against the automatic one (rounding), one launch per
    panel and block pair (MSFM_CHOL_LAUNCHES=1) against the default (bit-identical), and two default runs (bit-identical)."""
    sc = _c5()
    mk = lambda: K.step_arrays(sc)
    runs = {name: _resident(ctx, monkeypatch, mk, env, 2)
            for name, env in (("auto", {}), ("auto2", {}), ("dense", dict(MSFM_CHOL_DOMAINS="0")),
                              ("launches", dict(MSFM_CHOL_LAUNCHES="1")))}
    r, lay, a = runs["auto"]
    print("config 5 layout:", lay)
    # the automatic order cuts the camera graph three times (8 leaves | 4 | 2 | root); the leaf and first separator levels
    # are too wide for the persistent chain beside their row owners and run one launch per panel, the last separator level,
    # the root and the back substitution run as one launch each
    assert lay["reduced_order"] == 12003 and lay["n_domains"] > 1 and lay["n_levels"] == 3
    assert lay["solve_paths"] == A.MSFM_PATH_LEVEL_CHAIN(2) | A.MSFM_PATH_ROOT_CHAIN | BACK, hex(lay["solve_paths"])
    assert runs["auto2"][1]["solve_paths"] == lay["solve_paths"]
    assert runs["launches"][1]["solve_paths"] == 0
    for other in ("auto2", "launches"):
        r1, _, a1 = runs[other]
        for key in ("cost", "gradient_max_norm", "step_norm", "step_is_successful"):
            np.testing.assert_array_equal(r["iterations"][key], r1["iterations"][key], err_msg=other)
        for name in ("cam_pose", "cam_model", "point"):
            np.testing.assert_array_equal(getattr(a, name), getattr(a1, name), err_msg=other)
    r0, lay0, a0 = runs["dense"]
    assert lay0["n_domains"] == 1 and lay0["system_order"] == 12003
    np.testing.assert_array_equal(r0["iterations"]["step_is_successful"], r["iterations"]["step_is_successful"])
    np.testing.assert_allclose(r0["iterations"]["cost"], r["iterations"]["cost"], rtol=1e-9)
    for name in ("cam_pose", "cam_model", "point"):
        g, w = getattr(a0, name), getattr(a, name)
        assert np.abs(g - w).max() <= 1e-7 * np.abs(w).max(), name


FACTOR_CHAINS = A.MSFM_PATH_LEVEL_CHAIN(0) | A.MSFM_PATH_LEVEL_CHAIN(1) | A.MSFM_PATH_LEVEL_CHAIN(2) | A.MSFM_PATH_ROOT_CHAIN
LEVEL_CHAINS = A.MSFM_PATH_LEVEL_CHAIN(0) | A.MSFM_PATH_LEVEL_CHAIN(1) | A.MSFM_PATH_LEVEL_CHAIN(2)

# (case, cameras, CameraModels, MSFM_CHOL_DOMAINS, reduced order, system order range, solve_paths bits that must all be set,
#  bits of which one at least must be set, bits that must be clear).  In the dense order (one CameraModel per camera, 9
#  columns each) no factorisation from 14 k columns on has room for the persistent chain beside its row owners: those cases
#  cross the back-substitution limit and put M past 2 and 4 GiB on the launch path.  The persistent chain on a factor past
#  2 GiB comes from the dissected order of one shared CameraModel, cameras placed from the system order (domain padding
#  included) on both sides of npad = 23 168, the largest whose byte offsets fit the chain's 32-bit buffer addressing.
LADDER = [
    ("c3", 500, 1, None, 3003, (3003, 4096), BACK, LEVEL_CHAINS, 0),                     # control: config 3's shape
    ("dense_back_chain_224", 1592, 1592, "0", 14328, (14328, 14328), BACK, 0, FACTOR_CHAINS),   # 224 blocks: one launch
    ("dense_back_pairs_225", 1593, 1593, "0", 14337, (14337, 14337), 0, 0, FACTOR_CHAINS | BACK),  # 225: by block pairs
    ("dense_m_2_6gb", 2000, 2000, "0", 18000, (18000, 18000), 0, 0, FACTOR_CHAINS | BACK),   # npad 18 048: offsets past 2^31
    ("dense_npad_23168", 2574, 2574, "0", 23166, (23166, 23166), 0, 0, FACTOR_CHAINS | BACK),
    ("dense_npad_23232", 2575, 2575, "0", 23175, (23175, 23175), 0, 0, FACTOR_CHAINS | BACK),
    # 3795 cameras: system order 23 139 (8 | 4 | 2 | root), npad 23 168 - M is 4.29 GB and the last separator level and the
    # root run as persistent launches; 3794 cameras: 23 173 (the cut falls elsewhere), npad 23 232 - no persistent launch
    ("dissected_npad_23168", 3795, 1, None, 6 * 3795 + 3, (23104, 23167), A.MSFM_PATH_LEVEL_CHAIN(2) | A.MSFM_PATH_ROOT_CHAIN,
     LEVEL_CHAINS, BACK),
    ("dissected_npad_23232", 3794, 1, None, 6 * 3794 + 3, (23168, 23231), 0, 0, FACTOR_CHAINS | BACK),
]


@pytest.mark.parametrize("case", LADDER, ids=[c[0] for c in LADDER])
def test_ba_large_step_backward_error(ctx, oracle, monkeypatch, case):
    """One GPU LM iteration of an aerial scene (~60 points per camera, GPS rows): its camera step solves the oracle's reduced
    system with a normwise backward error below K.STEP_BAR, and iteration 0's cost and gradient match the oracle's.  Where
    the persistent chain ran on a factor past 2 GiB, one launch per panel (MSFM_CHOL_LAUNCHES=1) gives the same bits."""
    import time
    name, n_cams, n_models, domains, n_red, so_range, must, must_any, must_not = case
    t0 = time.perf_counter()
    # (start perturbations as in test_gpu_ba.py: with the generator's defaults the first step is rejected from 18 000
    #  columns on, by the oracle too, and a rejected step leaves nothing to check)
    sc = scene.make_aerial_scene(n_cams, 60 * n_cams, seed=1000 + n_cams, n_models=n_models, gps_sigma=0.5, rot_sigma=0.02,
                                 trans_sigma=0.2, point_sigma=0.2)
    t_scene = time.perf_counter() - t0
    mk = lambda: K.step_arrays(sc)
    env = {} if domains is None else dict(MSFM_CHOL_DOMAINS=domains)
    r, lay, a = _resident(ctx, monkeypatch, mk, env, 1)
    print("%s: layout %s" % (name, lay))
    assert lay["reduced_order"] == r["num_reduced_params"] == n_red
    assert so_range[0] <= lay["system_order"] <= so_range[1], (name, lay["system_order"])
    paths = lay["solve_paths"]
    assert paths & must == must and paths & must_not == 0, (name, hex(paths))
    assert must_any == 0 or paths & must_any != 0, (name, hex(paths))
    assert r["iterations"]["step_is_successful"][1] == 1, "the first step must be accepted"
    t0 = time.perf_counter()
    ref = K.reference(oracle, mk())
    t_ref = time.perf_counter() - t0
    assert r["iterations"]["cost"][0] == pytest.approx(ref["cost"], rel=K.COST_RTOL, abs=0)
    assert r["iterations"]["gradient_max_norm"][0] == pytest.approx(ref["gmax"], rel=K.GMAX_RTOL, abs=0)
    t0 = time.perf_counter()
    eta = K.check_step(ref, K.scaled_step(ref, a), K.STEP_BAR)
    t_eta = time.perf_counter() - t0
    print("%s: n %d, system order %d, solve_paths %#x, eta %.3e; host: scene %.1f s, reduced system %.1f s, eta %.1f s"
          % (name, n_red, lay["system_order"], paths, eta, t_scene, t_ref, t_eta))
    if paths & FACTOR_CHAINS and lay["system_order"] + 1 > 16384:
        # the persistent chain ran on a factor past 2 GiB: one launch per panel must give the same bits
        r1, lay1, a1 = _resident(ctx, monkeypatch, mk, dict(env, MSFM_CHOL_LAUNCHES="1"), 1)
        assert lay1["solve_paths"] == 0
        np.testing.assert_array_equal(r1["iterations"]["cost"], r["iterations"]["cost"])
        for nm in ("cam_pose", "cam_model", "point"):
            np.testing.assert_array_equal(getattr(a1, nm), getattr(a, nm))
