"""Two small launches of the LM step ride with launches of the factor-and-solve (metricsfm_amd/csrc/solve_riders.h): the body of
k_modelsum runs as extra workgroups of the level-0 corner update, and the arithmetic of k_update_params runs in
k_backsolve_chain behind the publication of each block, its two block sums in the first workgroups of k_backsub.
MSFM_SOLVE_RIDERS=0 keeps both as launches of their own.  No operand, order of additions or grouping of partial sums changes,
so both forms must give every iteration's scalars and the three parameter arrays to the last bit; msfm_ba_layout.rider_paths
says which form the last solve took.

Scenes: 151 aerial cameras (the camera graph is dissected from 128 on) and 2500 points, the camera count picked with
msfm_camera_graph_dissection on the CPU so that the part of the system behind the leaves is, with one bisection
(MSFM_CHOL_DOMAINS=1), a root of four 64-column blocks and, with two (MSFM_CHOL_DOMAINS=2), separators of one block and of two
blocks below that root - seven blocks, an odd count: the layout is asserted.  Every case runs 4 LM iterations with the stopping rules off and the fold tables forced
on (MSFM_FOLD_MIN=0), so that the reduced system is assembled beside the per-camera sums, and is compared with the CPU oracle
at check_parity's tolerances (cost 1e-9, parameters 1e-7, radius 1e-6, |gradient|_max and |step| 1e-5).  The oracle's runs are
computed once per scene and shared.

The 128 x 64 tile form of the corner update that was specified together with the riders was not built, so
there is no MSFM_CORNER_MACRO switch to compare against here."""
import numpy as np
import pytest

from metricsfm_amd import _abi as A
from metricsfm_amd import capi, scene

from tests.ba_step_check import NO_STOP

N_CAMS, N_POINTS, SEED = 151, 2500, 7
MODEL, UPDATE = A.MSFM_PATH_RIDER_MODELSUM, A.MSFM_PATH_RIDER_UPDATE
KEYS = ("cost", "cost_change", "gradient_max_norm", "trust_region_radius", "step_is_successful", "step_is_valid", "step_norm", "relative_decrease")
MILD = dict(rot_sigma=0.02, trans_sigma=0.2, point_sigma=0.2)
FROZEN = [3, 40, 77, 101]

_SCENES, _REF = {}, {}


def _case(name):
    """(scene, keyword arguments of BaArrays.from_scene, MSFM_CHOL_DOMAINS or None, solver options)."""
    if name not in _SCENES:
        opts, kw, domains = {}, {}, "1"
        if name in ("domains1", "domains2", "dense_order", "no_solve"):
            sc = scene.make_aerial_scene(N_CAMS, N_POINTS, seed=SEED, **MILD)
            domains = {"domains2": "2", "dense_order": "0"}.get(name, "1")
            if name == "no_solve":
                opts = dict(max_num_iterations=0)
        elif name == "rejected_step":
            # twelve cameras frozen at perturbed poses: the oracle accepts two steps and rejects the next two (rho = -0.82, -0.96).
            # Condition on the input, from the oracle's rows alone (asserted in the test before the GPU's are looked at): every
            # rho at least 0.05 away from min_relative_decrease, and no row's cost above ten times the initial cost.  The two
            # solvers' steps agree to check_parity's 1e-5 only; the cost of a candidate far outside the region the model holds
            # in (a first pick with four frozen cameras at twice the perturbation put a rejected candidate at 1e5 times the
            # cost of x) follows the step, not the 1e-9 bar of a cost near the iterate.
            sc = scene.make_aerial_scene(N_CAMS, N_POINTS, seed=SEED, rot_sigma=0.14, trans_sigma=0.7, point_sigma=0.7)
            kw = dict(cam_mutable=_mask(N_CAMS, list(range(3, 63, 5))))
        elif name == "frozen_camera":
            sc = scene.make_aerial_scene(N_CAMS, N_POINTS, seed=SEED, **MILD)
            kw = dict(cam_mutable=_mask(N_CAMS, FROZEN))
        elif name == "gps_rows":
            sc = scene.make_aerial_scene(N_CAMS, N_POINTS, seed=SEED, gps_sigma=0.5, **MILD)
            kw = dict(gps_xyz=sc.gps_xyz, gps_weight=40.0)
        elif name == "two_intrinsics":   # the intrinsics x camera products stay on the gather path: no assembly beside, k_modelsum launched
            sc = scene.make_aerial_scene(N_CAMS, N_POINTS, seed=SEED, n_models=2, **MILD)
        elif name == "few_points":       # 783 reduced parameters = 4 blocks of 256, 40 eliminated points = fewer point workgroups than that
            sc = scene.make_ring_scene(130, 40, seed=5, **MILD)
            domains = None
        else:
            raise KeyError(name)
        _SCENES[name] = (sc, kw, domains, dict(dict(max_num_iterations=4, **NO_STOP), **opts))
    return _SCENES[name]


def _mask(n, off):
    m = np.ones(n, np.uint8)
    m[off] = 0
    return m


def _arrays(name):
    sc, kw, _, _ = _case(name)
    return A.BaArrays.from_scene(sc, **kw)


def _reference(oracle, name):
    """The oracle's run of a case: computed once, shared, never written to again."""
    if name not in _REF:
        a = _arrays(name)
        r = oracle.ba_solve(a, oracle.default_options(**_case(name)[3]))
        for x in (a.cam_pose, a.cam_model, a.point, r["iterations"]):
            x.setflags(write=False)
        _REF[name] = (r, a)
    return _REF[name]


def _run(monkeypatch, name, riders=True, env=None):
    """One run of the case on a resident problem in a fresh context: summary, parameters, layout."""
    _, _, domains, opts = _case(name)
    env = dict(env or {}, MSFM_FOLD_MIN="0")
    if domains is not None:
        env["MSFM_CHOL_DOMAINS"] = domains
    if not riders:
        env["MSFM_SOLVE_RIDERS"] = "0"
    for k in ("MSFM_SOLVE_RIDERS", "MSFM_CHOL_DOMAINS", "MSFM_CHOL_LAUNCHES", "MSFM_ASM_BESIDE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = capi.Context(0)
    try:
        ba = c.ba(_arrays(name))
        r = ba.run(capi.default_options(**opts))
        out = (r, ba.download(), ba.layout())
        ba.close()
    finally:
        c.close()
        for k in env:
            monkeypatch.delenv(k)
    return out


def _same(x, y):
    assert x[0]["termination"] == y[0]["termination"] and x[0]["num_iterations"] == y[0]["num_iterations"]
    for key in KEYS:
        np.testing.assert_array_equal(x[0]["iterations"][key], y[0]["iterations"][key], err_msg=key)
    for u, v in zip(x[1], y[1]):
        np.testing.assert_array_equal(u, v)


def _rel(x, y):
    return float(np.abs(x - y).max() / max(np.abs(y).max(), 1e-300))


def _parity(run, ref):
    """check_parity (tests/test_gpu_ba.py) on two finished solves."""
    (r_gpu, params, _), (r_ref, a_ref) = run, ref
    assert r_gpu["num_residuals"] == r_ref["num_residuals"] and r_gpu["num_reduced_params"] == r_ref["num_reduced_params"]
    assert r_gpu["termination"] == r_ref["termination"] and r_gpu["num_iterations"] == r_ref["num_iterations"]
    ig, ir = r_gpu["iterations"], r_ref["iterations"]
    dev = [_rel(p, getattr(a_ref, n)) for p, n in zip(params, ("cam_pose", "cam_model", "point"))]
    print("GPU vs oracle: cost %.2e (bar 1e-9), parameters %.2e (bar 1e-7)" % (float((np.abs(ig["cost"] - ir["cost"]) / ir["cost"]).max()), max(dev)))
    np.testing.assert_array_equal(ig["step_is_successful"], ir["step_is_successful"])
    np.testing.assert_array_equal(ig["step_is_valid"], ir["step_is_valid"])
    np.testing.assert_allclose(ig["cost"], ir["cost"], rtol=1e-9)
    np.testing.assert_allclose(ig["trust_region_radius"], ir["trust_region_radius"], rtol=1e-6)
    np.testing.assert_allclose(ig["gradient_max_norm"], ir["gradient_max_norm"], rtol=1e-5, atol=1e-9)
    np.testing.assert_allclose(ig["step_norm"], ir["step_norm"], rtol=1e-5, atol=1e-12)
    assert abs(r_gpu["final_cost"] - r_ref["final_cost"]) <= 1e-9 * abs(r_ref["final_cost"])
    assert max(dev) < 1e-7, dev


def _sep_blocks(lay):
    """64-column blocks of every level behind the leaves, then of the root (with the rhs row)."""
    begin = lay["level_begin"] + [lay["system_order"] - lay["root_cols"]]
    return [(begin[l + 1] - begin[l]) // 64 for l in range(1, lay["n_levels"])] + [-(-(lay["root_cols"] + 1) // 64)]


def test_the_camera_count_gives_the_intended_trees():
    """On the CPU: one bisection leaves a root of 34 cameras, two leave separators of 10 and 14 cameras below it."""
    sc = _case("domains1")[0]
    inc = np.zeros((sc.n_points, sc.n_cams), np.int32)
    inc[sc.obs_pt, sc.obs_cam] = 1
    adj = (inc.T @ inc) > 0
    np.fill_diagonal(adj, False)
    label, n_leaves, _ = capi.camera_graph_dissection(adj.astype(np.uint8), tail_cols=4, force_depth=1)
    assert n_leaves == 2 and int((label == -1).sum()) == 34
    label, n_leaves, _ = capi.camera_graph_dissection(adj.astype(np.uint8), tail_cols=4, force_depth=2)
    assert n_leaves == 4 and int((label == -1).sum()) == 34 and int((label == -2).sum()) == 24


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["domains1", "domains2", "rejected_step", "frozen_camera", "gps_rows"])
def test_riders_are_bit_identical_to_the_launches_of_their_own(monkeypatch, oracle, name):
    ref_rows = _reference(oracle, name)[0]["iterations"]
    if name == "rejected_step":   # the condition on the input (see _case), from the oracle alone
        rho = ref_rows["relative_decrease"][1:]
        assert (ref_rows["step_is_successful"][1:] == 0).sum() >= 1 and (ref_rows["step_is_successful"][1:] == 1).sum() >= 1
        assert np.abs(rho - 1e-3).min() >= 0.05 and ref_rows["cost"].max() <= 10.0 * ref_rows["cost"][0], (rho, ref_rows["cost"])
    new = _run(monkeypatch, name)
    old = _run(monkeypatch, name, riders=False)
    lay = new[2]
    assert lay["assemble_paths"] == A.MSFM_PATH_ASM_BESIDE and lay["solve_paths"] & A.MSFM_PATH_BACKSOLVE_CHAIN
    assert lay["rider_paths"] == MODEL | UPDATE and old[2]["rider_paths"] == 0
    assert old[2]["assemble_paths"] == lay["assemble_paths"] and old[2]["solve_paths"] == lay["solve_paths"]
    if name == "domains1":      # 2 leaves | root of 34 cameras + intrinsics + rhs = 4 blocks
        assert lay["n_levels"] == 1 and lay["level_nodes"] == [2] and _sep_blocks(lay) == [4]
    if name == "domains2":      # 4 leaves | separators of 10 and 14 cameras = 1 + 2 blocks | root of 4 blocks
        assert lay["n_levels"] == 2 and lay["level_nodes"] == [4, 2] and _sep_blocks(lay) == [3, 4]
    ok = new[0]["iterations"]["step_is_successful"]
    assert (ok[1:] == 0).any() == (name == "rejected_step"), ok
    _same(new, old)
    _parity(new, _reference(oracle, name))


@pytest.mark.gpu
def test_riders_with_one_launch_per_panel(monkeypatch):
    """MSFM_CHOL_LAUNCHES=1: the model sums still ride with the level-0 corner update; the back substitution is a chain of
    launches, so k_update_params stays."""
    new = _run(monkeypatch, "domains2", env=dict(MSFM_CHOL_LAUNCHES="1"))
    old = _run(monkeypatch, "domains2", riders=False, env=dict(MSFM_CHOL_LAUNCHES="1"))
    assert new[2]["solve_paths"] == 0 and new[2]["rider_paths"] == MODEL and old[2]["rider_paths"] == 0
    _same(new, old)
    _same(new, _run(monkeypatch, "domains2"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["two_intrinsics", "dense_order", "no_solve", "few_points"])
def test_where_a_rider_must_not_run(monkeypatch, oracle, name):
    new = _run(monkeypatch, name)
    lay = new[2]
    if name == "two_intrinsics":
        assert lay["assemble_paths"] == 0 and lay["n_levels"] == 1 and lay["rider_paths"] == UPDATE
    elif name == "dense_order":
        assert lay["assemble_paths"] == A.MSFM_PATH_ASM_BESIDE and lay["n_levels"] == 0 and lay["rider_paths"] == UPDATE
    elif name == "no_solve":     # max_num_iterations reached at once: no solve follows the assembly
        assert lay["assemble_paths"] == A.MSFM_PATH_ASM_BESIDE and lay["n_levels"] == 1 and lay["rider_paths"] == 0 and lay["solve_paths"] == 0
    else:                        # fewer point workgroups than blocks of 256 reduced parameters: the separate k_update_params
        assert lay["reduced_order"] == 6 * 130 + 3 and lay["npb_S"] + lay["npb_L"] + lay["npb_X"] == 40
        assert lay["solve_paths"] & A.MSFM_PATH_BACKSOLVE_CHAIN and lay["rider_paths"] == 0
    _same(new, _run(monkeypatch, name, riders=False))
    _parity(new, _reference(oracle, name))
