"""The fold partials of the reduced system are summed into M by workgroups of the per-camera sums' launch (k_sums), the blocks
finished by k_camftf / k_modelsum, M zeroed for the next assembly behind the solve (k_tail) and the assembly's two sums taken by
the step's last k_reduce (ba.hip, FoldSumArgs).  MSFM_ASM_BESIDE=0 keeps the order before it - per-camera sums, k_reduce, then
k_asm_all.  No sum is reordered, so both orders must give the same trajectory and parameters to the last bit: small scenes whose
lists are short (one 18-lane group per block), long (one camera in every point workgroup: the list shared by three groups, every
loop of it) and mixed in one wave, frozen blocks with GPS rows, rejected and invalid steps (the "M is zeroed" flag), a resident
problem run twice, and the problems that must keep the old order."""
import numpy as np
import pytest

from metricsfm_amd import _abi as A
from metricsfm_amd import capi, scene

from tests.test_gpu_ba import check_parity

pytestmark = pytest.mark.gpu

N_CAMS = 12
BESIDE = A.MSFM_PATH_ASM_BESIDE
KEYS = ("cost", "gradient_max_norm", "trust_region_radius", "step_is_successful", "step_is_valid", "step_norm", "relative_decrease")


def _scene(n_points, seed, wide=0, **kw):
    """A ring scene thinned to track lengths 2..10 in turn; camera 0 also sees the first `wide` points."""
    lengths = np.array([2 + p % 9 for p in range(n_points)])
    kw = dict(dict(rot_sigma=0.02, trans_sigma=0.2, point_sigma=0.2), **kw)
    sc = scene.make_ring_scene(N_CAMS, n_points, seed=seed, **kw)
    rng = np.random.default_rng(seed)
    keep = np.zeros((n_points, N_CAMS), bool)
    for p, k in enumerate(lengths):
        keep[p, rng.choice(N_CAMS, int(k), replace=False)] = True
    keep[:wide, 0] = True
    keep = keep.reshape(-1)   # (the ring scene's observations are point-major with the cameras in order)
    sc.obs_cam, sc.obs_pt, sc.obs_xy = sc.obs_cam[keep], sc.obs_pt[keep], sc.obs_xy[keep]
    assert np.bincount(sc.obs_pt, minlength=n_points).max() <= 11   # (tracks of up to 16 rows fold: every entry leaves the gather lists)
    return sc


def _masks_gps(sc, seed=9):
    rng = np.random.default_rng(seed)
    cam_mut = np.ones(N_CAMS, np.uint8); cam_mut[[1, 5, 9]] = 0
    pt_mut = np.ones(sc.n_points, np.uint8); pt_mut[rng.choice(sc.n_points, 40, replace=False)] = 0
    gps = sc.cam_pose_gt[:, 3:] + rng.standard_normal((N_CAMS, 3)) * 0.5
    return dict(cam_mutable=cam_mut, pt_mutable=pt_mut, gps_xyz=gps, gps_weight=40.0)


def _run(monkeypatch, arrays, opts, beside, runs=1, env=None, upload_between=False):
    """`runs` runs of a resident problem in a fresh context: per run the iteration rows, then the parameters and the layout."""
    monkeypatch.setenv("MSFM_FOLD_MIN", "0")
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    if beside:
        monkeypatch.delenv("MSFM_ASM_BESIDE", raising=False)
    else:
        monkeypatch.setenv("MSFM_ASM_BESIDE", "0")
    c = capi.Context(0)
    try:
        a = arrays()
        ba = c.ba(a)
        rows = []
        for k in range(runs):
            if k and upload_between:
                ba.upload(a.cam_pose, a.cam_model, a.point)
            r = ba.run(capi.default_options(**(opts[k] if isinstance(opts, list) else opts)))
            rows.append((r["termination"], {key: r["iterations"][key].copy() for key in KEYS}))
        out = (rows, ba.download(), ba.layout())
        ba.close()
    finally:
        c.close()
        for k in (env or {}):
            monkeypatch.delenv(k)
    return out


def _same(x, y):
    assert len(x[0]) == len(y[0])
    for (tx, rx), (ty, ry) in zip(x[0], y[0]):
        assert tx == ty
        for key in KEYS:
            np.testing.assert_array_equal(rx[key], ry[key], err_msg=key)
    for u, v in zip(x[1], y[1]):
        np.testing.assert_array_equal(u, v)


def _both(monkeypatch, arrays, opts, taken=True, **kw):
    new = _run(monkeypatch, arrays, opts, True, **kw)
    old = _run(monkeypatch, arrays, opts, False, **kw)
    assert new[2]["assemble_paths"] == (BESIDE if taken else 0) and old[2]["assemble_paths"] == 0
    _same(new, old)
    return new


def _case(name):
    if name == "short_lists":          # 300 points: at most 14 point workgroups, so every list is short
        sc = _scene(300, 41)
        return sc, {}
    if name == "one_long_camera":      # camera 0 sees 1500 of 1600 points: a partial from (nearly) every point workgroup, > 48
        sc = _scene(1600, 42, wide=1500)
        return sc, {}
    if name == "frozen_and_gps":
        sc = _scene(300, 41)
        return sc, _masks_gps(sc)
    if name == "two_intrinsics":       # the intrinsics x camera products stay on the gather path: the order before
        sc = _scene(300, 41)
        sc.cam_model = np.tile(sc.cam_model, (2, 1))
        sc.cam_model_of_cam = (np.arange(N_CAMS) % 2).astype(np.int32)
        return sc, {}
    raise KeyError(name)


@pytest.mark.parametrize("name", ["short_lists", "one_long_camera", "frozen_and_gps", "two_intrinsics"])
def test_asm_beside_is_bit_identical_to_the_order_before(monkeypatch, name):
    sc, kw = _case(name)
    new = _both(monkeypatch, lambda: A.BaArrays.from_scene(sc, **kw), dict(max_num_iterations=8), taken=name != "two_intrinsics")
    lay = new[2]
    if name != "two_intrinsics":
        assert lay["fold"]["cc_entries_folded"] == lay["fold"]["cc_entries"] and lay["fold"]["mc_entries_folded"] == lay["fold"]["mc_entries"]
    if name == "one_long_camera":
        assert lay["npb_S"] // 32 + lay["npb_L"] // 16 >= 48   # full point workgroups, each with a row of camera 0 (1500 of 1600 points)
    assert (new[0][0][1]["step_is_successful"][1:] == 1).sum() >= 3


def test_asm_beside_run_equals_run(monkeypatch):
    sc, kw = _case("short_lists")
    arrays = lambda: A.BaArrays.from_scene(sc, **kw)
    _same(_run(monkeypatch, arrays, dict(max_num_iterations=8), True), _run(monkeypatch, arrays, dict(max_num_iterations=8), True))


def test_asm_beside_matches_the_oracle(ctx, oracle, monkeypatch):
    sc, kw = _case("frozen_and_gps")
    monkeypatch.setenv("MSFM_FOLD_MIN", "0")
    arrays = lambda: A.BaArrays.from_scene(sc, **kw)
    ba = ctx.ba(arrays())
    ba.run(capi.default_options(max_num_iterations=1))
    assert ba.layout()["assemble_paths"] == BESIDE
    ba.close()
    check_parity(ctx, oracle, arrays, dict(max_num_iterations=10))


def test_asm_beside_rejected_and_invalid_steps(monkeypatch):
    """The second assembly without an accepted step finds M zeroed by the k_tail of the rejected one; a 3 x 3 point block that
    cannot be factored makes every step invalid, and each of them is followed by an assembly again."""
    sc = _scene(300, 43, rot_sigma=0.3, trans_sigma=2.0, point_sigma=2.0)
    kw = _masks_gps(sc)
    kw.pop("gps_xyz"); kw.pop("gps_weight")    # frozen cameras left at perturbed poses: steps that do not pay
    new = _both(monkeypatch, lambda: A.BaArrays.from_scene(sc, **kw), dict(max_num_iterations=14))
    ok = new[0][0][1]["step_is_successful"][1:]
    assert (ok == 0).sum() >= 2 and (ok == 1).sum() >= 2, ok
    # a point whose rows all have weight 0, and no LM diagonal to stand in for them
    sc2 = _scene(300, 41)
    sc2.pt_weight = np.ones(sc2.n_points); sc2.pt_weight[::7] = 0.0
    new = _both(monkeypatch, lambda: A.BaArrays.from_scene(sc2), dict(max_num_iterations=14, max_lm_diagonal=0.0))
    term, rows = new[0][0]
    assert (rows["step_is_valid"][1:] == 0).sum() >= 1, rows["step_is_valid"]


def test_asm_beside_resident_runs_and_the_assembly_without_a_solve(monkeypatch):
    sc, kw = _case("frozen_and_gps")
    arrays = lambda: A.BaArrays.from_scene(sc, **kw)
    # twice on one resident problem, the start uploaded again in between; then 0 and 1 iterations (the last assembly of a run
    # has no solve behind it: its sums are reduced at once and nothing zeroes M for the next run)
    _both(monkeypatch, arrays, [dict(max_num_iterations=5), dict(max_num_iterations=5)], runs=2, upload_between=True)
    _both(monkeypatch, arrays, [dict(max_num_iterations=0), dict(max_num_iterations=1), dict(max_num_iterations=3)], runs=3)
