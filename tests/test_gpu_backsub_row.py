"""k_backsub evaluates each row through msfm_backsub_row (ba_device.h: residual, point block and the derivative of the residual
along the step, one forward-mode tangent) with every load of the row issued at once, at four waves per SIMD.
Small scenes - 16 cameras that look along +z, a few hundred points - around every body of the kernel: tracks of 2 and 4 (the
4-lane class forced on), 5 and 8, 9 and 16, 17 and 40 (rounds of 8), and all classes ending part-way through a workgroup.
Every scene holds a camera whose angle-axis vector is exactly zero at the start (the first-order branch), one at |a| = 1e-9
(below the branch threshold) and one at |a| = 1e-6 (just above it), a frozen camera, GPS rows, two intrinsics blocks whose rows
meet in one point - the second frozen in two of the scenes - and gross outlier rows that keep Huber active; one scene starts
so far off that the oracle itself rejects a step (same rows, new radius).  Per scene: parity with the CPU oracle at
check_parity's own tolerances, relative_decrease and cost_change per iteration against the oracle's, two runs bitwise,
host-built structures against device-built ones bitwise, and the same verdict sequence with the fold tables on and off."""
import numpy as np
import pytest

from metricsfm_amd import _abi as A
from metricsfm_amd import scene

from tests.test_gpu_ba import check_parity

pytestmark = pytest.mark.gpu

N_CAMS = 16
FOCAL = 2000.0


def _scene(lengths, seed, sigma=1.0):
    """16 cameras on a 4 x 4 grid at z = -100, all looking along +z at a slab of points.  Camera 0's rotation is the identity,
    camera 1's |a| = 1e-9 and camera 2's 1e-6 - in the ground truth AND at the start, so the first linearisations sit on those
    branches - the others are tilted by a few hundredths.  Point p is seen by lengths[p] cameras, round after round of all 16
    in a random order when there are more rows than cameras (another feature of the same image: its own noise).  One row in
    twenty is a gross outlier.  sigma scales the perturbation of the start."""
    lengths = np.asarray(lengths, np.int64)
    rng = np.random.default_rng(seed)
    n = len(lengths)
    pts = rng.uniform([-40, -40, -10], [40, 40, 10], size=(n, 3))
    centres = np.array([[20.0 * (i % 4) - 30.0, 20.0 * (i // 4) - 30.0, -100.0] for i in range(N_CAMS)])
    aa = rng.uniform(-0.04, 0.04, (N_CAMS, 3))
    aa[0] = 0.0
    aa[1] = 1e-9 * np.array([0.6, 0.0, 0.8])
    aa[2] = 1e-6 * np.array([0.0, -0.8, 0.6])
    poses = np.concatenate([aa, -np.einsum("nij,nj->ni", scene.angle_axis_to_R(aa), centres)], axis=1)
    model = np.array([[FOCAL, -0.05, 0.01], [0.9 * FOCAL, 0.03, 0.0]])
    model_of_cam = (np.arange(N_CAMS) % 2).astype(np.int32)   # neighbouring cameras differ: the rows of a point meet both
    obs_cam = np.concatenate([np.concatenate([rng.permutation(N_CAMS) for _ in range((int(k) + N_CAMS - 1) // N_CAMS)])[:int(k)] for k in lengths]).astype(np.int32)
    obs_pt = np.repeat(np.arange(n, dtype=np.int32), lengths)
    uv, depth = scene.project(poses[obs_cam], model[model_of_cam[obs_cam]], pts[obs_pt])
    assert (depth > 0).all()
    obs_xy = uv + rng.standard_normal(uv.shape) * 0.5
    outlier = rng.random(len(obs_cam)) < 0.05
    obs_xy[outlier] += rng.uniform(-60.0, 60.0, (int(outlier.sum()), 2))
    pose0 = poses.copy()
    pose0[3:, :3] += rng.standard_normal((N_CAMS - 3, 3)) * 0.01 * sigma
    pose0[:, 3:] += rng.standard_normal((N_CAMS, 3)) * 0.2 * sigma
    point0 = pts + rng.standard_normal(pts.shape) * 0.2 * sigma
    model0 = model * (1.0 + 0.002 * sigma * rng.standard_normal(model.shape))
    sc = scene.Scene("backsub_row", poses, model, pts, pose0, model0, point0, model_of_cam, obs_cam, obs_pt, obs_xy, np.ones(n))
    gps = centres + rng.standard_normal((N_CAMS, 3)) * 0.5
    return sc, gps


def _cycle(values, n):
    return [values[i % len(values)] for i in range(n)]


# name, track lengths, second intrinsics block frozen, scale of the start's perturbation, options
_CASES = [
    ("tracks_2_and_4", _cycle([2, 4], 260), False, 1.0, {}),
    ("tracks_5_and_8", _cycle([5, 8], 90), True, 1.0, {}),
    ("tracks_9_and_16", _cycle([9, 16], 60), False, 1.0, {}),
    ("tracks_17_and_40", _cycle([17, 40], 40), True, 1.0, {}),
    # (counted after the masks froze a few: Q 69 - one workgroup and five points - S 34, L 18, X 17) every class ends part-way
    ("all_classes_partly_filled", _cycle([2, 3, 4], 75) + _cycle([5, 8, 7], 36) + _cycle([9, 16], 19) + _cycle([17, 40, 24], 19), False, 1.0, {}),
    # a start the first steps overshoot from: the oracle rejects at least one of them
    ("far_start_rejected_steps", _cycle([2, 5, 9, 17, 4, 8, 16, 40, 3], 150), False, 6.0, {}),
]


def _solve(ctx, arrays, opts):
    from metricsfm_amd import capi
    a = arrays()
    r = ctx.ba_solve(a, capi.default_options(**opts))
    it = r["iterations"]
    return (it["cost"].copy(), it["gradient_max_norm"].copy(), it["relative_decrease"].copy(), it["step_is_successful"].copy(),
            a.cam_pose, a.cam_model, a.point)


def _same(x, y):
    for u, v in zip(x, y):
        np.testing.assert_array_equal(u, v)


@pytest.mark.parametrize("name,lengths,freeze_model,sigma,extra_opts", _CASES, ids=[c[0] for c in _CASES])
def test_backsub_row_form(ctx, oracle, monkeypatch, name, lengths, freeze_model, sigma, extra_opts):
    sc, gps = _scene(lengths, seed=4100 + len(lengths), sigma=sigma)
    rng = np.random.default_rng(17)
    cam_mutable = np.ones(N_CAMS, np.uint8)
    cam_mutable[5] = 0
    kw = dict(cam_mutable=cam_mutable, pt_mutable=(rng.random(len(lengths)) > 0.06).astype(np.uint8),
              model_mutable=np.array([1, 0 if freeze_model else 1], np.uint8), gps_xyz=gps, gps_weight=40.0)
    arrays = lambda: A.BaArrays.from_scene(sc, **kw)
    opts = dict(max_num_iterations=10, **extra_opts)
    monkeypatch.setenv("MSFM_LANES4_MIN", "0")   # (a problem this small would keep its short points in the 8-lane class)
    monkeypatch.setenv("MSFM_FOLD_MIN", "0")     # fold tables on
    lengths = np.asarray(lengths)
    free = kw["pt_mutable"].astype(bool)
    ba = ctx.ba(arrays())
    lay = ba.layout()
    ba.close()
    want = dict(npb_S4=int((free & (lengths <= 4)).sum()), npb_S=int((free & (lengths <= 8)).sum()),
                npb_L=int((free & (lengths > 8) & (lengths <= 16)).sum()), npb_X=int((free & (lengths > 16)).sum()))
    print(name, want)
    assert {k: lay[k] for k in want} == want
    if name == "all_classes_partly_filled":   # no class fills its last workgroup
        assert want["npb_S4"] % 64 and want["npb_S4"] > 64 and (want["npb_S"] - want["npb_S4"]) % 32 and want["npb_L"] % 16 and want["npb_X"] % 32
    r_gpu, r_ref, _ = check_parity(ctx, oracle, arrays, opts)
    ig, ir = r_gpu["iterations"], r_ref["iterations"]
    print("verdicts", ir["step_is_successful"].astype(int).tolist())
    if name == "far_start_rejected_steps":
        assert (ir["step_is_successful"][1:] == 0).any()   # the rejected-step path runs: same rows, new radius
    for k in range(len(ir)):   # the model cost change is where q enters (check_parity_strict's bars)
        for f in ("relative_decrease", "cost_change"):
            print(name, k, f, ig[f][k], ir[f][k])
            assert abs(ig[f][k] - ir[f][k]) <= 1e-5 * abs(ir[f][k]) + 1e-9 * abs(ir["cost"][k]), (f, k, ig[f][k], ir[f][k])
    dev = _solve(ctx, arrays, opts)
    _same(dev, _solve(ctx, arrays, opts))                    # the same problem twice
    monkeypatch.setenv("MSFM_CREATE_HOST", "1")
    _same(dev, _solve(ctx, arrays, opts))                    # host-built structures
    monkeypatch.delenv("MSFM_CREATE_HOST")
    monkeypatch.delenv("MSFM_FOLD_MIN")
    monkeypatch.setenv("MSFM_NO_FOLD", "1")                  # the gather path: another summation order of the reduced system
    gat = _solve(ctx, arrays, opts)
    np.testing.assert_array_equal(gat[3], dev[3])            # the same verdict sequence
