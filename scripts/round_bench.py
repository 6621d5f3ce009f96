"""Timing of the second half of a round (PartialBundleAdjustment + RemovePointOutliers, sfm_incremental.cc:172-186) at
BASELINE config 3, in the shape of scripts/newpoints_bench.py: images 0-249 of the 500 registered, image 250 just localised
(camera 250) with its new points applied - the state holds the 251 registered cameras, every point at least two of them see,
and one observation row per view.  Every camera has its own model (the WEB mode), so the partial stage frees the new camera
and its visible ones (more than 5 shared points) and leaves the rest frozen.  The model is adjusted already: ground-truth
cameras and points with 0.05 units of noise on the points, the new camera perturbed as `scene.perturb_camera` does.

  python scripts/round_bench.py [--reps 9] [--out FILE] [--no-host]

One JSON line each:
  call      one msfm_round_adjust call (partial stage + outliers) through the Python binding, its synchronisations and the fetch
            included: median / min / max of --reps after a warm-up, the bytes it sent to the device, the kernel split of
            msfm_ctx_profile_get from one further call, the solve's own time
  python    what a caller could do without the call: the numpy assembly of the same compact problem (window.partial_ba_masks +
            window.gather on a Scene), ctx.ba_solve, cameras_for_tracks + ctx.reproject_mse on host arrays and the flag update in
            numpy; its parts, and whether problem, solve and flags equal the call's
  host      the same round through the host mirror (tests/round_host_check.cc, -O2): IncrementalSfM::AdjustRound - both sides of
            the flat state gathered from the std::map objects, the call, everything written back - against its object-graph
            path, PartialBundleAdjustment -> RemovePointOutliers; whether the two solves came out bitwise equal"""
import argparse
import json
import os
import socket
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from metricsfm_amd import _abi as A  # noqa: E402
from metricsfm_amd import capi, scene, window  # noqa: E402
from tests import round_data as D  # noqa: E402

N_REGISTERED = 250


def build_round():
    sc = scene.config_scene(3)
    n_cams = N_REGISTERED + 1
    rng = np.random.default_rng(3)
    reg = sc.obs_cam < n_cams
    exists = np.bincount(sc.obs_pt[reg], minlength=sc.n_points) >= 2
    keep = reg & exists[sc.obs_pt]
    new_id = (np.cumsum(exists) - 1).astype(np.int32)
    n_points = int(exists.sum())
    pose = sc.cam_pose_gt[:n_cams].copy()
    sub = scene.Scene("C3-round", pose, np.tile(sc.cam_model_gt[:1], (n_cams, 1)), sc.point_gt[exists], pose.copy(),
                      np.tile(sc.cam_model_gt[:1], (n_cams, 1)), sc.point_gt[exists] + rng.normal(0, 0.05, (n_points, 3)),
                      np.arange(n_cams, dtype=np.int32), sc.obs_cam[keep], new_id[sc.obs_pt[keep]],
                      sc.obs_xy[keep].astype(np.float32).astype(np.float64), np.ones(n_points))
    scene.perturb_camera(sub, N_REGISTERED)
    st = D.scene_state(sub)
    st["pt_new_added"] = (np.bincount(sub.obs_pt[sub.obs_cam == N_REGISTERED], minlength=n_points) > 0).astype(np.uint8)
    st["new_cam"] = N_REGISTERED
    st["visible"] = window.visible_cameras(sub.obs_cam, sub.obs_pt, n_cams, N_REGISTERED)
    return sub, st


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def stats(ts):
    return dict(wall_ms=round(float(np.median(ts)), 3), wall_ms_min=round(min(ts), 3), wall_ms_max=round(max(ts), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    sub, c = build_round()
    box = socket.gethostname()
    ctx = capi.Context(0)
    st = ctx.match_store(*D.store_args(c))
    call = lambda **kw: ctx.round_adjust(st, *D.call_args(c), pt_new_added=c["pt_new_added"], new_cam=c["new_cam"], visible=c["visible"],  # noqa: E731
                                         keypoints=c["keypoints"], partial=True, full=False, outliers=True, **kw)
    r = call(keep_problem=1)
    q = r["problem"][0]
    shape = dict(box=box, cameras=len(c["cam_img"]), points=len(c["pt_bad"]), rows=len(c["obs_point"]), visible=len(c["visible"]),
                 free_cameras=int(r["adjust_cams"][0]), free_points=int(r["adjust_pts"][0]), problem_points=len(q["kept"]), problem_rows=len(q["obs_cam"]),
                 iterations=int(r["summary"][0]["num_iterations"]), outliers=r["count_outliers"])
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        r = call()
        ts.append((time.perf_counter() - t0) * 1e3)
    ctx.profile(True); ctx.profile_reset()
    call()
    prof = ctx.profile_get()
    ctx.profile(False)
    emit(dict(what="round", part="call", reps=a.reps, h2d_bytes=int(r["h2d_bytes"]), solve_ms=round(r["summary"][0]["solve_ms"], 3),
              ba_setup_ms=round(r["summary"][0]["setup_ms"], 3), kernels_ms={k: round(v["total_ms"], 3) for k, v in prof.items()}, **stats(ts), **shape), a.out)

    # what a caller could do without the call
    def python_path():
        lap = [time.perf_counter()]
        cam_mut, pt_mut = window.partial_ba_masks(sub.obs_cam, sub.obs_pt, sub.n_cams, sub.n_points, sub.cam_model_of_cam, c["new_cam"], c["visible"], None)
        arr, kept = window.gather(sub, cam_mut, pt_mut, window.PARTIAL_WEIGHT, None, False, True)
        lap.append(time.perf_counter())
        s = ctx.ba_solve(arr, capi.default_options(max_num_iterations=100))
        lap.append(time.perf_counter())
        xyz = sub.point.copy()
        xyz[kept] = arr.point
        R, t, cc, fk = scene.cameras_for_tracks(sub, pose=arr.cam_pose, model=arr.cam_model)
        tr = A.TrackArrays(sub.track_offsets(), sub.obs_cam, sub.obs_xy, R, t, cc, fk)
        mse = ctx.reproject_mse(tr, xyz)
        bad = np.sqrt(mse) > 1.0
        added = np.zeros(sub.n_points, np.uint8)
        lap.append(time.perf_counter())
        return np.diff(lap) * 1e3, arr, kept, s, xyz, mse, bad, added
    python_path()
    laps = np.array([python_path()[0] for _ in range(a.reps)])
    _, arr, kept, s, xyz, mse, bad, _ = python_path()
    same_problem = bool(np.array_equal(kept, q["kept"]) and np.array_equal(arr.obs_cam, q["obs_cam"]) and np.array_equal(arr.obs_pt, q["obs_pt"])
                        and np.array_equal(arr.obs_xy, q["obs_xy"]) and np.array_equal(arr.pt_weight, q["pt_weight"]))
    emit(dict(what="round", part="python", reps=a.reps, box=box, assemble_ms=round(float(np.median(laps[:, 0])), 3),
              ba_solve_ms=round(float(np.median(laps[:, 1])), 3), outliers_ms=round(float(np.median(laps[:, 2])), 3),
              same_problem=same_problem, same_solve=bool(np.array_equal(xyz, r["point_xyz"]) and np.array_equal(arr.cam_pose, r["cam_pose"])),
              same_flags=bool(np.array_equal(bad.astype(np.uint8), r["pt_bad"])), max_abs_dmse=float(np.nanmax(np.abs(mse - r["pt_mse"]))),
              **stats(laps.sum(axis=1))), a.out)
    st.close(); ctx.close()
    if a.no_host:
        return
    with tempfile.TemporaryDirectory() as tmp:
        exe, src, dst = (os.path.join(tmp, x) for x in ("round_host_check", "in.bin", "out.bin"))
        subprocess.check_call(D.host_check_command(exe))
        D.write_model(src, c)
        run = subprocess.run([exe, src, dst, "time"], capture_output=True, text=True, timeout=900)
        if run.returncode != 0:
            raise RuntimeError(run.stdout + run.stderr)
        word = [ln for ln in run.stdout.splitlines() if ln.startswith("time_ms")][0].split()
        got = D.read_host_result(dst, c)
        emit(dict(what="round", part="host", box=box, reps=9, adjust_round_ms=float(word[2]), object_graph_ms=float(word[4]),
                  solve_bitwise_equal="solve bitwise equal: yes" in run.stdout,
                  equals_python_call=bool(np.array_equal(got["point_xyz"], r["point_xyz"]) and np.array_equal(got["cam_pose"], r["cam_pose"])
                                          and np.array_equal(got["pt_bad"], r["pt_bad"]))), a.out)


if __name__ == "__main__":
    main()
