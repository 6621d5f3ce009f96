"""Timing of one GenerateNew3DPoints round (sfm_incremental.cc:755-915) at BASELINE config 3, in the shape of
scripts/localize_bench.py: 500 images, the matches of `flat_matches_from_scene`, images 0-249 registered, image 250 just
localised (camera 250).  A point exists when at least two registered images see it and a seeded draw keeps it (70 %: the rest
stands for points earlier rounds rejected or have not reached); the new camera holds the existing points it sees, and its
visible list is what IncrementalSfM::VisibleCameras gives it: the cameras through which it has more than 5 2D-3D matches.

  python scripts/newpoints_bench.py [--reps 9] [--out FILE] [--no-host] [--calls-only N]

One JSON line each:
  call      one msfm_new_points call through the Python binding, its synchronisation and fetch included: median / min / max of
            --reps after a warm-up, the bytes it sent to the device, and the kernel split of msfm_ctx_profile_get from one further call
  python    metricsfm_amd/tracks.py::generate_new_points fed from host match arrays (the per-match Python loop, numpy gathers,
            up to two msfm_triangulate_midpoint_batch calls): the path the project had
  host      the same round through the host mirror (tests/newpoints_host_check.cc, -O2): its library call, gathering the flat
            state from the std::map objects included, and GenerateNew3DPointsHost, the reference's walk with one Trianglate2
            (one library call) per candidate
--calls-only N: build the round, create the store, make N calls and exit (the program to put behind
`rocprofv3 --kernel-trace --stats --`)."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from metricsfm_amd import capi, scene, tracks  # noqa: E402
from metricsfm_amd.tracks import flat_matches_from_scene  # noqa: E402
from tests import newpoints_data as D  # noqa: E402

N_REGISTERED = 250
TH_VISIBLE = 5


def build_round():
    sc = scene.config_scene(3)
    nf, pairs, moff, m = flat_matches_from_scene(sc)
    rng = np.random.default_rng(3)
    n_cams = N_REGISTERED + 1
    new = N_REGISTERED
    by_cam = np.argsort(sc.obs_cam, kind="stable")                 # feature f of image c = its f-th observation
    start = np.concatenate([[0], np.cumsum(nf)])
    seen = np.bincount(sc.obs_pt[sc.obs_cam < N_REGISTERED], minlength=sc.n_points)
    exists = (seen >= 2) & (rng.random(sc.n_points) < 0.7)
    pid = sc.obs_pt[by_cam][:start[n_cams]].astype(np.int32)
    feat_point = np.where(exists[pid], pid, -1).astype(np.int32)
    # VisibleCameras: row `new` of the store, matches whose feature in the registered image holds a point
    visible = []
    lo, hi = np.searchsorted(pairs[:, 0], [new, new + 1])
    for p in range(lo, hi):
        j = int(pairs[p, 1])
        if j < N_REGISTERED and int((feat_point[start[j] + m[moff[p]:moff[p + 1], 1]] >= 0).sum()) > TH_VISIBLE:
            visible.append(j)
    R, t, cc, fk = scene.cameras_for_tracks(sc)
    c = dict(n_features=nf, pairs=pairs, match_off=moff, matches=m, keypoints=sc.obs_xy[by_cam].astype(np.float32),
             cam_img=np.arange(n_cams, dtype=np.int32), feat_point=feat_point, n_points=np.int32(sc.n_points), cam_R=R[:n_cams], cam_t=t[:n_cams],
             cam_c=cc[:n_cams], cam_fk=fk[:n_cams], new_cam=np.array([new], np.int32), vis_off=np.array([0, len(visible)], np.int32),
             vis_cam=np.array(visible, np.int32))
    return c


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--calls-only", type=int, default=0)
    a = ap.parse_args()
    c = build_round()
    ctx = capi.Context(0)
    st = ctx.match_store(*D.store_args(c))
    call = lambda: ctx.new_points(st, *D.call_args(c), keypoints=c["keypoints"])  # noqa: E731
    if a.calls_only:
        for _ in range(a.calls_only):
            call()
        st.close(); ctx.close()
        return
    r = call()
    shape = dict(images=len(c["n_features"]), registered=N_REGISTERED, matches=int(c["match_off"][-1]), visible=len(c["vis_cam"]),
                 walked_matches=int(r["n_matches"].sum()), candidates=int(r["n_candidates"].sum()), new_points=len(r["mse"]),
                 large_entries=int(r["large"].sum()))
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        r = call()
        ts.append((time.perf_counter() - t0) * 1e3)
    ctx.profile(True); ctx.profile_reset()
    call()
    prof = ctx.profile_get()
    ctx.profile(False)
    emit(dict(what="newpoints", part="call", wall_ms=round(float(np.median(ts)), 3), wall_ms_min=round(min(ts), 3), wall_ms_max=round(max(ts), 3),
              reps=a.reps, h2d_bytes=int(r["h2d_bytes"]), kernels_ms={k: round(v["total_ms"], 3) for k, v in prof.items()} if isinstance(prof, dict) else prof,
              **shape), a.out)
    # (a) the path the project had: the matches pulled out to host arrays are its input, so slicing them is not timed
    legacy = D.legacy_args(c, 0)
    old = tracks.generate_new_points(ctx, *legacy)
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        old = tracks.generate_new_points(ctx, *legacy)
        ts.append((time.perf_counter() - t0) * 1e3)
    # same points in the same order; X within 1e-9 of its own length (the older call triangulates with fused multiply-adds)
    same = bool(np.array_equal(old[2], r["cam2"]) and np.array_equal(old[3], r["feat1"]) and np.array_equal(old[4], r["feat2"]))
    dev = float((np.linalg.norm(old[0] - r["X"], axis=1) / np.linalg.norm(r["X"], axis=1)).max()) if same and len(r["mse"]) else None
    emit(dict(what="newpoints", part="python", wall_ms=round(float(np.median(ts)), 3), wall_ms_min=round(min(ts), 3), wall_ms_max=round(max(ts), 3),
              reps=a.reps, same_points_and_order=same, n_points=len(old[1]), max_rel_dX=dev), a.out)
    st.close(); ctx.close()
    if a.no_host:
        return
    with tempfile.TemporaryDirectory() as tmp:
        exe, src, dst = (os.path.join(tmp, x) for x in ("newpoints_host_check", "in.bin", "out.bin"))
        subprocess.check_call(D.host_check_command(exe))
        D.write_model(src, c)
        run = subprocess.run([exe, src, dst, "time"], capture_output=True, text=True, timeout=900)
        if run.returncode != 0:
            raise RuntimeError(run.stdout + run.stderr)
        word = [ln for ln in run.stdout.splitlines() if ln.startswith("time_ms")][0].split()
        got = D.read_host_result(dst, c)
        emit(dict(what="newpoints", part="host", library_call_ms=float(word[2]), walk_one_call_per_candidate_ms=float(word[4]), reps=9,
                  equals_python_call=bool(np.array_equal(got["X"], r["X"]) and np.array_equal(got["cam2"], r["cam2"]))), a.out)


if __name__ == "__main__":
    main()
