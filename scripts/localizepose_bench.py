"""Timing of the localisation tries of one round (IncrementalSfM::Run, sfm_incremental.cc:143-164, around LocalizeImage, :565-753)
on the round of scripts/localize_bench.py: BASELINE config 3, 500 images, images 0-249 registered, the true focal length.

  python scripts/localizepose_bench.py [--reps 9] [--out FILE] [--no-host]

One JSON line each; wall times are the median / min / max of --reps after a warm-up, search included, from the call to the answer
on the host:
  resident   msfm_localize_candidates with the points kept on the device + msfm_localize_poses: known focal length with
             max_tries 16 and 0 (every row), the sweep arm (default options) with max_tries 1 and 16; for the first the kernel
             split of msfm_ctx_profile_get from one further call
  roundtrip  what a caller had before msfm_localize_poses, on the same inputs: localize_candidates with the points (fetched to
             the host), epnp_ransac on the fetched arrays (uploaded again), the rules of :708-729 for the winner in numpy - for
             the first 16 rows and for every row
  host       the host mirror (tests/localizepose_host_check.cc, -O2): LocalizeNextImage against its LocalizeImage walk
Every variant must name the same winner as the first resident call."""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import localize_bench as LB  # noqa: E402
from metricsfm_amd import capi, scene  # noqa: E402
from tests import localize_data as D  # noqa: E402
from tests import localizepose_data as PD  # noqa: E402

TH_MSE, TH_MIN = 5.0, 20


def numpy_rules(err, avg, points, added):
    """:709-729 for one row: the states msfm_localize_poses reports."""
    state = np.where(err > avg, 1, 3).astype(np.uint8)
    free = np.nonzero((state == 3) & (added[points] == 0))[0]
    _, first = np.unique(points[free], return_index=True)
    state[free[first]] = 2
    return state


def timed(fn, reps):
    out = fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, dict(wall_ms=round(float(np.median(ts)), 3), wall_ms_min=round(min(ts), 3), wall_ms_max=round(max(ts), 3), reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    c = LB.build_round()
    n_pts = len(c["pt_bad"])
    f = float(scene.FOCAL)
    added = np.zeros(n_pts, np.uint8)
    ctx = capi.Context(0)
    st = ctx.match_store(*D.store_args(c))
    search = dict(point_xyz=c["point_xyz"], keypoints=c["keypoints"])

    def resident(row_f, **opts):
        s = ctx.localize_set(st, *D.problem_args(c), **search)
        try:
            return s.poses(row_f, row_f_init=f, pt_new_added=added, **opts), s.n_kept, s.n_corr
        finally:
            s.close()

    def roundtrip(rows):
        loc = ctx.localize_candidates(st, *D.problem_args(c), **search)
        off = loc["corr_off"]
        n = len(off) - 1 if rows == 0 else min(rows, len(off) - 1)
        R, t, err, avg, _ = ctx.epnp_ransac(off[:n + 1], loc["pts_w"][:off[n]], loc["pts_2d"][:off[n]], f)
        for r in range(n):
            if off[r + 1] - off[r] >= TH_MIN and not avg[r] > TH_MSE:
                return r, numpy_rules(err[off[r]:off[r + 1]], avg[r], loc["corr_point"][off[r]:off[r + 1]], added)
        return -1, None

    (first, n_kept, n_corr), tm = timed(lambda: resident(f, max_tries=16), a.reps)
    ctx.profile(True); ctx.profile_reset()
    resident(f, max_tries=16)
    prof = ctx.profile_get()
    ctx.profile(False)
    shape = dict(images=len(c["n_features"]), registered=LB.N_REGISTERED, matches=int(c["match_off"][-1]), kept=n_kept, correspondences=n_corr,
                 points=n_pts)
    LB.emit(dict(what="localizepose", part="resident", arm="known", max_tries=16, winner=first["winner"], n_tried=first["n_tried"], **tm, **shape,
                 kernels_ms={k: round(v["total_ms"], 3) for k, v in prof.items()}), a.out)
    loc0 = ctx.localize_candidates(st, *D.problem_args(c), **search)
    off, w = loc0["corr_off"], first["winner"]
    win_image = int(c["cand_img"][loc0["rank"][w]]) if w >= 0 else -1
    for rows in (16, 0):
        (win, state), tm = timed(lambda: roundtrip(rows), a.reps)
        same = win == w and (w < 0 or np.array_equal(state, first["corr_state"][off[w]:off[w + 1]]))
        LB.emit(dict(what="localizepose", part="roundtrip", arm="known", rows=rows, winner=win, same_winner_and_states=bool(same), **tm), a.out)
    (r, _, _), tm = timed(lambda: resident(f, max_tries=0), a.reps)
    LB.emit(dict(what="localizepose", part="resident", arm="known", max_tries=0, winner=r["winner"], n_tried=r["n_tried"], **tm), a.out)
    for tries in (1, 16):
        (r, _, _), tm = timed(lambda: resident(0.0, max_tries=tries), a.reps)
        LB.emit(dict(what="localizepose", part="resident", arm="sweep", max_tries=tries, winner=r["winner"], n_tried=r["n_tried"],
                     f_kept=float(r["f"][r["winner"]]) if r["winner"] >= 0 else None, **tm), a.out)
    st.close(); ctx.close()
    if a.no_host:
        return
    sc = scene.config_scene(3)
    n_img, n_reg = len(c["n_features"]), LB.N_REGISTERED
    R = scene.angle_axis_to_R(sc.cam_pose_gt[:n_reg, :3])
    t = sc.cam_pose_gt[:n_reg, 3:]
    state = dict(cam_img=c["cam_img"], feat_point=c["feat_point"], cam_R=R, cam_t=t, cam_c=-np.einsum("nji,nj->ni", R, t),
                 cam_fk=np.tile([f, 0.0, 0.0], (n_reg, 1)), point_xyz=c["point_xyz"], pt_bad=c["pt_bad"], pt_mse=c["pt_mse"], pt_views=c["pt_views"],
                 pt_new_added=added)
    h = dict(case=c, state=state, image_f=np.full(n_img, f), image_f_init=np.full(n_img, f), image_model=np.arange(n_img, dtype=np.int32),
             fail_times=c["fail_by_image"])
    with tempfile.TemporaryDirectory() as tmp:
        exe, src, dst = (os.path.join(tmp, x) for x in ("localizepose_host_check", "in.bin", "out.bin"))
        subprocess.check_call(PD.host_check_command(exe))
        PD.write_host_round(src, h)
        run = subprocess.run([exe, src, dst, "time"], capture_output=True, text=True, timeout=900)
        if run.returncode != 0:
            raise RuntimeError(run.stdout + run.stderr)
        word = [ln for ln in run.stdout.splitlines() if ln.startswith("time_ms")][0].split()
        got = PD.read_host_round_result(dst, h)
        LB.emit(dict(what="localizepose", part="host", batched_ms=float(word[2]), walk_ms=float(word[4]), image=got["image"],
                     same_image=bool(got["image"] == win_image)), a.out)


if __name__ == "__main__":
    main()
