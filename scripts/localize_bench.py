"""Timing of one FindImageToLocalize round (sfm_incremental.cc:417-563) at BASELINE config 3: 500 images, the matches of
`flat_matches_from_scene`, images 0-249 registered, the candidates `candidate_images` yields.

  python scripts/localize_bench.py [--reps 9] [--out FILE] [--no-host] [--calls-only N]

Three numbers, one JSON line each:
  store     msfm_match_store_create, once (the only transfer that scales with the matches)
  round     one msfm_localize_candidates call through the Python binding: median / min / max of --reps after a warm-up, the
            bytes it sent to the device, and the kernel split of msfm_ctx_profile_get from one further call
  host      the same round through the host mirror (tests/localize_host_check.cc, -O2): its library round, gathering the flat
            state from the std::map objects included, and its literal std::map walk on one thread with the matches in memory
            (the reference re-parses `<i>_match` files on top of that)
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
from metricsfm_amd import capi, localize, scene  # noqa: E402
from metricsfm_amd.tracks import flat_matches_from_scene  # noqa: E402
from tests import localize_data as D  # noqa: E402

N_REGISTERED = 250


def build_round():
    sc = scene.config_scene(3)
    nf, pairs, moff, m = flat_matches_from_scene(sc)
    n = sc.n_cams
    rng = np.random.default_rng(3)
    by_cam = np.argsort(sc.obs_cam, kind="stable")                 # feature f of image c = its f-th observation
    start = np.concatenate([[0], np.cumsum(nf)])
    cam_img = np.arange(N_REGISTERED, dtype=np.int32)
    feat_point = sc.obs_pt[by_cam][:start[N_REGISTERED]].astype(np.int32)
    pt_views = np.bincount(sc.obs_pt, minlength=sc.n_points).astype(np.int32)
    match_count = np.zeros((n, n), np.int32)
    match_count[pairs[:, 0], pairs[:, 1]] = np.diff(moff)
    fail = np.zeros(n, np.int32)
    processed = np.zeros(n, bool); processed[cam_img] = True
    cand = localize.candidate_images(match_count, processed, fail)
    c = dict(n_features=nf, pairs=pairs, match_off=moff, matches=m, cam_img=cam_img, feat_point=feat_point,
             pt_bad=(rng.random(sc.n_points) < 0.05).astype(np.uint8), pt_mse=rng.uniform(0, 4, sc.n_points), pt_views=pt_views,
             cand_img=cand, fail_times=fail[cand], point_xyz=sc.point_gt, fail_by_image=fail)
    walked = np.isin(pairs[:, 0], cand) & processed[pairs[:, 1]]
    c["walked_matches"] = int(np.diff(moff)[walked].sum())
    c["keypoints"] = sc.obs_xy[by_cam].astype(np.float32)         # (row of image c, feature f = start[c] + f)
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
    shape = dict(images=len(c["n_features"]), registered=N_REGISTERED, candidates=len(c["cand_img"]), matches=int(c["match_off"][-1]),
                 walked_matches=c["walked_matches"], registered_features=len(c["feat_point"]), points=len(c["pt_bad"]))
    ctx = capi.Context(0)
    t0 = time.perf_counter()
    st = ctx.match_store(*D.store_args(c))
    ms_store = (time.perf_counter() - t0) * 1e3
    call = lambda: ctx.localize_candidates(st, *D.problem_args(c), point_xyz=c["point_xyz"], keypoints=c["keypoints"])  # noqa: E731
    if a.calls_only:
        for _ in range(a.calls_only):
            call()
        st.close(); ctx.close()
        return
    emit(dict(what="localize", part="store", ms=round(ms_store, 3), h2d_bytes=int(c["matches"].nbytes), **shape), a.out)
    r = call()
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        r = call()
        ts.append((time.perf_counter() - t0) * 1e3)
    ctx.profile(True); ctx.profile_reset()
    call()
    prof = ctx.profile_get()
    ctx.profile(False)
    emit(dict(what="localize", part="round", wall_ms=round(float(np.median(ts)), 3), wall_ms_min=round(min(ts), 3), wall_ms_max=round(max(ts), 3),
              reps=a.reps, h2d_bytes=int(r["h2d_bytes"]), kept=len(r["rank"]), correspondences=int(r["corr_off"][-1]),
              longest_segment=int(np.diff(r["corr_off"]).max()) if len(r["rank"]) else 0,
              kernels_ms={k: round(v["total_ms"], 3) for k, v in prof.items()} if isinstance(prof, dict) else prof), a.out)
    st.close(); ctx.close()
    if a.no_host:
        return
    with tempfile.TemporaryDirectory() as tmp:
        exe, src, dst = (os.path.join(tmp, x) for x in ("localize_host_check", "in.bin", "out.bin"))
        subprocess.check_call(D.host_check_command(exe))
        D.write_round(src, c, c["fail_by_image"])
        run = subprocess.run([exe, src, dst, "time"], capture_output=True, text=True, timeout=900)
        if run.returncode != 0:
            raise RuntimeError(run.stdout + run.stderr)
        word = [ln for ln in run.stdout.splitlines() if ln.startswith("timing_ms")][0].split()
        ids, corres, _ = D.read_round_result(dst)
        same = ids == [int(c["cand_img"][k]) for k in r["rank"]] and all(
            np.array_equal(x[:, 0], r["corr_feat"][r["corr_off"][i]:r["corr_off"][i + 1]]) for i, x in enumerate(corres))
        emit(dict(what="localize", part="host", store_ms=float(word[2]), library_round_ms=float(word[4]), map_walk_one_thread_ms=float(word[6]),
                  equals_python_round=bool(same)), a.out)


if __name__ == "__main__":
    main()
