"""Timing of SLAMGPS::FeatureMatching step 1 on the GPU (msfm_slam_priors) and of the homography RANSAC alone.

  python scripts/slam_priors_bench.py [--configs 2 5] [--reps 3] [--cpu-sample 16] [--out FILE]

Per config (BASELINE scenes 2 and 5, their observations used as the SLAM points): wall time of msfm_slam_priors (median of
--reps after one warm-up call) and its kernel split (msfm_ctx_profile_*), candidates and kept pairs.  Then homography
pairs/s of msfm_homography_ransac_batch on 200- and 1 500-point pairs (planar, 30 % outliers, polish on), and the
sequential CPU restatement tests/hransac_ref.cpp on ONE thread for --cpu-sample pairs of each size: its per-pair time and
that time multiplied by the number of pairs - an extrapolation, labelled as such.  One JSON line per result."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from metricsfm_amd import capi, scene  # noqa: E402
from tests import hransac_data as D  # noqa: E402


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=int, nargs="*", default=[2, 5])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-sample", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = capi.Context(0)
    for cfg in a.configs:
        t0 = time.perf_counter()
        sc = scene.config_scene(cfg)
        toff = sc.track_offsets()
        gen = time.perf_counter() - t0
        run = lambda: ctx.slam_priors(sc.n_cams, toff, sc.obs_cam, sc.obs_xy)
        wall, (pairs, F, H, cand) = timed(run, a.reps)
        ctx.profile(True)
        ctx.profile_reset()
        run()
        prof = ctx.profile_get()
        ctx.profile(False)
        ns = cand[:, 2]
        emit(dict(what="slam_priors", config=cfg, n_cams=sc.n_cams, n_points=sc.n_points, n_obs=sc.n_obs, scene_s=round(gen, 2),
                  wall_ms=round(wall * 1e3, 3), slots=len(cand), candidates=int((cand[:, 5] != 1).sum()), kept=len(pairs),
                  verdicts=np.bincount(cand[:, 5], minlength=4).tolist(), shared_mean=float(ns[ns >= 20].mean()) if (ns >= 20).any() else 0.0,
                  f_pass=int(((cand[:, 5] == 0) | (cand[:, 5] == 3)).sum()),
                  kernels={k: round(v["total_ms"], 3) for k, v in prof.items()} if isinstance(prof, dict) else prof), a.out)
    rng = np.random.default_rng(7)
    with tempfile.TemporaryDirectory() as tmp:
        try:
            L = D.build_ref(tmp)
        except Exception as e:   # no host compiler: GPU numbers only
            L = None
            print("CPU restatement not built: %s" % e, file=sys.stderr)
        for n, count in ((200, 4000), (1500, 1000)):
            parts = [D.make_pair(rng, n, 0.3, planar=True, noise=0.5)[:2] for _ in range(count)]
            off, p1, p2 = D.batch(parts)
            wall, res = timed(lambda: ctx.homography_ransac(off, p1, p2, threshold=5.0), a.reps)
            rec = dict(what="homography_ransac", points_per_pair=n, pairs=count, wall_ms=round(wall * 1e3, 3),
                       pairs_per_s=round(count / wall, 1), ok=int(res[3].sum()))
            if L is not None:
                k = min(a.cpu_sample, count)
                so, s1, s2 = off[:k + 1], p1[:off[k]], p2[:off[k]]
                t0 = time.perf_counter()
                D.ref_hransac(L, so, s1, s2, threshold=5.0)
                cpu = time.perf_counter() - t0
                rec.update(cpu_sample_pairs=k, cpu_one_thread_ms_per_pair=round(cpu / k * 1e3, 3),
                           cpu_one_thread_extrapolated_ms=round(cpu / k * count * 1e3, 1),
                           note="CPU: sequential restatement, one thread, measured on the first cpu_sample_pairs pairs and "
                                "extrapolated to all pairs")
            emit(rec, a.out)
    ctx.close()


if __name__ == "__main__":
    main()
