"""Timing of dense stereo (msfm_sgm_execute + the fetch of the uint8 plane) on the device, beside the one-thread C++ restatement
tests/sgm_ref.cpp on the same pair and the same host.

  python scripts/sgm_bench.py [--reps 9] [--out FILE (default profiles/sgm_bench.jsonl, rewritten)] [--only NAME] [--no-cpu]
                              [--label TEXT] [--append]

Workloads: slam = 1 280 x 720 and photo = 2 000 x 1 500, each at D = 64 and 128, P1 = 10, P2 = 120, uniqueness 0.96, on a seeded
texture pair with two planted disparities and noise (tests/sgm_data.planted_pair).  Per workload one JSON line:
  wall     execute + fetch of the final plane, every wait inside, median / min / max of --reps after a warm-up
  kernels  the classes sgm_census, sgm_path_h, sgm_path_v, sgm_path_d, sgm_wta, sgm_median, sgm_check as the per-class median of
           five further, profiled runs (event pairs of the library)
  gbps     achieved GB/s of the path kernels (together and per class) and of the winner kernel against their algorithmic bytes:
           the eight volumes of W H D bytes written once by the former, read once by the latter.  The copy rate of this machine,
           6.3 TB/s (README, "Describing the features"), is the number to hold them against.
  cpu      tests/sgm_ref.cpp on one thread of this host on the same pair; whether the device's final plane equals its plane
--label names the build that was measured; the machine and its GPU are named in the first line."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from tests import sgm_data as X  # noqa: E402
from words_bench import box, emit  # noqa: E402

IMAGES = dict(slam=(1280, 720), photo=(2000, 1500))
DISPS = (64, 128)
CLASSES = ("sgm_census", "sgm_path_h", "sgm_path_v", "sgm_path_d", "sgm_wta", "sgm_median", "sgm_check")
PATHS_OF = dict(sgm_path_h=2, sgm_path_v=2, sgm_path_d=4)


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(wall_ms=round(float(np.median(ts)), 3), wall_ms_min=round(min(ts), 3), wall_ms_max=round(max(ts), 3), reps=reps)


def profiled(ctx, fn, runs=5):
    ctx.profile(True)
    got = []
    for _ in range(runs):
        ctx.profile_reset()
        fn()
        p = ctx.profile_get()
        got.append({k: p[k]["total_ms"] for k in CLASSES if k in p})
    ctx.profile(False)
    return {k: round(float(np.median([g[k] for g in got])), 4) for k in got[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sgm_bench.jsonl"))
    ap.add_argument("--only", default=None)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--label", default="as committed")
    ap.add_argument("--append", action="store_true", help="add to --out instead of rewriting it")
    a = ap.parse_args()
    from metricsfm_amd import capi
    ctx = capi.Context(0)   # fails without a GPU: nothing here is measured on a CPU fallback
    if a.out and not a.append:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()
    emit(dict(what="sgm_bench", box=box(), reps=a.reps, label=a.label, options=dict(p1=10, p2=120, uniqueness=0.96)), a.out)
    for name, (w, h) in IMAGES.items():
        if a.only and name != a.only:
            continue
        for D in DISPS:
            left, right, _ = X.planted_pair(w, h, 21, D // 8, D // 3, noise=2.0)
            rec = dict(image=name, w=w, h=h, disp_size=D, label=a.label)
            with ctx.stereo_sgm(w, h, D) as sgm:
                rec["device_bytes"] = sgm.size()["device_bytes"]

                def pair():
                    sgm.execute(left, right)
                    return sgm.disparity()
                rec["wall"] = timed(pair, a.reps)
                rec["stats"] = sgm.stats
                k = profiled(ctx, pair)
                rec["kernels_ms"] = k
                vol = float(w) * h * D   # bytes of one volume
                paths_ms = sum(k[c] for c in PATHS_OF)
                rec["gbps"] = dict(paths=round(8 * vol / paths_ms * 1e-6, 1), wta=round(8 * vol / k["sgm_wta"] * 1e-6, 1),
                                   **{c: round(n * vol / k[c] * 1e-6, 1) for c, n in PATHS_OF.items()})
                rec["floor_bytes"] = int(16 * vol)
                disp = sgm.disparity()
            if not a.no_cpu:
                ref = X.run_ref_cpp(left, right, D, volumes=False)
                rec["cpu_one_thread"] = dict(ms=round(ref["seconds"] * 1e3, 1), disparity_equal=bool(np.array_equal(disp, ref["disparity"])))
            emit(rec, a.out)
    ctx.close()


if __name__ == "__main__":
    main()
