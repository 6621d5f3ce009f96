"""Timing of stereo rectification in front of dense stereo: what it costs to start from the posed pair on the device instead of
from a pair that was rectified elsewhere.

  python scripts/rectify_bench.py [--reps 9] [--out FILE (default profiles/rectify_bench.jsonl, rewritten)] [--only NAME] [--no-cpu]
                                  [--label TEXT] [--append]

Workloads: slam = 1 280 x 720 and photo = 2 000 x 1 500, each at D = 64 and 128, on a seeded texture pair with planted
disparities (tests/sgm_data.planted_pair) under convergent poses (rotations of 0.02 .. 0.04 rad, focal lengths near the width).
Per workload one JSON line:
  posed      (a) rectify + execute_rectified + fetch of the uint8 plane, from the raw pair: wall time with every wait inside,
             median / min / max of --reps after a warm-up
  rectified  (b) execute + fetch on the already rectified pair (host arrays), in the same process and alternating with (a) run by
             run: what a caller ran who rectified elsewhere
  a_minus_b  the difference of the two medians, whichever sign it has
  kernels    rectify_remap and the seven sgm classes, per-class median of five further, profiled runs of (a) (event pairs of the
             library); remap_gbps: the remap launch's algorithmic bytes, 4 w h (two planes read, two written), per second - the
             copy rate of this machine, 6.3 TB/s (README, "Describing the features"), is the number to hold it against
  cpu        (c) tests/rectify_ref.cpp's maps and warp of the same pair on one thread of this host, which is what those callers
             paid in front of (b); whether the device's rectified planes equal its planes
--label names the build that was measured; the machine and its GPU are named in the first line."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from tests import rectify_data as RD  # noqa: E402
from tests import sgm_data as X  # noqa: E402
from sgm_bench import CLASSES, DISPS, IMAGES  # noqa: E402
from words_bench import box, emit  # noqa: E402


def bench_poses(w, h):
    """Camera 1 (the left image) at the origin, camera 2 one unit to its right, both turned a little about all three axes."""
    def K(fx, fy, cx, cy):
        return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float64)
    R1, R2 = RD.rot(0.03, -0.02, 0.02), RD.rot(0.02, 0.04, -0.03)
    c2 = np.array([1.0, 0.03, -0.02])
    return [K(0.95 * w, 0.93 * w, 0.5 * w + 3.5, 0.5 * h - 2.25), R1, np.zeros(3), K(0.9 * w, 0.96 * w, 0.5 * w - 5.0, 0.5 * h + 4.5), R2, -R2 @ c2]


def stats_of(ts, reps):
    return dict(wall_ms=round(float(np.median(ts)), 3), wall_ms_min=round(min(ts), 3), wall_ms_max=round(max(ts), 3), reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rectify_bench.jsonl"))
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
    emit(dict(what="rectify_bench", box=box(), reps=a.reps, label=a.label, options=dict(p1=10, p2=120, uniqueness=0.96)), a.out)
    for name, (w, h) in IMAGES.items():
        if a.only and name != a.only:
            continue
        poses = bench_poses(w, h)
        for D in DISPS:
            left, right, _ = X.planted_pair(w, h, 21, D // 8, D // 3, noise=2.0)
            rec = dict(image=name, w=w, h=h, disp_size=D, label=a.label)
            with ctx.rectifier(w, h) as rect, ctx.stereo_sgm(w, h, D) as sgm:
                rec["device_bytes"] = dict(rectifier=rect.size()["device_bytes"], sgm=sgm.size()["device_bytes"])

                def posed():
                    rect.rectify(left, right, *poses)
                    sgm.execute_rectified(rect)
                    return sgm.disparity()
                from_posed = posed()
                rl, rr = rect.fetch(0), rect.fetch(1)

                def rectified():
                    sgm.execute(rl, rr)
                    return sgm.disparity()
                rec["same_disparity"] = bool(np.array_equal(from_posed, rectified()))
                ta, tb = [], []
                for _ in range(a.reps):      # alternating, so that a drift of the machine meets both alike
                    for fn, ts in ((posed, ta), (rectified, tb)):
                        t0 = time.perf_counter()
                        fn()
                        ts.append((time.perf_counter() - t0) * 1e3)
                rec["posed"], rec["rectified"] = stats_of(ta, a.reps), stats_of(tb, a.reps)
                rec["a_minus_b_ms"] = round(rec["posed"]["wall_ms"] - rec["rectified"]["wall_ms"], 3)
                ctx.profile(True)
                runs = []
                for _ in range(5):
                    ctx.profile_reset()
                    posed()
                    p = ctx.profile_get()
                    runs.append({k: p[k]["total_ms"] for k in ("rectify_remap",) + CLASSES if k in p})
                ctx.profile(False)
                k = {c: round(float(np.median([r[c] for r in runs])), 4) for c in runs[0]}
                rec["kernels_ms"] = k
                rec["remap_bytes"] = 4 * w * h
                rec["remap_gbps"] = round(4.0 * w * h / k["rectify_remap"] * 1e-6, 1)
            if not a.no_cpu:
                ref = RD.run_ref_cpp(left, right, dict(zip(("K1", "R1", "t1", "K2", "R2", "t2"), poses)))
                rec["cpu_one_thread"] = dict(ms=round(ref["seconds"] * 1e3, 1),
                                             planes_equal=bool(np.array_equal(rl, ref["left"]) and np.array_equal(rr, ref["right"])))
            emit(rec, a.out)
    ctx.close()


if __name__ == "__main__":
    main()
