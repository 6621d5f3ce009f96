"""Timing of the SIFT detector (msfm_scalespace_detect) and of the whole extraction (msfm_descset_extract) on the device, beside
the one-thread C++ restatement tests/siftdetect_ref.cpp on the same planes and the same host.

  python scripts/siftdetect_bench.py [--reps 9] [--out FILE (default profiles/siftdetect_bench.jsonl, rewritten)] [--only NAME]
                                     [--no-cpu] [--label TEXT] [--append]

Images: photo = 4 000 x 3 000 and slam = 1 280 x 720, the synthetic images of scripts/sift_bench.py; O = 4, S = 5.  Thresholds:
peak_thresh 0 (the reference's) and 0.5, edge_thresh 10.  Per image and peak_thresh one JSON line:
  detect   wall time of ScaleSpace.detect with its three waits, median / min / max of --reps after a warm-up; the kernel classes
           sift_extrema, sift_compact, sift_refine, sift_orient as the per-class median of five further, profiled runs (event
           pairs of the library); candidates, keypoints, n_found, frames returned, bytes each way
  extract  DescSet.extract (one call) beside ScaleSpace.detect + DescSet.describe (two calls, the frames crossing the binding),
           quantised rows, at most 65 535 frames
  cpu      tests/siftdetect_ref.cpp on one thread of this host on the planes tests/sift_ref.cpp made of the same image; whether
           the device's frames equal its frames bit for bit
--label names the build that was measured; the machine and its GPU are named in the first line."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from sift_bench import IMAGES, O, S, big_image, timed  # noqa: E402
from tests import sift_data as D  # noqa: E402
from tests import siftdetect_data as X  # noqa: E402
from words_bench import box, emit  # noqa: E402

F32 = np.float32
PEAKS = (0.0, 0.5)
CLASSES = ("sift_extrema", "sift_compact", "sift_refine", "sift_orient", "sift_describe", "descset_prep")


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "siftdetect_bench.jsonl"))
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
    emit(dict(what="siftdetect_bench", box=box(), reps=a.reps, label=a.label, options=dict(n_octaves=O, n_levels=S, edge_thresh=10.0)), a.out)
    for name, (w, h) in IMAGES.items():
        if a.only and name != a.only:
            continue
        img = big_image(w, h, 21)
        planes = None if a.no_cpu else D.run_ref_cpp(img, O, S, np.zeros((0, 4), F32))
        ss = ctx.scalespace(img, O, S)
        ds = ctx.descset([np.zeros((0, 128), F32)] * 2)
        for peak in PEAKS:
            rec = dict(image=name, w=w, h=h, peak_thresh=peak, label=a.label)
            out = []
            r = timed(lambda: out.append(ss.detect(peak)), a.reps)
            frames, st = out[-1]
            r["kernels_ms"] = profiled(ctx, lambda: ss.detect(peak))
            r.update({k: st[k] for k in ("candidates", "keypoints", "n_found", "host_waits", "h2d_bytes", "d2h_bytes")}, frames_returned=len(frames))
            rec["detect"] = r

            def two_calls():
                fr, _ = ss.detect(peak)
                ds.describe(1, ss, fr, 1)
            rec["extract"] = dict(one_call=timed(lambda: ds.extract(0, ss, peak, quantize=1), a.reps), detect_then_describe=timed(two_calls, a.reps))
            rec["extract"]["kernels_ms"] = profiled(ctx, lambda: ds.extract(0, ss, peak, quantize=1))
            rec["extract"]["rows_equal"] = bool(np.array_equal(ds.fetch(0)[0].view(np.uint32), ds.fetch(1)[0].view(np.uint32)))
            if planes is not None:
                ref = X.run_detect_cpp(planes, w, h, O, S, peak, 10.0)
                n = len(frames)
                rec["cpu_one_thread"] = dict(detect_ms=round(ref["seconds"] * 1e3, 1), n_found=ref["stats"]["n_found"],
                                             frames_equal=bool(np.array_equal(frames.view(np.uint32), ref["frames"][:n].view(np.uint32))),
                                             counters_equal=X.counters(st) == X.counters(ref["stats"]))
            emit(rec, a.out)
        ds.close()
        ss.close()
    ctx.close()


if __name__ == "__main__":
    main()
