"""Timing of the scale space (msfm_scalespace_create) and of the descriptors of given frames (msfm_descset_describe) on the device,
beside the one-thread C++ restatement tests/sift_ref.cpp on the same inputs.

  python scripts/sift_bench.py [--reps 9] [--out FILE (default profiles/sift_bench.jsonl, rewritten)] [--only NAME] [--no-cpu]
                               [--label TEXT] [--append]

Images: photo = 4 000 x 3 000 (the reference's photographs), slam = 1 280 x 720 (the SLAM frames); synthetic: a small blob image
enlarged eight times, a ramp and noise.  O = 4, S = 5.  Frame sets: 4 096 and 60 000 frames (the reference's cap), the share of
octave o proportional to 2^-o, the level uniform, positions and angles uniform.  Per image one JSON line:
  create   wall time of Context.scalespace (upload, every wait), median / min / max of --reps after a warm-up; the sift_* kernel
           classes as the per-class median of five further, profiled runs (event pairs of the library); bytes sent; per blur pass the algorithmic bytes (one
           read and one write of 4 bytes per pixel) over its time, in GB/s
  describe per frame set: wall time of DescSet.describe, the sift_describe and descset_prep classes, bytes sent
  window   4 096 frames of one window size each: W = 9 (sigma' = 0.85 on level (0, 0)), W = 34 (the top level of octave 0) and
           W = 39 (the top octave's clamp, sigma' = 3.68): the descriptor kernel in ns per frame
  handover describe of two images + match_pairs against upload of the same rows and keypoints from the host + match_pairs
  cpu      tests/sift_ref.cpp on one thread of this host: scale space, and the 4 096-frame set (the 60 000-frame set on the slam
           image only); whether the device's rows equal its rows bit for bit
--label names the build that was measured; the machine and its GPU are named in the first line."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from tests import sift_data as D  # noqa: E402
from words_bench import box, emit, stats  # noqa: E402

IMAGES = {"photo": (4000, 3000), "slam": (1280, 720)}
O, S = 4, 5
F32 = np.float32


def big_image(w, h, seed):
    small = D.image((w + 7) // 8, (h + 7) // 8, seed).astype(np.float64)
    v = np.kron(small, np.ones((8, 8)))[:h, :w]
    rng = np.random.default_rng(seed + 1)
    v = 0.8 * v + 20.0 * np.arange(w)[None, :] / w + rng.uniform(-8, 8, (h, w))
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def frame_set(w, h, n, seed):
    rng = np.random.default_rng(seed)
    share = np.array([2.0 ** -o for o in range(O)])
    o = rng.choice(O, n, p=share / share.sum())
    i_s = rng.integers(0, S, n)
    sigma = np.array([D.sigma_for(S, a, b) for a, b in zip(o, i_s)])
    return np.column_stack([rng.uniform(0, w, n), rng.uniform(0, h, n), sigma, rng.uniform(-np.pi, np.pi, n)]).astype(F32)


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return stats(ts)


def profiled(ctx, fn, runs=5):
    """The library's kernel classes of fn(): the per-class median over `runs` profiled runs (one run alone now and then catches a
    launch that waited)."""
    ctx.profile(True)
    got = []
    for _ in range(runs):
        ctx.profile_reset()
        fn()
        got.append({k: v["total_ms"] for k, v in ctx.profile_get().items() if k.startswith("sift_") or k == "descset_prep"})
    ctx.profile(False)
    return {k: round(float(np.median([g[k] for g in got])), 4) for k in got[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sift_bench.jsonl"))
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
    emit(dict(what="sift_bench", box=box(), reps=a.reps, label=a.label, options=dict(n_octaves=O, n_levels=S)), a.out)
    for name, (w, h) in IMAGES.items():
        if a.only and name != a.only:
            continue
        img = big_image(w, h, 21)
        rec = dict(image=name, w=w, h=h, label=a.label)
        held = []

        def create():
            for s in held:
                s.close()
            held[:] = [ctx.scalespace(img, O, S)]
        rec["create"] = timed(create, a.reps)
        kern = profiled(ctx, create)
        ss = held[0]
        rec["create"]["kernels_ms"] = kern
        rec["create"]["h2d_bytes"] = ss.size(0)["h2d_bytes"]
        px = sum((w >> o) * (h >> o) * (S + 3 if o == 0 else S + 2) for o in range(O))   # blurred planes, in pixels
        for k in ("sift_blur_rows", "sift_blur_cols"):
            rec["create"][k + "_GBps"] = round(8.0 * px / (kern[k] * 1e-3) / 1e9, 1)
        ds = ctx.descset([np.zeros((0, 128), F32)] * 2)
        sets = {n: frame_set(w, h, n, 31 + n) for n in (4096, 60000)}
        rec["describe"] = {}
        for n, fr in sets.items():
            sent = []
            r = timed(lambda: sent.append(ds.describe(0, ss, fr, 1)), a.reps)
            r["kernels_ms"] = profiled(ctx, lambda: ds.describe(0, ss, fr, 1))
            r["h2d_bytes"] = sent[-1]
            r["describe_ns_per_frame"] = round(r["kernels_ms"]["sift_describe"] * 1e6 / n, 1)
            rec["describe"][str(n)] = r
        rec["window"] = {}
        rng = np.random.default_rng(5)
        for W, sigma in ((9, 0.85), (34, D.sigma_for(S, 0, S - 1)), (39, 3.68 * 2 ** (O - 1))):
            sc = 2.0 ** (O - 1) if W == 39 else 1.0
            m = min(50 * sc, 0.25 * min(w, h))   # the windows stay inside the level
            fr = np.column_stack([rng.uniform(m, w - m, 4096), rng.uniform(m, h - m, 4096), np.full(4096, sigma),
                                  rng.uniform(-3, 3, 4096)]).astype(F32)
            ds.describe(1, ss, fr, 1)
            k = profiled(ctx, lambda: ds.describe(1, ss, fr, 1))
            rec["window"]["W%d" % W] = dict(sigma=round(float(sigma), 3), describe_ms=k["sift_describe"], ns_per_frame=round(k["sift_describe"] * 1e6 / 4096, 1))
        # hand-over: two images of 4 096 frames each, quantised rows
        fa, fb = sets[4096], frame_set(w, h, 4096, 77)
        pairs = [[0, 1]]

        def resident():
            ds.describe(0, ss, fa, 1)
            ds.describe(1, ss, fb, 1)
            ds.match_pairs(pairs).close()
        rec["handover"] = dict(describe_match=timed(resident, a.reps))
        host = [ds.fetch(0), ds.fetch(1)]

        def from_host():
            with ctx.descset([r for r, _ in host], [xy for _, xy in host]) as up:
                up.match_pairs(pairs).close()
        rec["handover"]["upload_match"] = timed(from_host, a.reps)
        rec["handover"]["upload_bytes"] = int(sum(r.nbytes + xy.nbytes for r, xy in host))
        if not a.no_cpu:
            rec["cpu_one_thread"] = {}
            for n in ((4096, 60000) if name == "slam" else (4096,)):
                ds.describe(0, ss, sets[n], 1)
                got = ds.fetch(0)[0]
                ref = D.run_ref_cpp(img, O, S, sets[n])
                rec["cpu_one_thread"][str(n)] = dict(scalespace_ms=round(ref["seconds"][0] * 1e3, 1), describe_ms=round(ref["seconds"][1] * 1e3 / 2, 1),
                                                     rows_equal=bool(np.array_equal(got.view(np.uint32), ref["rows"][1].view(np.uint32))))
        ds.close()
        ss.close()
        emit(rec, a.out)
    ctx.close()


if __name__ == "__main__":
    main()
