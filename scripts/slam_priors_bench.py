"""Timing of SLAMGPS::FeatureMatching step 1 on the GPU (msfm_slam_priors) and of the homography RANSAC alone.

  python scripts/slam_priors_bench.py [--configs 2 5] [--reps 3] [--cpu-sample 16] [--out FILE]

Per config (BASELINE scenes 2 and 5, their observations used as the SLAM points): wall time of msfm_slam_priors (median of
--reps after one warm-up call) and its kernel split (msfm_ctx_profile_*), candidates and kept pairs.  Then homography
pairs/s of msfm_homography_ransac_batch on 200- and 1 500-point pairs (planar, 30 % outliers, polish on), and the
sequential CPU restatement tests/hransac_ref.cpp on ONE thread for --cpu-sample pairs of each size: its per-pair time and
that time multiplied by the number of pairs - an extrapolation, labelled as such.  One JSON line per result.

  python scripts/slam_priors_bench.py --baseline-lib LIBMSFM_OF_THE_PARENT_COMMIT [--configs 2 5] [--reps 5] [--out FILE]

A/B of the two RANSACs against another build of the library: the inputs are written once, then child processes run them
alternately with the baseline and with this tree's library (baseline, new, baseline, new; MSFM_LIB picks the build).  The
workloads: F on the benchmark's verification leg (2 048 pairs of 256 matches, 30 % outliers) and on the same pair count at
60 % outliers (nearly every pair takes the second pass), H on 4 000 pairs of 200 and 1 000 pairs of 1 500 points,
msfm_slam_priors at --configs.  Each child makes one warm-up call, --reps timed calls and three profiled calls per workload
and hashes every output array.  Per workload one line: whether all four runs gave byte-identical outputs, the band
[min, max] of all the baseline's timed calls, the new build's median / min / max, and the same per kernel class of the
profiled calls; "pass" = the new median is not above the top of the baseline's band."""
import argparse
import hashlib
import json
import os
import subprocess
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


def bench_verification_leg(n_pairs=2048, n_matches=256):
    """The input of bench.py's geometric-verification leg (64 two-view geometries tiled to n_pairs pairs): a copy of the
    generator in bench.py (main(), under "geometric-verification leg", the lines from `rng = np.random.default_rng(0x4D53464D)`
    to `voff = ...`) - compare with it when bench.py changes."""
    rng = np.random.default_rng(0x4D53464D)

    def two_view(n):
        X = np.column_stack([rng.uniform(-40, 40, n), rng.uniform(-30, 30, n), rng.uniform(80, 120, n)])
        a = rng.normal(0, 0.05, 3)
        th = np.linalg.norm(a)
        K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]]) / th
        R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
        Xc = X @ R.T + np.array([10.0, 1.0, 0.5])
        x1 = 4800 * X[:, :2] / X[:, 2:3] + rng.normal(0, 0.5, (n, 2))
        x2 = 4800 * Xc[:, :2] / Xc[:, 2:3] + rng.normal(0, 0.5, (n, 2))
        bad = rng.choice(n, int(0.3 * n), replace=False)
        x2[bad] = np.column_stack([rng.uniform(-2000, 2000, len(bad)), rng.uniform(-1500, 1500, len(bad))])
        return x1.astype(np.float32), x2.astype(np.float32)

    tv = [two_view(n_matches) for _ in range(64)]
    v1 = np.concatenate([tv[p % 64][0] for p in range(n_pairs)])
    v2 = np.concatenate([tv[p % 64][1] for p in range(n_pairs)])
    return (np.arange(n_pairs + 1) * n_matches).astype(np.int32), v1, v2


def ab_inputs(configs, tmp):
    """Writes the A/B workloads to tmp; returns [(name, kind, file)]."""
    from tests import twoview
    W = []

    def put(name, kind, **arrays):
        f = os.path.join(tmp, name + ".npz")
        np.savez(f, **arrays)
        W.append((name, kind, f))

    off, p1, p2 = bench_verification_leg()
    put("f_bench_leg_30pct", "f", off=off, p1=p1, p2=p2)
    off, p1, p2, _ = twoview.make_batch(11, [256] * 2048, outlier_frac=0.6)
    put("f_2048x256_60pct", "f", off=off, p1=p1, p2=p2)
    rng = np.random.default_rng(7)
    for n, count in ((200, 4000), (1500, 1000)):
        off, p1, p2 = D.batch([D.make_pair(rng, n, 0.3, planar=True, noise=0.5)[:2] for _ in range(count)])
        put("h_%dx%d" % (count, n), "h", off=off, p1=p1, p2=p2)
    for cfg in configs:
        sc = scene.config_scene(cfg)
        put("slam_priors_c%d" % cfg, "priors", n_cams=np.int64(sc.n_cams), toff=sc.track_offsets(), cam=sc.obs_cam, xy=sc.obs_xy)
    return W


def ab_child(a):
    """One build of the library (the one this process loaded) on every workload of --child; one JSON line each."""
    ctx = capi.Context(0)
    for item in a.child:
        name, kind, f = item.split(",")
        z = np.load(f)
        if kind == "f":
            run = lambda: ctx.fundamental_ransac(z["off"], z["p1"], z["p2"])
        elif kind == "h":
            run = lambda: ctx.homography_ransac(z["off"], z["p1"], z["p2"], threshold=5.0)
        else:
            run = lambda: ctx.slam_priors(int(z["n_cams"]), z["toff"], z["cam"], z["xy"])
        res = run()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            run()
            ts.append((time.perf_counter() - t0) * 1e3)
        kernels = []
        ctx.profile(True)
        for _ in range(3):
            ctx.profile_reset()
            run()
            kernels.append({k: v["total_ms"] for k, v in ctx.profile_get().items()})
        ctx.profile(False)
        sha = [hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest() for x in res]
        print(json.dumps(dict(workload=name, lib=capi.LIB_PATH, wall_ms=ts, kernels=kernels, sha256=sha)), flush=True)
    ctx.close()


def ab_parent(a):
    base = os.path.abspath(a.baseline_lib)
    runs = {}   # workload -> {"baseline": [child records], "new": [...]}
    with tempfile.TemporaryDirectory() as tmp:
        W = ab_inputs(a.configs, tmp)
        for which in ("baseline", "new", "baseline", "new"):
            env = dict(os.environ)
            env.pop("MSFM_LIB", None)
            if which == "baseline":
                env["MSFM_LIB"] = base
            cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--child"] + [",".join(w) for w in W]
            out = subprocess.run(cmd, check=True, timeout=900, env=env, stdout=subprocess.PIPE, text=True).stdout
            for line in out.splitlines():
                if line.startswith("{"):
                    r = json.loads(line)
                    runs.setdefault(r["workload"], {}).setdefault(which, []).append(r)
    stat = lambda v: dict(median=round(float(np.median(v)), 4), min=round(min(v), 4), max=round(max(v), 4), n=len(v))
    for name, _, _ in W:
        b, n = runs[name]["baseline"], runs[name]["new"]
        bw, nw = sum((r["wall_ms"] for r in b), []), sum((r["wall_ms"] for r in n), [])
        classes = {}
        for k in sorted(set().union(*[c.keys() for r in b + n for c in r["kernels"]])):
            bk = [c.get(k, 0.0) for r in b for c in r["kernels"]]
            nk = [c.get(k, 0.0) for r in n for c in r["kernels"]]
            classes[k] = dict(baseline=stat(bk), new=stat(nk), **{"pass": bool(np.median(nk) <= max(bk))})
        emit(dict(what="ransac_core_ab", note=a.note, workload=name, baseline_lib=os.path.basename(os.path.dirname(base)) + "/" + os.path.basename(base),
                  outputs_identical=len({tuple(r["sha256"]) for r in b + n}) == 1, wall_ms=dict(baseline=stat(bw), new=stat(nw)),
                  **{"pass": bool(np.median(nw) <= max(bw))}, kernel_ms=classes), a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=int, nargs="*", default=[2, 5])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-sample", type=int, default=16)
    ap.add_argument("--out", default=None)
    ap.add_argument("--baseline-lib", default=None, help="A/B against this build of libmsfm.so (see the module text)")
    ap.add_argument("--note", default=None, help="A/B: stored in every result line (which build the new side is, say)")
    ap.add_argument("--child", nargs="*", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        return ab_child(a)
    if a.baseline_lib:
        return ab_parent(a)
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
