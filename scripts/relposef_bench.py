"""Timing of the unknown-focal seed-pair arm (msfm_relpose_8pt_batch) with the known-focal arm (msfm_relpose_5pt_batch on the
same matches and the true focal lengths) beside it as a scale.  The capability is new: there is no route of a parent commit.

  python scripts/relposef_bench.py [--reps 5] [--cpu] [--out FILE]

Two workloads at the reference's 200 samples, generic scenes with 0.5 px noise: one pair of 2 000 matches (the reference's own
per-pair call) and 64 candidate seed pairs of 500.  Per workload and route: wall time of the call (median, min and max of
--reps after one warm-up call; the clock stops after the call's own device synchronise) and, from one further profiled
call, the kernel split of msfm_ctx_profile_get.  Each route runs in a child process (`--route`); MSFM_LIB in the environment
times a differently built libmsfm.so (`lib` in the result line says which).
--cpu adds the sequential CPU restatement (tests/relposef_ref.cpp, one thread) on both workloads and checks that the GPU
equals it bit for bit.  One JSON line per result, appended to --out."""
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
from tests import relposef_data as D  # noqa: E402

WORKLOADS = (("1x2000", 41, [2000]), ("64x500", 42, [500] * 64))
TIMES = 200


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
    return ts, r


def workload(seed, sizes):
    rng = np.random.default_rng(seed)
    return D.batch([D.make_pair(rng, n, noise=0.5)[:2] for n in sizes])


def run_route(route, reps, out):
    from metricsfm_amd import capi
    ctx = capi.Context(0)
    for name, seed, sizes in WORKLOADS:
        off, a, b = workload(seed, sizes)
        if route == "eight_point":
            call = lambda: ctx.relpose_8pt(off, a, b, ransac_times=TIMES)
        else:
            call = lambda: ctx.relpose_5pt(off, a, b, D.F_REF, D.F_CUR, ransac_times=TIMES)
        ts, res = timed(call, reps)
        ctx.profile(True)
        ctx.profile_reset()
        call()
        prof = ctx.profile_get()
        ctx.profile(False)
        rec = dict(what="relposef", route=route, lib=os.path.relpath(capi.LIB_PATH, ROOT), workload=name, pairs=len(sizes), ransac_times=TIMES,
                   wall_ms=round(float(np.median(ts)) * 1e3, 3), wall_ms_min=round(min(ts) * 1e3, 3), wall_ms_max=round(max(ts) * 1e3, 3),
                   reps=reps, kernels={k: round(v["total_ms"], 3) for k, v in prof.items()})
        if route == "eight_point":
            _, f1, f2, _, _, _, ok, _, _, _ = res
            good = ok == 1
            rec.update(ok=int(good.sum()),
                       f_ref_median_rel_err=round(float(np.median(np.abs(f1[good] / D.F_REF - 1))), 5) if good.any() else None,
                       f_cur_median_rel_err=round(float(np.median(np.abs(f2[good] / D.F_CUR - 1))), 5) if good.any() else None)
        else:
            rec.update(ok=int(res[3].sum()))
        emit(rec, out)
    ctx.close()


def run_cpu(out):
    from metricsfm_amd import capi
    ctx = capi.Context(0)
    with tempfile.TemporaryDirectory() as tmp:
        L = D.build_ref(tmp)
        for name, seed, sizes in WORKLOADS:
            off, a, b = workload(seed, sizes)
            t0 = time.perf_counter()
            want = D.ref_relpose_8pt(L, off, a, b, ransac_times=TIMES)
            dt = time.perf_counter() - t0
            got = ctx.relpose_8pt(off, a, b, ransac_times=TIMES)
            same = all(np.array_equal(g, w, equal_nan=g.dtype.kind == "f") for g, w in zip(got, want))
            emit(dict(what="relposef", route="cpu_reference_one_thread", workload=name, pairs=len(sizes), ransac_times=TIMES,
                      wall_ms=round(dt * 1e3, 3), gpu_equals_cpu_reference=bool(same)), out)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--route", choices=("eight_point", "five_point", "cpu"), default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relposef_bench.jsonl"))
    a = ap.parse_args()
    if a.route == "cpu":
        return run_cpu(a.out)
    if a.route:
        return run_route(a.route, a.reps, a.out)
    for route in ("eight_point", "five_point") + (("cpu",) if a.cpu else ()):
        subprocess.run([sys.executable, os.path.abspath(__file__), "--route", route, "--reps", str(a.reps), "--out", a.out],
                       check=True, timeout=600)


if __name__ == "__main__":
    main()
