"""Timing of the pair selection from visual words (msfm_wordset_create + msfm_pair_select) against what a caller had.

  python scripts/pairselect_bench.py [--reps 9] [--out FILE (default profiles/pairselect_bench.jsonl, rewritten)] [--no-cpu] [--no-match]
                                     [--only NAME]

Workloads (synthetic: image i sees the points of a window that moves by `step` points per image, a point's word is its own, a
point's keypoint is its plane position shifted by the image's offset plus 0.3 px noise - a pure translation, which a
fundamental matrix explains -, the other features draw random words and positions; K by the reference's rule):
  c3_100k, c3_1m   config 3's shape: 500 images x 4 096 features, 2 458 observed, num_words 100 000 / 1 000 000
  c5_200           the first 200 images of config 5's shape: 4 096 features, 3 000 observed, num_words 1 000 000
Per workload, one JSON line each:
  batched   wall time of Context.wordset (create) and of the selection over all rows in chunks of --rows images (fetch of the
            per-hypothesis record included, the match lists left out), median / min / max of --reps after a warm-up; the
            pairsel_* and geo_* kernel times of one further profiled run; h2d_bytes; kept pairs against n (n - 1)
  cpu       tests/pairselect_ref.cpp on one thread: everything before the verification, and the verification as one
            msfm_fundamental_ransac_batch call per hypothesis for the first --ransac-calls of them (mean per call, and that
            mean times the hypotheses that reach the verification)
  match     msfm_match_pairs over all n (n - 1) ordered pairs and over the kept ones, same process, random descriptors
The machine and its GPU are named in the first line."""
import argparse
import json
import os
import re
import socket
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import pairselect_data as D  # noqa: E402

WORKLOADS = {"c3_100k": dict(n=500, feats=4096, observed=2458, step=100, num_words=100000),
             "c3_1m": dict(n=500, feats=4096, observed=2458, step=100, num_words=1000000),
             "c5_200": dict(n=200, feats=4096, observed=3000, step=120, num_words=1000000)}


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def workload(n, feats, observed, step, num_words, seed=0x5eb):
    rng = np.random.Generator(np.random.PCG64(seed))
    n_points = step * n + observed
    word_of_point = rng.permutation(num_words)[:n_points].astype(np.int32)
    xy_of_point = rng.uniform(-1500, 1500, size=(n_points, 2))
    words, kps = [], []
    for i in range(n):
        pts = np.arange(step * i, step * i + observed)
        w = np.concatenate([word_of_point[pts], rng.integers(0, num_words, feats - observed).astype(np.int32)])
        xy = np.concatenate([xy_of_point[pts] + rng.uniform(-300, 300, 2) + rng.normal(0, 0.3, (observed, 2)),
                             rng.uniform(-2000, 2000, size=(feats - observed, 2))])
        perm = rng.permutation(feats)
        words.append(w[perm])
        kps.append(xy[perm].astype(np.float32))
    return dict(n_features=np.full(n, feats, np.int32), words=words, num_words=num_words, keypoints=np.concatenate(kps))


def box():
    gpu = "unknown"
    try:
        txt = subprocess.run(["/opt/rocm/bin/rocminfo"], capture_output=True, text=True, timeout=60).stdout
        m = re.search(r"Marketing Name:\s*(AMD Instinct[^\n]*)", txt) or re.search(r"Name:\s*(gfx\w+)", txt)
        gpu = m.group(1).strip() if m else gpu
    except Exception:
        pass
    return dict(host=socket.gethostname(), gpu=gpu)


def stats(ts):
    return dict(wall_ms=round(float(np.median(ts)) * 1e3, 3), wall_ms_min=round(min(ts) * 1e3, 3), wall_ms_max=round(max(ts) * 1e3, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--ransac-calls", type=int, default=400)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairselect_bench.jsonl"))
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-match", action="store_true")
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    from metricsfm_amd import capi, scene
    ctx = capi.Context(0)   # fails without a GPU: nothing here is measured on a CPU fallback
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()
    emit(dict(what="pairselect_bench", box=box(), reps=a.reps, rows_per_call=a.rows), a.out)
    tmp = tempfile.mkdtemp()
    exe = os.path.join(tmp, "pairselect_ref")
    if not a.no_cpu:
        lib = os.path.join(ROOT, "metricsfm_amd")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "pairselect_ref.cpp"),
                               "-o", exe, "-L" + lib, "-lmsfm", "-Wl,-rpath," + lib, "-Wl,-rpath-link,/opt/rocm/lib"])
    for name, shape in WORKLOADS.items():
        if a.only and name != a.only:
            continue
        d = workload(**shape)
        n = shape["n"]
        base = dict(workload=name, **shape)

        def create():
            return ctx.wordset(d["n_features"], d["words"], d["num_words"], d["keypoints"])

        def select(ws):
            return [ws.select(r, min(a.rows, n - r), details=False) for r in range(0, n, a.rows)]

        ws = create()
        parts = select(ws)
        t_create, t_select = [], []
        for _ in range(a.reps):
            ws.close()
            t0 = time.perf_counter()
            ws = create()
            t_create.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            select(ws)
            t_select.append(time.perf_counter() - t0)
        ws.close()
        ctx.profile(True); ctx.profile_reset()
        ws = create()
        prof_create = ctx.profile_get()
        ctx.profile_reset()
        select(ws)
        prof_select = ctx.profile_get()
        ctx.profile(False); ctx.profile_reset()
        pairs = np.concatenate([p["pairs"] for p in parts]).reshape(-1, 2)
        n_init = np.concatenate([p["n_init"] for p in parts])
        verdict = np.concatenate([p["verdict"] for p in parts])
        emit(dict(base, route="batched", K=ws.n_hypotheses, create=stats(t_create), select=stats(t_select), h2d_bytes=ws.h2d_bytes,
                  n_inverted=ws.n_inverted, n_mapped=ws.n_mapped, hypotheses=int(verdict.size), reach_verification=int((n_init >= 30).sum()),
                  joined_matches=int(n_init.sum()), kept_pairs=len(pairs), all_pairs=n * (n - 1),
                  verdicts=[int((verdict == v).sum()) for v in range(4)],
                  kernels_create_ms={k: round(v["total_ms"], 3) for k, v in prof_create.items()},
                  kernels_select_ms={k: round(v["total_ms"], 3) for k, v in prof_select.items()}), a.out)
        ws.close()
        if not a.no_cpu:
            src = os.path.join(tmp, "in.bin")
            D.write_image_set(src, d, a.rows)
            run = subprocess.run([exe, src, str(a.ransac_calls)], capture_output=True, text=True, timeout=1200)
            m = re.search(r"restate_ms ([\d.]+) n_hyp (\d+) n_ransac (\d+) ransac_timed (\d+) ransac_ms ([\d.]+) kept (\d+) n_init_total (\d+)", run.stdout)
            if run.returncode != 0 or not m:
                emit(dict(base, route="cpu", error=(run.stdout + run.stderr)[-400:]), a.out)
            else:
                restate, n_r, timed, r_ms = float(m.group(1)), int(m.group(3)), int(m.group(4)), float(m.group(5))
                per_call = r_ms / max(1, timed)
                emit(dict(base, route="cpu", restatement_one_thread_ms=restate, reach_verification=n_r, ransac_calls_timed=timed,
                          ransac_ms_per_call=round(per_call, 4), ransac_one_at_a_time_ms_extrapolated=round(per_call * n_r, 1),
                          joined_matches=int(m.group(7)), equals_batched=bool(n_r == int((n_init >= 30).sum()) and int(m.group(7)) == int(n_init.sum()))),
                     a.out)
        if not a.no_match:
            rng = np.random.Generator(np.random.PCG64(0x5ec))
            descs = [rng.integers(0, 256, size=(shape["feats"], 128), dtype=np.uint8).astype(np.float32) for _ in range(n)]
            ds = capi.DescSet(ctx, descs)
            rec = dict(base, route="match")
            for label, pr in (("all_pairs", scene.all_pairs(n)), ("kept_pairs", pairs)):
                ts = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    res = ds.match_pairs(pr)
                    ctx.synchronize()
                    ts.append(time.perf_counter() - t0)
                    res.close()
                rec[label] = dict(pairs=len(pr), wall_ms=round(float(np.median(ts[1:])) * 1e3, 3))
            ds.close()
            del descs
            emit(rec, a.out)
    ctx.close()


if __name__ == "__main__":
    main()
