"""Timing of the visual words on the device (msfm_descset_words) against the one-thread C++ restatement.

  python scripts/words_bench.py [--reps 9] [--out FILE (default profiles/words_bench.jsonl, rewritten)] [--cpu-images 8] [--only NAME]
                                [--label TEXT] [--levels 6] [--append]

The tree is synthetic and made here: k = 10, six blocks deep (111 111 blocks, 10^6 words, 569 MB of node descriptors), integer
descriptors drawn uniformly from 0 .. 255, so a descent takes a random path and the last level's blocks are gathered from all
over the table.  Workloads: c3 = config 3's shape, 500 images x 4 096 features; c5_200 = the first 200 images of config 5's
shape, 4 096 features each.  Per workload one JSON line:
  wall time of DescSet.words (the call and its one wait), median / min / max of --reps after a warm-up; the words_* kernel
  classes of one further profiled run; bytes sent (the tree once, at msfm_voctree_create; per call the tables of the set);
  tests/words_ref.cpp on one thread of this host over the first --cpu-images images, and that time scaled to all images
  (marked extrapolated); whether its words equal the device's on those images.
--label names the build that was measured (a variant under test); the machine and its GPU are named in the first line."""
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
from tests import words_data as D  # noqa: E402

WORKLOADS = {"c3": dict(n=500, feats=4096), "c5_200": dict(n=200, feats=4096)}
K, LEVELS = 10, 6
LEAF = 0x80000000


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def box():
    gpu = "unknown"
    try:
        txt = subprocess.run(["/opt/rocm/bin/rocminfo"], capture_output=True, text=True, timeout=60).stdout
        m = re.search(r"Marketing Name:\s*(AMD Instinct[^\n]*)", txt) or re.search(r"Name:\s*(gfx\w+)", txt)
        gpu = m.group(1).strip() if m else gpu
    except Exception:
        pass
    return dict(host=socket.gethostname(), gpu=gpu)


def synthetic_tree(levels=LEVELS, seed=0x30d5):
    """Heap numbering: node i of block b links block 10 b + i + 1; the blocks of the last level hold the leaves, word = their rank."""
    rng = np.random.Generator(np.random.PCG64(seed))
    inner = sum(K ** l for l in range(levels - 1))
    nb = inner + K ** (levels - 1)
    link = np.zeros((nb, K), np.uint32)
    link[:inner] = (np.arange(inner, dtype=np.uint32)[:, None] * K + np.arange(K, dtype=np.uint32)[None, :] + 1)
    link[inner:] = (np.arange((nb - inner) * K, dtype=np.uint32) | np.uint32(LEAF)).reshape(-1, K)
    desc = rng.integers(0, 256, size=(nb, K, 128), dtype=np.uint8).astype(np.float32)
    weight = rng.uniform(0.5, 1.5, size=(nb, K)).astype(np.float32)
    return dict(k=K, block_n=np.full(nb, K, np.uint16), node_desc=desc, node_link=link, node_weight=weight)


def stats(ts):
    return dict(wall_ms=round(float(np.median(ts)) * 1e3, 3), wall_ms_min=round(min(ts) * 1e3, 3), wall_ms_max=round(max(ts) * 1e3, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--cpu-images", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "words_bench.jsonl"))
    ap.add_argument("--only", default=None)
    ap.add_argument("--label", default="as committed")
    ap.add_argument("--append", action="store_true", help="add to --out instead of rewriting it")
    ap.add_argument("--levels", type=int, default=LEVELS, help="blocks on a path of the synthetic tree (5: a tree of 57 MB, to price the last level)")
    a = ap.parse_args()
    from metricsfm_amd import capi
    ctx = capi.Context(0)   # fails without a GPU: nothing here is measured on a CPU fallback
    if a.out and not a.append:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()
    emit(dict(what="words_bench", box=box(), reps=a.reps, label=a.label, tree=dict(k=K, levels=a.levels)), a.out)
    tree = synthetic_tree(a.levels)
    t0 = time.perf_counter()
    vt = ctx.voctree(tree["k"], tree["block_n"], tree["node_desc"], tree["node_link"], tree["node_weight"])
    t_tree = time.perf_counter() - t0
    tsize = vt.size()
    tmp = tempfile.mkdtemp()
    exe = os.path.join(tmp, "words_ref")
    if a.cpu_images:
        D.build_ref_cpp(exe)
    for name, shape in WORKLOADS.items():
        if a.only and name != a.only:
            continue
        n, feats = shape["n"], shape["feats"]
        rng = np.random.Generator(np.random.PCG64(0x30d6))
        descs = [rng.integers(0, 256, size=(feats, 128), dtype=np.uint8).astype(np.float32) for _ in range(n)]
        ds = capi.DescSet(ctx, descs)
        res = ds.words(vt)      # warm-up
        size = res.size()
        first = res.fetch()
        res.close()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            res = ds.words(vt)
            ts.append(time.perf_counter() - t0)
            res.close()
        ctx.profile(True); ctx.profile_reset()
        res = ds.words(vt)
        prof = ctx.profile_get()
        res.close()
        ctx.profile(False); ctx.profile_reset()
        rec = dict(workload=name, label=a.label, n=n, feats=feats, words=stats(ts), features=size["n_features"], n_bow=size["n_bow"],
                   num_words=size["num_words"], n_unassigned=size["n_unassigned"],
                   kernels_ms={k: round(v["total_ms"], 3) for k, v in prof.items() if k.startswith("words_")},
                   tree_h2d_bytes=tsize["h2d_bytes"], tree_create_ms=round(t_tree * 1e3, 1),
                   call_h2d_bytes=8 * n + 4 * (n + 1) + n)   # the row pointers, feat_off, has_words: what msfm_descset_words uploads
        if a.cpu_images:
            m = min(a.cpu_images, n)
            want, seconds = D.run_ref_cpp(exe, tmp, tree, descs[:m], 300)
            rec.update(cpu_one_thread_images=m, cpu_one_thread_ms=round(seconds * 1e3, 1),
                       cpu_one_thread_ms_all_images_extrapolated=round(seconds * 1e3 * n / m, 1),
                       cpu_words_equal_device=bool(np.array_equal(want["word_id"], first["word_id"][:m * feats])))
        emit(rec, a.out)
        ds.close()
        del descs
    vt.close()
    ctx.close()


if __name__ == "__main__":
    main()
