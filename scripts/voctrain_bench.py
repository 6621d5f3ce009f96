"""Timing of the vocabulary training on the device (msfm_descset_voctree_train) against the one-thread C++ restatement, and of the
resident hand-over train -> words against read_voctree -> upload -> words for the same tree.

  python scripts/voctrain_bench.py [--reps 9] [--out FILE (default profiles/voctrain_bench.jsonl, rewritten)] [--cpu-images 8]
                                   [--only NAME] [--label TEXT] [--append]

Workloads: c3 = config 3's shape, 500 images x 4 096 features; c5_200 = the first 200 images of config 5's shape, 4 096 features
each; k = 10, levels = 6, image_step = 1.  The descriptors are synthetic, integer-valued and clustered on three scales (10 x 10 x
10 centres and noise), because uniform noise has nothing to converge on and every node would run to max_iters.  Per workload
one JSON line:
  wall time of DescSet.train_voctree (the call with all its waits), median / min / max of --reps after a warm-up; the voctrain_*
  kernel classes of one further profiled run (event pairs of the library); the stats (iterations per level, nodes, host waits);
  bytes sent by the call (the sample's two tables) and by the tree (none);
  tests/voctrain_ref.cpp on one thread of this host over the first --cpu-images images, that time scaled by the feature count
  to all images (marked extrapolated: deeper levels of a larger sample split more nodes, so the scaling is a lower bound), and
  whether the device trains the same tree from those images;
  hand-over: train_voctree + words (resident) against read_voctree + Context.voctree + words for the same tree from a file.
--label names the build that was measured; the machine and its GPU are named in the first line."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from tests import voctrain_data as D  # noqa: E402
from tests import voctrain_ref as V  # noqa: E402
from words_bench import box, emit, stats  # noqa: E402

WORKLOADS = {"c3": dict(n=500, feats=4096), "c5_200": dict(n=200, feats=4096)}
K, LEVELS = 10, 6
TREE_KEYS = ("k", "block_n", "node_desc", "node_link", "node_weight")


def clustered_images(n, feats, seed=0x7a12):
    """Integer descriptors in [0, 255]: 10 centres, 10 offsets of +-24 around each, 10 of +-8 around those, noise of +-2."""
    rng = np.random.Generator(np.random.PCG64(seed))
    top = rng.integers(48, 208, (10, 128)).astype(np.int16)
    mid = rng.integers(-24, 25, (10, 10, 128)).astype(np.int16)
    low = rng.integers(-8, 9, (10, 10, 10, 128)).astype(np.int16)
    cent = (top[:, None, None] + mid[:, :, None] + low).reshape(1000, 128)
    out = []
    for _ in range(n):
        pick = rng.integers(0, 1000, feats)
        out.append(np.clip(cent[pick] + rng.integers(-2, 3, (feats, 128), dtype=np.int16), 0, 255).astype(np.float32))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--cpu-images", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voctrain_bench.jsonl"))
    ap.add_argument("--only", default=None)
    ap.add_argument("--label", default="as committed")
    ap.add_argument("--append", action="store_true", help="add to --out instead of rewriting it")
    a = ap.parse_args()
    from metricsfm_amd import capi, featurefiles
    ctx = capi.Context(0)   # fails without a GPU: nothing here is measured on a CPU fallback
    if a.out and not a.append:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()
    emit(dict(what="voctrain_bench", box=box(), reps=a.reps, label=a.label, options=dict(k=K, levels=LEVELS, max_iters=11, image_step=1, seed=0)), a.out)
    tmp = tempfile.mkdtemp()
    exe = os.path.join(tmp, "voctrain_ref")
    if a.cpu_images:
        D.build_ref_cpp(exe)
    for name, shape in WORKLOADS.items():
        if a.only and name != a.only:
            continue
        n, feats = shape["n"], shape["feats"]
        descs = clustered_images(n, feats)
        ds = capi.DescSet(ctx, descs)
        opt = dict(k=K, levels=LEVELS, seed=0)
        vt = ds.train_voctree(**opt)      # warm-up
        st, size = vt.stats, vt.size()
        vt.close()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            vt = ds.train_voctree(**opt)
            ts.append(time.perf_counter() - t0)
            vt.close()
        ctx.profile(True); ctx.profile_reset()
        vt = ds.train_voctree(**opt)
        prof = ctx.profile_get()
        vt.close()
        ctx.profile(False); ctx.profile_reset()
        n_img = st["n_images"]
        rec = dict(workload=name, label=a.label, n=n, feats=feats, train=stats(ts), features=st["n_features"], n_blocks=st["n_blocks"],
                   n_leaves=st["n_leaves"], depth=st["depth"], level_nodes=st["level_nodes"], level_split=st["level_split"],
                   level_max_iters=st["level_max_iters"], level_capped=st["level_capped"], host_waits=st["host_waits"],
                   weight_shift=st["weight_shift"], sum_shift=st["sum_shift"],
                   kernels_ms={k: round(v["total_ms"], 3) for k, v in prof.items() if k.startswith("voctrain_")},
                   tree_h2d_bytes=size["h2d_bytes"], call_h2d_bytes=8 * n_img + 4 * (n_img + 1) + 4,   # row pointers, offsets, the root's count
                   tree_bytes=int(size["n_blocks"]) * K * (512 + 8) + 2 * int(size["n_blocks"]))
        if a.cpu_images:
            m = min(a.cpu_images, n)
            want, want_st, seconds = D.run_ref_cpp(exe, tmp, descs[:m], **opt)
            sub = capi.DescSet(ctx, descs[:m])
            vs = sub.train_voctree(**opt)
            same = V.same_tree(want, vs.fetch()) is None and V.same_stats(want_st, vs.stats) is None
            t0 = time.perf_counter()
            vs2 = sub.train_voctree(**opt)
            t_sub = time.perf_counter() - t0
            vs.close(); vs2.close(); sub.close()
            rec.update(cpu_one_thread_images=m, cpu_one_thread_ms=round(seconds * 1e3, 1), device_ms_same_images=round(t_sub * 1e3, 3),
                       cpu_one_thread_ms_all_images_extrapolated=round(seconds * 1e3 * n / m, 1), cpu_tree_equals_device=bool(same))
        # the hand-over: a tree that stays on the device against the same tree read from a file and uploaded
        vt = ds.train_voctree(**opt)
        path = os.path.join(tmp, "voctree_" + name)
        featurefiles.write_voctree(path, **vt.fetch())
        vt.close()
        vt = ds.train_voctree(**opt)
        res = ds.words(vt)      # warm-up of the words call
        res.close(); vt.close()
        t_res, t_words, t_file, t_read, t_up = [], [], [], [], []
        for _ in range(3):
            t0 = time.perf_counter()
            vt = ds.train_voctree(**opt)
            t1 = time.perf_counter()
            res = ds.words(vt)
            t_res.append(time.perf_counter() - t0)
            t_words.append(time.perf_counter() - t1)
            first = res.fetch()["word_id"]
            res.close(); vt.close()
            t0 = time.perf_counter()
            tree = featurefiles.read_voctree(path)
            t1 = time.perf_counter()
            vu = ctx.voctree(**{key: tree[key] for key in TREE_KEYS})
            t2 = time.perf_counter()
            res = ds.words(vu)
            t_file.append(time.perf_counter() - t0)
            t_read.append(t1 - t0); t_up.append(t2 - t1)
            second = res.fetch()["word_id"]
            res.close(); vu.close()
            del tree
        rec.update(handover=dict(train_words_ms=round(float(np.median(t_res)) * 1e3, 3), words_ms=round(float(np.median(t_words)) * 1e3, 3), read_upload_words_ms=round(float(np.median(t_file)) * 1e3, 3),
                                 read_ms=round(float(np.median(t_read)) * 1e3, 3), upload_ms=round(float(np.median(t_up)) * 1e3, 3),
                                 words_equal=bool(np.array_equal(first, second)), file_bytes=os.path.getsize(path)))
        os.remove(path)
        emit(rec, a.out)
        ds.close()
        del descs
    ctx.close()


if __name__ == "__main__":
    main()
