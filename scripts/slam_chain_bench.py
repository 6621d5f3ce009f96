"""Timing of the SLAM arm of the resident chain: from the result of msfm_match_pairs_slam to built tracks.

  python scripts/slam_chain_bench.py [--reps 9] [--out FILE (default profiles/slam_chain_bench.jsonl, rewritten)]
                                     [--configs 2 5] [--c5-images 200] [--features 4096]

Per workload the SLAM points are the scene's own observations (as in scripts/slam_priors_bench.py): msfm_slam_priors gives the
window pairs and their prior F / H, msfm_match_pairs_slam matches them once, outside the timed windows.  Config 5 is taken on its
first --c5-images cameras (default 200: generating the descriptors of all 2 000 images takes minutes and 4 GB of host memory;
--c5-images 2000 is the whole of it); the pairs are the window pairs among those.  Then, in the same process, median / min / max of --reps after a warm-up, one JSON line each:
  chain        msfm_chain_create + msfm_chain_verify_slam + msfm_chain_build_tracks, and the wall time of each of the three
               calls (every one ends in a stream wait); the tracks stay on the device
  host_arrays  what a caller had before: msfm_match_result_fetch of every pair's codes, the survivors gathered on the host,
               msfm_fundamental_ransac_batch on host arrays, kept by mask, msfm_tracks_build_device from host arrays
               (Context.build_tracks, which also downloads the tracks)
with the bytes each route moves over PCIe (counted from the array sizes) and the kernel split of msfm_ctx_profile_get from
one further profiled run.  The track build has no class in that profile (csrc/tracks.hip carries no timer), so its share is
the wall time of msfm_chain_build_tracks, not a kernel time.  The first line names the machine and its GPU."""
import argparse
import json
import os
import re
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from metricsfm_amd import _abi as A  # noqa: E402
from metricsfm_amd import capi, scene, slam  # noqa: E402

SEED = 0x4D53464D46


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


def stats(ts):
    return dict(wall_ms=round(float(np.median(ts)), 3), wall_ms_min=round(min(ts), 3), wall_ms_max=round(max(ts), 3))


def workload(ctx, cfg, n_img, feats):
    sc = scene.config_scene(cfg)
    n_img = sc.n_cams if n_img is None else min(n_img, sc.n_cams)
    sel = sc.obs_cam < n_img                               # the SLAM points: the observations of the first n_img cameras
    order = np.argsort(sc.obs_pt[sel], kind="stable")
    pt, cam, xy = sc.obs_pt[sel][order], sc.obs_cam[sel][order], sc.obs_xy[sel][order]
    toff = np.concatenate([[0], np.cumsum(np.bincount(pt, minlength=sc.n_points))]).astype(np.int32)
    scene.add_features(sc, feats, images=range(n_img))
    kps = [np.ascontiguousarray(sc.kp_xy[i], np.float32) for i in range(n_img)]
    ds = ctx.descset([sc.desc[i] for i in range(n_img)], keypoints=kps)
    th_e, th_d = slam.thresholds(1.0)                      # the scene's observations are at the resolution of its features
    pairs, Fp, Hp, _ = ctx.slam_priors(n_img, toff, cam, xy, th_epipolar=th_e, th_distance=th_d)
    res = ds.match_pairs_slam(pairs, Fp, Hp, th_first_second_ratio=slam.TH_FIRST_SECOND_RATIO, th_epipolar=th_e, th_distance=th_d)
    return n_img, kps, ds, res, pairs


def chain_route(res, laps=None):
    t0 = time.perf_counter()
    ch = capi.Chain(res)
    t1 = time.perf_counter()
    n_m, ok, _ = ch.verify_slam(seed=SEED)
    t2 = time.perf_counter()
    nt, no = ch.build_tracks()
    t3 = time.perf_counter()
    ch.close()
    if laps is not None:
        for k, v in (("chain_create", t1 - t0), ("chain_verify_slam", t2 - t1), ("chain_build_tracks", t3 - t2)):
            laps.setdefault(k, []).append(1e3 * v)
    return n_m, ok, nt, no


def host_route(ctx, res, pairs, kps, n_feat):
    surv = []
    for p in range(len(pairs)):
        code = res.fetch(p)[0]
        m = np.nonzero(code >= 0)[0]
        surv.append(np.column_stack([code[m], m]).astype(np.int32).reshape(-1, 2))
    off = np.concatenate([[0], np.cumsum([len(s) for s in surv])]).astype(np.int32)
    p1 = np.concatenate([kps[i][s[:, 0]] for (i, j), s in zip(pairs, surv)])
    p2 = np.concatenate([kps[j][s[:, 1]] for (i, j), s in zip(pairs, surv)])
    _, inl, _, ok = ctx.fundamental_ransac(off, p1, p2, seed=SEED)
    fin = [surv[p][inl[off[p]:off[p + 1]] != 0] for p in range(len(pairs))]
    moff = np.concatenate([[0], np.cumsum([len(m) for m in fin])]).astype(np.int32)
    flat = (n_feat, A.as_c(pairs, np.int32), moff, A.as_c(np.concatenate(fin).reshape(-1, 2), np.int32))
    toff, _, _ = ctx.build_tracks(None, None, None, flat=flat)
    return np.diff(moff), ok, len(toff) - 1, int(off[-1])


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return r, ts


def profiled(ctx, fn):
    ctx.profile(True); ctx.profile_reset()
    fn()
    prof = ctx.profile_get()
    ctx.profile(False); ctx.profile_reset()
    return {k: dict(ms=round(v["total_ms"], 4), launches=v["launches"]) for k, v in sorted(prof.items()) if v["launches"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slam_chain_bench.jsonl"))
    ap.add_argument("--configs", type=int, nargs="+", default=[2, 5])
    ap.add_argument("--c5-images", type=int, default=200)
    ap.add_argument("--features", type=int, default=4096)
    a = ap.parse_args()
    ctx = capi.Context(0)   # fails without a GPU: nothing here is measured on a CPU fallback
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()
    emit(dict(what="slam_chain_bench", box=box(), reps=a.reps), a.out)
    for cfg in a.configs:
        n_img, kps, ds, res, pairs = workload(ctx, cfg, a.c5_images if cfg == 5 else None, a.features)
        n_feat = np.array([len(k) for k in kps], np.int32)
        laps = {}
        (n_c, ok_c, nt_c, no_c), ts_c = timed(lambda: chain_route(res, laps), a.reps)
        calls_ms = {k: round(float(np.median(v[1:])), 3) for k, v in laps.items()}      # (the first pass warms up)
        (n_h, ok_h, nt_h, n_surv), ts_h = timed(lambda: host_route(ctx, res, pairs, kps, n_feat), a.reps)
        P, Q, S, M = len(pairs), int(n_feat[pairs[:, 1]].sum()), n_surv, int(n_c.sum())
        shape = dict(config=cfg, images=n_img, features=int(n_feat.sum()), pairs=P, queries=Q, survivors=S, matches=M, pairs_ok=int(ok_c.sum()),
                     pairs_kept_without_verdict=int(((ok_c == 0) & (n_c > 0)).sum()), tracks=nt_c, observations=no_c)
        same = bool(np.array_equal(n_c, n_h) and np.array_equal(ok_c, ok_h) and nt_c == nt_h)
        # PCIe bytes, from the array sizes: the chain moves per-pair integers and matrices only
        chain_bytes = dict(h2d=32 * P + 4 * (P + 1) * 2 + 8 * P + 4 * (2 * len(n_feat) + 1), d2h=P * (8 + 4 + 1 + 72))
        host_bytes = dict(h2d=4 * (P + 1) + 16 * S + 4 * len(n_feat) + 8 * P + 4 * (P + 1) + 8 * M, d2h=4 * Q + S + P * (72 + 4 + 1))
        emit(dict(shape, route="chain", **stats(ts_c), calls_wall_ms=calls_ms, pcie_bytes=chain_bytes, kernels=profiled(ctx, lambda: chain_route(res))), a.out)
        emit(dict(shape, route="host_arrays", **stats(ts_h), pcie_bytes=host_bytes, same_result=same,
                  kernels=profiled(ctx, lambda: host_route(ctx, res, pairs, kps, n_feat))), a.out)
        emit(dict(config=cfg, summary="chain / host_arrays", wall_ratio=round(float(np.median(ts_c) / np.median(ts_h)), 3)), a.out)
        res.close(); ds.close()
    ctx.close()


if __name__ == "__main__":
    main()
