"""Timing of the start of a model: from the ranked pair list to the adjusted seed model, resident against the route that
existed before msfm_recon_create_from_seed.

  python scripts/seedstart_bench.py [--reps 9] [--out FILE (default profiles/seedstart_bench.jsonl, rewritten)]

Workload: a store made from a chain (the keypoints inside it) with K = 64 image pairs; K - 1 pairs of 2 100 points fail the
gates after the full work and rank first, the pair of 2 000 points passes.  One JSON line each:
  resident  incremental.start_model(ResidentBackend): seed.find_seed_pair(keep=True), Recon.from_seed, Recon.normalize with noise,
            the camera side on the host, Recon.set_cameras, Recon.adjust(full, outliers)
  host      the same result by the earlier route: seed.find_seed_pair with the match callback (Chain.fetch_matches: a
            download of what is resident), incremental.state_from_seed, normalize_points / normalize_cameras on the host,
            Context.recon (the upload), Recon.adjust(full, outliers)
            wall time around the whole route with every wait inside (median, min, max of --reps after a warm-up), the bytes
            sent, and the kernel split of msfm_ctx_profile_get from one further profiled run
  normalize the two kernels of msfm_recon_normalize alone at P = 2 000 and P = 60 000 (the reference's feature cap per image,
            the worst case of the ordered sum): medians of the event-pair times over --reps profiled calls
The machine and its GPU are named in the first line."""
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
from tests import seed_data as D  # noqa: E402
from tests import seedstart_data as SD  # noqa: E402

K, N_WIN, N_FAIL, NOISE_SEED = 64, 2000, 2100, 7


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


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return dict(wall_ms=round(float(np.median(ts)) * 1e3, 3), wall_ms_min=round(min(ts) * 1e3, 3), wall_ms_max=round(max(ts) * 1e3, 3))


def profiled(ctx, fn):
    ctx.profile(True); ctx.profile_reset()
    out = fn()
    prof = ctx.profile_get()
    ctx.profile(False); ctx.profile_reset()
    return out, {k: round(v["total_ms"], 4) for k, v in prof.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seedstart_bench.jsonl"))
    a = ap.parse_args()
    from metricsfm_amd import capi, incremental, seed
    ctx = capi.Context(0)   # fails without a GPU: nothing here is measured on a CPU fallback
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()
    emit(dict(what="seedstart_bench", box=box(), reps=a.reps, K=K, matches=N_WIN), a.out)
    specs = [dict(n=N_FAIL, kw=dict(baseline=2.0, **D.EXACT))] * (K - 1) + [dict(n=N_WIN, kw=dict(outlier_frac=0.0))]
    st, ch, n_m, kps, close = SD.chain_pairs(ctx, specs, 101)
    n = 2 * K
    graph = np.zeros((n, n), np.int32)
    graph[2 * np.arange(K), 2 * np.arange(K) + 1] = n_m
    pair_index = {(2 * h, 2 * h + 1): h for h in range(K)}
    book_args = dict(match_count=graph, image_f=np.full(n, D.F), image_f_init=np.full(n, D.F))

    def resident():
        book = incremental.Book(**book_args)
        backend, rec = incremental.start_model(incremental.ResidentBackend, ctx, st, book, noise_seed=NOISE_SEED)
        z = backend.recon.size()
        state = backend.fetch() if resident.fetch else None
        backend.close()
        return rec, z["h2d_bytes"], state

    def host():
        s = seed.find_seed_pair(ctx, st, graph, np.zeros(n, bool), np.full(n, D.F), np.arange(n), pair_matches=lambda i, j: ch.fetch_matches(pair_index[(i, j)]),
                                image_keypoints=lambda i: kps[i])
        state = incremental.state_from_seed(s, st.n_features)
        P = len(s["point"])
        rng = np.random.default_rng(NOISE_SEED)
        noise_p, noise_c = rng.standard_normal((P, 3)), rng.standard_normal((2, 2, 3))
        mid, scale, state["point_xyz"] = incremental.normalize_points(state["point_xyz"], noise_p)
        pose, state["cam_R"], state["cam_t"], state["cam_c"] = incremental.normalize_cameras(s["cam_pose"], s["cam_c"], mid, scale, noise_c)
        q = ctx.recon(st, state, pose, s["cam_model"], s["cam_model_of_cam"])
        r = q.adjust(-1, [], partial=False, full=True, outliers=True)
        z = q.size()
        out = q.fetch() if resident.fetch else None
        q.close()
        return dict(images=s["images"], n_visited=s["n_visited"], n_points=P, summary=r["summary"]), z["h2d_bytes"] + s["hypotheses"]["h2d_bytes"], out

    resident.fetch = True
    (ra, _, sa), (rb, _, sb) = resident(), host()
    equal = all(np.array_equal(np.asarray(sa[k]), np.asarray(sb[k])) for k in sb if k in sa)
    resident.fetch = False
    for name, fn in (("resident", resident), ("host", host)):
        t = timed(fn, a.reps)
        (rec, sent, _), prof = profiled(ctx, fn)
        solve = rec["summary"][1]
        emit(dict(route=name, **t, images=[int(i) for i in rec["images"]], n_visited=int(rec["n_visited"]), points=int(rec["n_points"]),
                  h2d_bytes_behind_the_seed_call=int(sent), solve_iterations=int(solve["num_iterations"]), solve_ms=round(solve["solve_ms"], 3),
                  setup_ms=round(solve["setup_ms"], 3), kernels_ms=prof, states_equal=bool(equal)), a.out)
    close()
    # the normalisation kernels alone
    st1 = ctx.match_store(np.array([1, 1], np.int32), np.array([[0, 1]], np.int32), np.array([0, 1], np.int32), np.zeros((1, 2), np.int32))
    for P in (2000, 60000):
        rng = np.random.default_rng(P)
        state = dict(cam_img=[0, 1], feat_point=[-1, -1], obs_point=[], obs_cam=[], obs_feat=[], pt_views=np.zeros(P, np.int32), pt_bad=np.zeros(P, np.uint8),
                     pt_mutable=np.ones(P, np.uint8), pt_new_added=np.zeros(P, np.uint8), cam_R=np.tile(np.eye(3), (2, 1, 1)), cam_t=np.zeros((2, 3)),
                     cam_c=np.zeros((2, 3)), cam_fk=np.tile([D.F, 0.0, 0.0], (2, 1)), point_xyz=rng.normal(0, 30, (P, 3)), pt_mse=np.zeros(P))
        q = ctx.recon(st1, state, np.zeros((2, 6)), [[D.F, 0.0, 0.0]], [0, 0], keypoints=np.zeros((2, 2), np.float32))
        noise = rng.standard_normal((P, 3))
        q.normalize(noise)
        sums, write, wall = [], [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            _, prof = profiled(ctx, lambda: q.normalize(noise))
            wall.append(time.perf_counter() - t0)
            sums.append(prof["recon_normalize_sums"]); write.append(prof["recon_normalize_write"])
        emit(dict(route="normalize", points=P, sums_kernel_ms=round(float(np.median(sums)), 4), write_kernel_ms=round(float(np.median(write)), 4),
                  call_wall_ms=round(float(np.median(wall)) * 1e3, 3), noise_bytes=24 * P), a.out)
        q.close()
    st1.close()
    ctx.close()


if __name__ == "__main__":
    main()
