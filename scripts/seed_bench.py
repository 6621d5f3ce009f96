"""Timing of the batched seed-pair call (msfm_seed_hypotheses) against what existed before it.

  python scripts/seed_bench.py [--reps 9] [--out FILE (default profiles/seed_bench.jsonl, rewritten)] [--no-cpu]

Workloads: K in {1, 16, 64} hypotheses of {500, 2000} matches, all on the five-point arm (known focal lengths) or all on the
eight-point arm.  K - 1 image pairs fail the gates after the full work (pose, every match triangulated) and the pair the
ranking puts last passes, so a walk that stops at the winner answers K hypotheses too.  Per workload, one JSON line each:
  batched   one Context.seed_hypotheses call on the resident store: wall time around the call, which ends in its device
            synchronise and includes the fetch into numpy arrays (median, min, max of --reps after a warm-up call), the
            kernel split of msfm_ctx_profile_get from one further profiled call, h2d_bytes
  mirror    tests/seed_host_check.cc in a child process: the C++ host's FindSeedPairThenReconstruct (ranking + one batched
            call + adopting the winner) and (a) its one-hypothesis-at-a-time walk FindSeedPairThenReconstructHost through
            msfm_relpose_5pt_batch / msfm_relpose_8pt_batch / msfm_triangulate_midpoint_batch on host arrays; median of 5
  cpu       (b) the sequential restatement on one CPU thread: the pose oracles and tests/seed_ref.cpp (one run)
  summary   per arm and match count: K = 64 against 64 x (K = 1), and the mirror's batched search against its walk (a)
The machine and its GPU are named in the first line.  Stores, cases and the C++ driver are built outside the timed windows."""
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
from tests import seed_data as D  # noqa: E402

KS, SIZES, ARMS = (1, 16, 64), (500, 2000), (5, 8)


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def workload(K, n, arm):
    """K pairs: K - 1 with n matches that fail the gates, then one with n - 1 matches that passes (ranked last: the strength
    of a pair whose images match nothing else grows with its match count)."""
    if arm == 5:
        fail = dict(n=n, f=(D.F, D.F), kw=dict(baseline=2.0, **D.EXACT))            # every angle under 3 degrees
        good = dict(n=n - 1, f=(D.F, D.F), kw=D.EXACT)
    else:
        fail = dict(n=n, f=(0.0, 0.0), same=True, kind="generic")                     # large rotation: the reprojection gate fails
        good = dict(n=n - 1, f=(0.0, 0.0), same=True, kind="generic", kw=dict(f_cur=4800.0, **D.SMALL_ROT))
    return D.build_case([fail] * (K - 1) + [good], 1000 + K + n + arm)


def box():
    gpu = "unknown"
    try:
        txt = subprocess.run(["/opt/rocm/bin/rocminfo"], capture_output=True, text=True, timeout=60).stdout
        m = re.search(r"Marketing Name:\s*(AMD Instinct[^\n]*)", txt) or re.search(r"Name:\s*(gfx\w+)", txt)   # (no marketing name in a container)
        gpu = m.group(1).strip() if m else gpu
    except Exception:
        pass
    return dict(host=socket.gethostname(), gpu=gpu)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seed_bench.jsonl"))
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    from metricsfm_amd import capi
    ctx = capi.Context(0)   # fails without a GPU: nothing here is measured on a CPU fallback
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()
    wall, mirror = {}, {}
    emit(dict(what="seed_bench", box=box(), reps=a.reps), a.out)
    tmp = tempfile.mkdtemp()
    exe = os.path.join(tmp, "seed_host_check")
    subprocess.check_call(D.host_check_command(exe))
    refs = None
    if not a.no_cpu:
        from oracle import oracle as O
        from tests import relposef_data as RF
        from tests import seed_ref as SR
        O.build()
        refs = (O, RF.build_ref(tmp), SR.build_ref(tmp))
    for arm in ARMS:
        for n in SIZES:
            for K in KS:
                c = workload(K, n, arm)
                st = ctx.match_store(*D.store_args(c))
                call = lambda: ctx.seed_hypotheses(st, c["hyp_img"], c["cam_fk"], c["same_model"], keypoints=c["keypoints"])  # noqa: E731
                r = call()
                ts = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    call()
                    ts.append(time.perf_counter() - t0)
                ctx.profile(True); ctx.profile_reset()
                call()
                prof = ctx.profile_get()
                ctx.profile(False); ctx.profile_reset()
                st.close()
                base = dict(arm=arm, K=K, matches=n)
                wall[(arm, n, K)] = float(np.median(ts)) * 1e3
                emit(dict(base, route="batched", wall_ms=round(float(np.median(ts)) * 1e3, 3), wall_ms_min=round(min(ts) * 1e3, 3),
                          wall_ms_max=round(max(ts) * 1e3, 3), winner=int(r["winner"]), points=np.diff(r["pt_off"]).tolist()[-3:],
                          h2d_bytes=int(r["h2d_bytes"]), kernels_ms={k: round(v["total_ms"], 3) for k, v in prof.items()}), a.out)
                src, dst = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
                nimg = len(c["n_features"])
                D.write_image_set(src, c, np.full(nimg, D.F if arm == 5 else 0.0), np.arange(nimg) // 2 if arm == 8 else np.arange(nimg), 64)
                run = subprocess.run([exe, src, dst, "time"], capture_output=True, text=True, timeout=600)
                m = re.search(r"time_ms batched ([\d.]+) walk ([\d.]+) visited (\d+)", run.stdout)
                if run.returncode != 0 or not m:
                    emit(dict(base, route="mirror", error=(run.stdout + run.stderr)[-400:]), a.out)
                else:
                    mirror[(arm, n, K)] = (float(m.group(1)), float(m.group(2)))
                    emit(dict(base, route="mirror", batched_ms=float(m.group(1)), walk_one_at_a_time_ms=float(m.group(2)), visited=int(m.group(3))), a.out)
                if refs:
                    t0 = time.perf_counter()
                    w = D.expected(*refs, c)
                    emit(dict(base, route="cpu_restatement_one_thread", wall_ms=round((time.perf_counter() - t0) * 1e3, 1),
                              equals_batched=bool(all(np.array_equal(np.asarray(w[k]), np.asarray(r[k])) for k in w))), a.out)
    for arm in ARMS:
        for n in SIZES:
            rec = dict(route="summary", arm=arm, matches=n, K64_ms=round(wall[(arm, n, 64)], 3), K1_ms=round(wall[(arm, n, 1)], 3),
                       K1_times_64_ms=round(64 * wall[(arm, n, 1)], 3), K64_over_64xK1=round(wall[(arm, n, 64)] / (64 * wall[(arm, n, 1)]), 4))
            if (arm, n, 64) in mirror:
                b, w = mirror[(arm, n, 64)]
                rec.update(mirror_batched_ms=b, mirror_walk_ms=w, walk_over_batched=round(w / b, 2), batched_beats_walk=bool(b < w))
            emit(rec, a.out)
    ctx.close()


if __name__ == "__main__":
    main()
