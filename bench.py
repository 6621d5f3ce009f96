#!/usr/bin/env python3
"""bench.py — BA iterations/s + Mmatches/s on BASELINE.json's headline configuration.

  python bench.py --gpus 1 --steps K --warmup W [--dump-outputs DIR] [--full]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

One "step" = one Levenberg–Marquardt iteration (linearise if the last step was accepted, build the Schur complement,
factor + solve the reduced camera system, back-substitute, evaluate the trial cost) of the 500-camera / 200k-point /
1.2M-observation synthetic scene (BASELINE config 3), problem resident in HBM.  Rank 0 prints ONE JSON line.  A plain run
does only what the headline needs: scene, W warm-up iterations, K timed iterations, the line (`value` = BA iterations/s,
`ms_per_step` = ms per timed iteration).

  --full                the same line also carries the other half of the metric — exhaustive 2-NN + ratio tests over ALL
                        249 500 ordered image pairs of the scene (integer SIFT-like descriptors, and once more on non-integral
                        VLFeat-style floats) — plus the triangulation / reprojection, geometric-verification and pose-initialiser
                        legs, the per-kernel profiled pass with `roofline` for the dominant BA kernel, the one-shot solve and
                        `cpu_baseline` (the CPU oracle on the host's cores: 1 thread and all cores)
  --dump-outputs DIR    after the timed iterations, what they computed as DIR/<name>.npy (float64): the adjusted cam_pose,
                        cam_model and point arrays (rank 0's points when N > 1), the per-iteration cost and [initial, final] cost
                        (of the last run of at most STEP_CHUNK iterations: K steps are timed as such runs from one start state)
  --config 5 --window   BASELINE config 5: partial bundle adjustment of the newest of 2000 cameras (window chosen by the
                        host as PartialBundleAdjustment does, one CameraModel per camera, GPS rows on the window)
"""
import argparse
import hashlib
import json
import os
import sys
import time

os.environ.setdefault("OMP_WAIT_POLICY", "passive")   # the CPU-baseline legs must not spin on cores the job does not own

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from metricsfm_amd import _abi as A  # noqa: E402
from metricsfm_amd import capi, scene, shard, window  # noqa: E402

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (~6.3 TB/s achievable)
BF16_PEAK_TFLOPS = 2500.0      # MI355X_MICROARCH.md: ~2.5 PF dense bf16 / f16 MFMA
I8_PEAK_TOPS = 5000.0          # MI355X_MICROARCH.md: I8 32x32x32 = 2x the bf16 rate per clock
FP64_PEAK_TFLOPS = 78.6        # vendor FP64 vector = matrix figure (not in the micro-arch guide)


def fixed_iteration_options(steps):
    """Exactly `steps` LM iterations: stopping rules off (negative tolerances can never fire)."""
    return capi.default_options(max_num_iterations=steps, function_tolerance=-1.0, gradient_tolerance=-1.0,
                                parameter_tolerance=-1.0, max_num_consecutive_invalid_steps=1 << 30,
                                min_trust_region_radius=0.0)


# The one stopping rule that cannot be switched off: once a solve has converged every step is rejected, each rejection divides
# the trust-region radius by a factor that doubles every time, and some 46 rejections in a row take it to 0 (MIN_RADIUS) - a
# run asked for more iterations than that ends early.  K steps are therefore timed as runs of at most STEP_CHUNK iterations,
# each from the same start state: every timed step is an iteration of the same LM trajectory whatever K is, and K <= STEP_CHUNK
# is one run as before.  (Fixed-iteration solves end by themselves after 69 / 182 / 1282 iterations at configs 1 / 2 / 3; the
# config 5 problems run past 3000.)
STEP_CHUNK = 50


def ba_algorithmic_bytes(n_obs, n_pts, n_cams, n_red):
    """SURVEY.md §8d per-LM-iteration algorithmic HBM bytes (n_red = order of the reduced system)."""
    jac = n_obs * (16 + 8) + n_pts * (24 + 24 + 8) + n_cams * 96
    trial = n_obs * 24 + n_pts * 24
    return jac + trial + 2 * n_red * n_red * 8


def ba_schur_build_flops(k, b=9):
    """SURVEY.md §8d Schur-build flops per LM iteration: sum over the points of
    k_p (2*2*b^2/2 + 2*2*b*3 + 2*2*9/2) + k_p^2 (2*b*3*3 + 2*b*3*b), k = observations per point (array), b = 9."""
    k = np.asarray(k, dtype=np.float64)
    return float((k * (2 * 2 * b * b / 2 + 2 * 2 * b * 3 + 2 * 2 * 9 / 2) + k * k * (2 * b * 3 * 3 + 2 * b * 3 * b)).sum())


def kernel_source_hash():
    """Identifies the kernels a PMC collection was made with (profiles/pmc_traffic.json carries the same hash): the GPU box
    has no git history, so the sources themselves are hashed."""
    h = hashlib.sha256()
    d = os.path.join(ROOT, "metricsfm_amd", "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith((".hip", ".h")):
            h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:16]


_T0 = time.time()


def log(msg):
    """Progress on stderr (rank 0): a long default run must keep writing, or the harness takes it for hung."""
    if int(os.environ.get("RANK", "0")) == 0:
        print("[bench %7.1f s] %s" % (time.time() - _T0, msg), file=sys.stderr, flush=True)


def spawn_ranks(n_gpus, argv=None):
    """`python bench.py --gpus N` without a launcher: run `python -m torch.distributed.run --nproc-per-node N bench.py <same flags>`
    as a child process (never exec: this process may not be replaced once a GPU library is loaded) on a free local port."""
    import socket
    import subprocess
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n_gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + list(sys.argv[1:] if argv is None else argv)
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # (30 / 3 since round 5: a run starts with one evaluation + the Jacobi scaling, ~0.4 ms that ten timed iterations carried as 4 %
    #  of their time and thirty carry as 1.3 %; the reference caps a solve at 100 iterations, test_sfm.cc:35-36)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", type=int, default=3, help="BASELINE config number (3 = headline)")
    ap.add_argument("--window", action="store_true", help="config 5: the partial bundle adjustment of the newest camera")
    ap.add_argument("--match-images", type=int, default=0, help="images in the matching legs (0 = every image of the scene)")
    ap.add_argument("--match-steps", type=int, default=2, help="timed passes over the whole pair list")
    ap.add_argument("--feats", type=int, default=4096)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-matching", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="skip the triangulation / verification / pose-initialiser legs")
    ap.add_argument("--verify-pairs", type=int, default=2048, help="image pairs in the geometric-verification leg")
    ap.add_argument("--pose-images", type=int, default=1024, help="images / pairs in the pose-initialiser leg")
    ap.add_argument("--chain-images", type=int, default=96, help="images in the resident-chain leg (all their ordered pairs)")
    ap.add_argument("--backend", default=None, help="torch.distributed backend for N>1 (default nccl = RCCL)")
    ap.add_argument("--full", action="store_true",
                    help="every leg beyond the headline: profiled pass + rooflines, one-shot solve, matching, extras, CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the timed iterations computed as DIR/<name>.npy")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1 and "RANK" not in os.environ:
            # started as a plain `python bench.py --gpus N`: start the N ranks as CHILD processes (one per GPU, RCCL) before
            # anything in this process touches the GPU, pass rank 0's JSON line through and exit with the launcher's code
            sys.exit(spawn_ranks(args.gpus))
        raise SystemExit("WORLD_SIZE %d != --gpus %d" % (world, args.gpus))

    # torch only carries the collectives of N > 1 ranks: one rank leaves the GPU to the library alone and does not pay for
    # importing torch (its first import on a fresh machine can take longer than the whole timed run)
    torch = dist = None
    if world > 1:
        import torch
        import torch.distributed as dist
        # one rank per GPU on the real node; a rehearsal with more ranks than GPUs (gloo, one test GPU) shares devices
        local_rank = local_rank % max(1, torch.cuda.device_count())
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = args.backend or "nccl"
        torch.cuda.set_device(local_rank)
        dist.init_process_group(backend=backend, rank=rank, world_size=world)
        if world > max(1, torch.cuda.device_count()):
            # a rehearsal with more ranks than GPUs: tell the library how many contexts launch on this device at the same time
            os.environ["MSFM_DEVICE_SHARE"] = str(-(-world // max(1, torch.cuda.device_count())))

    ctx = capi.Context(local_rank)
    collective = "none (1 rank)"
    if world > 1:
        if dist.get_backend() == "nccl":
            # the library's own RCCL communicator: ncclAllReduce from C++ on the library's stream, no Python in the LM loop
            shard.init_native_rccl(ctx, dist, rank, world)
            collective = "RCCL ncclAllReduce inside libmsfm (msfm_ctx_init_rccl)"
        else:   # rehearsal on CPU-staged gloo (several ranks sharing one GPU)
            ctx.set_allreduce(shard.make_allreduce(dist, local_rank, ctx), rank, world)
            collective = "torch.distributed %s through the hook (host staged)" % dist.get_backend()

    def barrier():
        ctx.synchronize()
        if world > 1:
            torch.cuda.synchronize()
            dist.barrier()
            torch.cuda.synchronize()

    def max_over_ranks(x):
        if world == 1:
            return x
        t = torch.tensor([x], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    def finish(out):
        log("done")
        if rank == 0:
            print(json.dumps(out))
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()

    # ------------------------------------------------------------------ scene (seeded, identical on every rank)
    t0 = time.time()
    win = None
    if args.window:
        if args.config != 5:
            raise SystemExit("--window is BASELINE config 5")
        # the model is in its adjusted state, the newest camera comes straight from localisation (tests/test_gpu_ba.py)
        sc = scene.config_scene(5, n_models=2000, rot_sigma=2e-4, trans_sigma=0.01, point_sigma=0.02)
        scene.perturb_camera(sc, sc.n_cams - 1)
        # (compact: only the rows that make residual blocks are handed over, as the reference's own loop adds them)
        full, win = window.partial_bundle_adjustment_problem(sc, sc.n_cams - 1, gps=True, compact=True)
        workload = ("BASELINE config 5: partial bundle adjustment (sfm_incremental.cc:917-1014) of the newest of %d cameras / %d points / "
                    "%d observations: window of %d cameras (> 5 shared matches), %d free points, one CameraModel per camera, weight 2.0, "
                    "GPS rows (slam_gps.cc:818-830) on the window, dense-Schur LM, Huber(1)"
                    % (sc.n_cams, sc.n_points, sc.n_obs, int(win["cam_mutable"].sum()), int(win["pt_mutable"].sum())))
    else:
        sc = scene.config_scene(args.config)
        kw = {}
        if sc.gps_xyz is not None:   # config 5 carries GPS rows (slam_gps.cc:818-830, weight :824)
            kw = dict(gps_xyz=sc.gps_xyz, gps_weight=window.gps_weight(sc.n_obs, sc.n_cams))
        full = A.BaArrays.from_scene(sc, **kw)
        workload = ("BASELINE config %d: %d cameras / %d points / %d observations%s, dense-Schur LM, Huber(1)"
                    % (args.config, sc.n_cams, sc.n_points, sc.n_obs, ", GPS rows" if kw else ""))
    gen_s = time.time() - t0
    log("scene generated: " + workload)
    mine = shard.shard_ba_arrays(full, rank, world)  # points (+ their observations) of this rank; cameras replicated
    ba = ctx.ba(mine)
    start = (mine.cam_pose.copy(), mine.cam_model.copy(), mine.point.copy())

    def run_iterations(n):
        """n LM iterations as runs of at most STEP_CHUNK, each from `start` (uploaded outside the timed window): the seconds
        inside the runs (maximum over ranks) and the last run's summary with the step counts of all runs."""
        secs, res, ok, bad = 0.0, None, 0, 0
        for k in [STEP_CHUNK] * (n // STEP_CHUNK) + ([n % STEP_CHUNK] if n % STEP_CHUNK else []):
            ba.upload(*start)
            barrier()
            t0 = time.perf_counter()
            res = ba.run(fixed_iteration_options(k))
            barrier()
            secs += max_over_ranks(time.perf_counter() - t0)
            assert res["num_iterations"] == k, res["termination"]
            ok, bad = ok + res["num_successful_steps"], bad + res["num_unsuccessful_steps"]
        return secs, dict(res, num_iterations=n, num_successful_steps=ok, num_unsuccessful_steps=bad)

    # ------------------------------------------------------------------ BA: warmup, then exactly K iterations
    if args.warmup > 0:
        run_iterations(args.warmup)
    ba_s, res = run_iterations(args.steps)
    n_red = res["num_reduced_params"]
    it_s = args.steps / ba_s
    log("BA: %.1f iterations/s (%.3f ms per LM iteration)" % (it_s, 1e3 * ba_s / args.steps))
    out = dict(metric="BA iterations/sec", value=it_s, unit="iterations/s", n_gpus=world, steps=args.steps,
               warmup=args.warmup, ms_per_step=1e3 * ba_s / args.steps, higher_is_better=True, scaling="strong",
               vs_baseline=None, dtype="f64", data="synthetic",
               config=dict(workload=workload, reduced_system_order=n_red,
                           parallelism="points sharded over %d rank(s), camera block all-reduced" % world, collective=collective,
                           scaling_expectation="matching, verification, triangulation: no collective, rate proportional to N; bundle adjustment at this "
                                               "size is Amdahl-bound - every rank repeats the dense-Schur factorisation of the %d-column camera system "
                                               "(~0.45 of ~0.93 ms per iteration at N = 1): <= 1.6 x at N = 8 by any partitioning (DESIGN.md 5)" % n_red,
                           successful_steps=res["num_successful_steps"], unsuccessful_steps=res["num_unsuccessful_steps"],
                           setup_ms=res["setup_ms"], scene_gen_s=gen_s),
               ba_cost=dict(initial=res["initial_cost"], final=res["final_cost"]))
    if args.dump_outputs and rank == 0:
        # the parameters after the last timed iteration (before any later leg uploads the start state again) and its summary
        cp, cm, pt = ba.download()
        dump = dict(cam_pose=cp, cam_model=cm, point=pt, iteration_cost=res["iterations"]["cost"],
                    cost=np.array([res["initial_cost"], res["final_cost"]]))
        assert sum(a.nbytes for a in dump.values()) <= 64 << 20   # config 5's million points are 24 MB
        os.makedirs(args.dump_outputs, exist_ok=True)
        for name, a in dump.items():
            np.save(os.path.join(args.dump_outputs, name + ".npy"), np.ascontiguousarray(a, dtype=np.float64))
        log("outputs written to %s" % args.dump_outputs)
    if not args.full:
        ba.close()
        finish(out)
        return

    # profiled pass (HIP events per kernel class on the ctx stream) for the roofline figures
    # (two passes, per kernel class the one with the smaller total: the event pairs around every launch make the pass sensitive to
    #  whatever else the box does - one collection of round 5 read 360 us for a kernel that rocprofv3 and the other passes put at 300)
    ba_stats = None
    for _ in range(2):
        ctx.profile(True)
        ctx.profile_reset()
        _, res_p = run_iterations(args.steps)
        st = ctx.profile_get()
        ctx.profile(False)
        if ba_stats is None:
            ba_stats = st
        else:
            for k, v in st.items():
                if k not in ba_stats or (v["launches"] == ba_stats[k]["launches"] and v["total_ms"] < ba_stats[k]["total_ms"]):
                    ba_stats[k] = v

    # the same K iterations as ONE msfm_ba_solve call on the host arrays (what replaces ceres::Solve in the reference):
    # index-structure setup + upload + K iterations + download, on the warm GPU; reported beside `value`, never as it
    # (K capped at STEP_CHUNK: one call cannot run more iterations of the timed trajectory)
    one_shot = None
    if rank == 0 and world == 1:
        tmp = A.BaArrays(full.cam_pose, full.cam_model, full.cam_model_of_cam, full.point, full.obs_cam, full.obs_pt, full.obs_xy, full.pt_weight,
                         cam_mutable=full.cam_mutable, model_mutable=full.model_mutable, pt_mutable=full.pt_mutable, gps_xyz=full.gps_xyz,
                         gps_weight=full.struct.gps_weight)
        os_s = None
        for _ in range(2):   # the incremental loop solves again and again: the second call (device-block cache warm) is the steady state
            tmp.cam_pose[:], tmp.cam_model[:], tmp.point[:] = full.cam_pose, full.cam_model, full.point
            t0 = time.perf_counter()
            r1 = ctx.ba_solve(tmp, fixed_iteration_options(min(args.steps, STEP_CHUNK)))
            dt = time.perf_counter() - t0
            os_s = dt if os_s is None else min(os_s, dt)
        one_shot = dict(ms=1e3 * os_s, iterations=r1["num_iterations"], setup_ms=r1["setup_ms"], iterations_per_s=r1["num_iterations"] / os_s,
                        note="msfm_ba_solve on host arrays (what replaces ceres::Solve): upload + index structures built on the device + "
                             "iterations + download + destroy; best of two calls")

    n_act_obs = res["num_residuals"] // 2
    alg_bytes = ba_algorithmic_bytes(n_act_obs, int(win["pt_mutable"].sum()) if win else sc.n_points,
                                     int(win["cam_mutable"].sum()) if win else sc.n_cams, n_red)
    chol_flops = n_red ** 3 / 3.0 + 2.0 * n_red ** 2
    kernels = []
    for name, st in sorted(ba_stats.items(), key=lambda kv: -kv[1]["total_ms"]):
        kernels.append(dict(kernel=name, launches=st["launches"], ms_per_step=st["total_ms"] / args.steps,
                            avg_launch_us=1e3 * st["total_ms"] / max(1, st["launches"])))
    # per-kernel rooflines from the live HIP-event timings (profiled pass); algorithmic work per launch:
    #   chol_panel_mfma : the panel launches carry the whole factorisation, n^3/3 flops per solve (FP64 MFMA)
    #   the streaming kernels: bytes each must read + write once
    rooflines = {}
    n_solves = res_p["num_iterations"]

    def add(kname, bound, work_per_launch, note):
        st = ba_stats.get(kname)
        if not st or not st["launches"]:
            return
        t = st["total_ms"] * 1e-3 / st["launches"]
        if bound == "mfma":
            ach, peak, unit = work_per_launch / t / 1e12, FP64_PEAK_TFLOPS, "TFLOP/s"
        else:
            ach, peak, unit = work_per_launch / t / 1e9, HBM_PEAK_GBS, "GB/s"
        rooflines[kname] = dict(bound=bound, achieved=ach, peak=peak, unit=unit, frac=ach / peak, traffic=None,
                                avg_launch_us=t * 1e6, launches=st["launches"], note=note)

    st = ba_stats.get("chol_panel_mfma")
    lay = ba.layout()
    if st:
        dense_flops = n_red ** 3 / 3.0
        # `achieved` follows the contract: ALGORITHMIC flops of the path (the dense factorisation, n^3/3) per launch
        # / launch time.  With camera domains the kernel executes fewer flops for the same result; that figure is given beside it.
        exe_flops = dense_flops
        # (the timing class counts 64-column panel STEPS on the critical path, whether they run as one launch each or inside the
        #  persistent launch of their tree level)
        note = ("n^3/3 = %.2f GFLOP per factorisation (SURVEY 8d) over %d 64-column panel steps on the critical path (trailing update + next "
                "potrf + trsm fused; one persistent launch per tree level)" % (dense_flops / 1e9, st["launches"] // max(1, n_solves)))
        if lay["n_domains"] > 1:
            sep = lay["separator_cols"] + 1
            exe_flops = sep ** 3 / 3.0 + sum(nk ** 3 / 3.0 + nk * nk * sep + nk * sep * sep for nk in lay["domain_cols"])
            note += ("; elimination tree: %d leaf domains of %s columns side by side, then %s separator node(s) per level, the root of %d columns "
                     "last (separator part %d columns in all): %.2f GFLOP actually executed"
                     % (lay["n_domains"], lay["domain_cols"], lay.get("level_nodes", [])[1:], lay.get("root_cols", 0), lay["separator_cols"], exe_flops / 1e9))
        add("chol_panel_mfma", "mfma", dense_flops * n_solves / max(1, st["launches"]), note)
        # the deferred corner updates of the elimination levels (k_corner_syrk + k_merge_corners, their own timing class) are part
        # of the same factorisation: `achieved` charges their time to it; avg_launch_us stays the panel kernel's own (the figure
        # the rocprofv3 kernel trace reports for k_panel_v2)
        syrk = ba_stats.get("chol_corner_syrk")
        fac_s = (st["total_ms"] + (syrk["total_ms"] if syrk else 0.0)) * 1e-3
        rl = rooflines["chol_panel_mfma"]
        rl["achieved"] = dense_flops * n_solves / fac_s / 1e12
        rl["frac"] = rl["achieved"] / rl["peak"]
        rl["factorisation_ms"] = 1e3 * fac_s / max(1, n_solves)
        rl["executed_tflops"] = exe_flops * n_solves / fac_s / 1e12
        rooflines["chol_panel_mfma"]["layout"] = lay
    if not win:
        k = np.bincount(sc.obs_pt, minlength=sc.n_points).astype(np.int64)
        n_pairs_cc = int((k * (k + 1) // 2).sum())
        # (the rows are linearised inside k_point and again inside k_backsub: 52 bytes of row data per observation in,
        # instead of a 26-double stored Jacobian row written once and read twice)
        # With the fold tables (round 3) the camera x camera and intrinsics x camera products are formed inside k_point: its
        # algorithmic bytes gain the slot partials it writes (288 B per camera x camera slot, 144 B per intrinsics x camera
        # slot), and the gather kernels keep only the entries that did not fold (plus the intrinsics x intrinsics list).
        fold = lay.get("fold", {})
        cc_live = fold.get("cc_entries", n_pairs_cc) - fold.get("cc_entries_folded", 0)
        mc_live = fold.get("mc_entries", sc.n_obs) - fold.get("mc_entries_folded", 0)
        fold_bytes = fold.get("slots", 0) * 288 + fold.get("mc_slots", 0) * 144
        impl_bytes = sc.n_obs * (52 + 144 + 48) + sc.n_points * (24 + 96) + fold_bytes
        add("ba_point", "hbm", impl_bytes,
            "row data + point in; T (144 B), T.u (48 B) per observation and L, g, diagonal per point out"
            + ("; %d + %d slot partials of the Schur products formed in the kernel (%.1f MB)" % (fold.get("slots", 0), fold.get("mc_slots", 0), fold_bytes / 1e6)
               if fold_bytes else ""))
        if "ba_point" in rooflines:
            # SURVEY.md 8d accounting for the Jacobian / Schur-build pass (what the contract's `frac` is): the pass's algorithmic
            # bytes No*24 + Np*56 + Nc*96 against HBM, its Schur-build flops against the FP64 roof, `frac` = the larger of the two.
            # The bytes the IMPLEMENTATION moves by design (intermediates it writes for later kernels included) stay beside it as
            # frac_impl_bytes, and `traffic_ratio` (measured HBM bytes / 8d bytes) is added where the PMC counters are attached.
            rl = rooflines["ba_point"]
            t_pt = rl["avg_launch_us"] * 1e-6
            b8d = sc.n_obs * 24 + sc.n_points * 56 + sc.n_cams * 96
            folded = (fold.get("cc_entries_folded", 0) / max(1, fold.get("cc_entries", 1))) if fold else 0.0
            f8d = ba_schur_build_flops(k) * (folded if fold else 0.0)   # the share of the Schur build that this kernel executes
            f8d_self = float((k * (2 * 2 * 81 / 2 + 2 * 2 * 9 * 3 + 2 * 2 * 9 / 2)).sum())   # the per-observation part is always here
            f8d = max(f8d, f8d_self)
            frac_b, frac_f = b8d / t_pt / 1e9 / HBM_PEAK_GBS, f8d / t_pt / 1e12 / FP64_PEAK_TFLOPS
            rl["frac_impl_bytes"] = rl["frac"]
            rl["achieved_impl_GBs"] = rl["achieved"]
            rl["bytes_8d"] = b8d
            rl["flops_8d"] = f8d
            rl["frac_bytes_8d"] = frac_b
            rl["frac_flops_8d"] = frac_f
            if frac_f >= frac_b:
                rl.update(bound="mfma", achieved=f8d / t_pt / 1e12, peak=FP64_PEAK_TFLOPS, unit="TFLOP/s", frac=frac_f)
            else:
                rl.update(bound="hbm", achieved=b8d / t_pt / 1e9, peak=HBM_PEAK_GBS, unit="GB/s", frac=frac_b)
            rl["note"] = ("SURVEY 8d: max(%.1f MB of algorithmic bytes, %.2f GFLOP of Schur build - %.1f %% of the camera x camera products fold "
                          "into this kernel) / launch time against the respective roof (FP64 vector = matrix rate, %.1f TFLOP/s); "
                          "frac_impl_bytes = the bytes the kernel moves by design (%.1f MB: %s) / time / HBM peak"
                          % (b8d / 1e6, f8d / 1e9, 100 * folded, FP64_PEAK_TFLOPS, impl_bytes / 1e6, rl["note"]))
        add("ba_schur_pairs", "hbm", (cc_live + mc_live) * 288 + sc.n_points * 144,
            "two 144-byte T records gathered per pair entry that is not folded into k_point (%d of %d camera x camera, %d of %d intrinsics x camera)"
            % (cc_live, fold.get("cc_entries", n_pairs_cc), mc_live, fold.get("mc_entries", sc.n_obs)))
        add("ba_assemble", "hbm", fold_bytes + (cc_live + mc_live > 0) * 0 + lay["reduced_order"] ** 2 * 4,
            "slot partials in, lower triangle of the reduced system out")
        add("ba_backsub", "hbm", sc.n_obs * 52 + sc.n_points * 12 * 8, "row data, point and its 3x3 factor in, candidate point out")
        add("ba_ftf", "hbm", sc.n_obs * (28 + 24 + 48 + 4), "camera-major statics (28 B), point (24 B), T.u (48 B) per row in; the rows are linearised again.  "
            "(round 4: the class times k_sums + k_camftf and k_modelsum as two scopes per iteration - k_sums also carries the residue of the pair lists and the "
            "zero fill of the reduced system, which used to be the class ba_schur_pairs on a second stream)")
    dom = kernels[0]
    step_bw = alg_bytes / (ba_s / args.steps) / 1e9
    whole = dict(bound="hbm", achieved=step_bw, peak=HBM_PEAK_GBS, unit="GB/s", frac=step_bw / HBM_PEAK_GBS, traffic=None,
                 kernel="lm_iteration (all kernels)",
                 note="algorithmic bytes of one LM iteration (SURVEY 8d: %.1f MB) / measured time per iteration; "
                      "FP64 side: %.3f GFLOP Cholesky per iteration" % (alg_bytes / 1e6, chol_flops / 1e9))
    roofline = dict(rooflines[dom["kernel"]], kernel=dom["kernel"]) if dom["kernel"] in rooflines else whole
    # HBM traffic of the dominant kernel from the rocprofv3 PMC passes (profiles/), per launch - only if the counters were
    # collected with the kernels that are running now
    pmc_path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    if os.path.exists(pmc_path) and args.config == 3 and world == 1:
        try:
            pmc = json.load(open(pmc_path))
            if pmc.get("_kernel_source_hash") == kernel_source_hash() and roofline.get("kernel") in pmc:
                roofline["traffic"] = pmc[roofline["kernel"]]["bytes_per_launch"]
                roofline["traffic_source"] = pmc[roofline["kernel"]].get("source")
                if roofline.get("bytes_8d"):
                    roofline["traffic_ratio"] = roofline["traffic"] / roofline["bytes_8d"]
            elif roofline.get("kernel") in pmc:
                roofline["traffic_note"] = "profiles/pmc_traffic.json was collected with other kernel sources (%s); not attached" % pmc.get("_kernel_source_hash")
        except Exception:
            pass

    # matrix-pipe utilisation from the SQ counter passes (scripts/mfma_util.sh -> profiles/rNN_mfma_util.json): attached to the
    # rooflines of the MFMA kernels, with a note when the counters were collected with other kernel sources
    util, util_name = {}, "none"
    try:
        import glob
        util_path = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_mfma_util.json")))[-1]   # the newest round's
        util_name = "profiles/" + os.path.basename(util_path)
        util = json.load(open(util_path))
    except Exception:
        pass

    def attach_util(rl, key):
        u = util.get(key)
        if not rl or not u:
            return
        for k in ("mfma_busy", "valu_busy", "valu_per_mfma"):
            if k in u:
                rl[k] = u[k]
        rl["mfma_busy_source"] = util_name + " (SQ_VALU_MFMA_BUSY_CYCLES / (1024 SIMDs x GRBM_GUI_ACTIVE / 8))" + (
            "" if util.get("_kernel_source_hash") == kernel_source_hash() else "; collected with other kernel sources (%s)" % util.get("_kernel_source_hash"))

    attach_util(rooflines.get("chol_panel_mfma"), "ba")
    if roofline.get("kernel") == "chol_panel_mfma":
        attach_util(roofline, "ba")
    out.update(roofline=roofline, roofline_whole_step=whole, kernel_rooflines=rooflines, ba_kernels=kernels,
               bound_note=("`bound` names the roof the dominant kernel is priced against (the contract's two values; 'mfma' = the FP64 rate, "
                           "which vector and matrix pipe share), not a throughput limit that has been reached: an LM iteration moves ~1.1 GB "
                           "(PMC) = ~14 % of HBM bandwidth and executes ~15 GFLOP = ~20 % of the FP64 roof - it is latency- and issue-bound "
                           "(dependent pivot chains, LDS gathers, two or three waves per SIMD)"),
               ba_one_shot=one_shot)
    ba.close()

    # ------------------------------------------------------------------ matching legs: every ordered pair of the scene
    descs = None
    if not args.no_matching and not win:
        n_img = sc.n_cams if args.match_images <= 0 else min(args.match_images, sc.n_cams)
        t0 = time.time()
        scene.add_features(sc, args.feats, images=range(n_img))
        feat_s = time.time() - t0
        log("features of %d images generated" % n_img)
        descs = [sc.desc[i] for i in range(n_img)]
        pairs = scene.all_pairs(n_img)
        counts = np.array([len(d) for d in descs], dtype=np.int64)
        my_pairs = shard.shard_pairs(pairs, rank, world, counts)
        queries = int(counts[pairs[:, 1]].sum())
        flops = float(2 * 128 * (counts[pairs[:, 0]] * counts[pairs[:, 1]]).sum())
        my_flops = float(2 * 128 * (counts[my_pairs[:, 0]] * counts[my_pairs[:, 1]]).sum())

        def run_matching(dset, label, steps):
            ds = ctx.descset(dset)
            log("matching [%s]: descriptors uploaded" % label[:24])
            mres = ds.match_pairs(my_pairs, 0.6, 0.85, keep_knn=False)   # first pass: allocation + warm-up
            barrier()
            log("matching: first pass done")
            t0 = time.perf_counter()
            for _ in range(steps):
                mres.rerun()
            barrier()
            m_s = max_over_ranks(time.perf_counter() - t0)
            log("matching: %d timed pass(es), %.1f Mmatches/s" % (steps, 1e-6 * queries * steps / m_s))
            ctx.profile(True)
            ctx.profile_reset()
            mres.rerun()
            ctx.synchronize()
            mstats = ctx.profile_get()
            ctx.profile(False)
            na, ng = mres.counts()
            stats = mres.stats()
            mres.close()
            ds.close()
            peaks = {"knn2_i8_mfma": (I8_PEAK_TOPS, "i8"), "knn2_bf16_mfma": (BF16_PEAK_TFLOPS, "bf16"), "knn2_f16_mfma": (BF16_PEAK_TFLOPS, "f16"),
                     "knn2_split_bf16_mfma": (BF16_PEAK_TFLOPS, "bf16x3"), "knn2_exact_f64": (FP64_PEAK_TFLOPS, "f64")}
            kname = next((k for k in peaks if k in mstats), None)
            kst = mstats.get(kname)
            kern_tf = my_flops / (kst["total_ms"] * 1e-3) / 1e12 if kst else None
            peak = peaks[kname][0] if kname else None
            return dict(metric="Mmatches/sec", value=1e-6 * queries * steps / m_s, unit="Mmatches/s (query descriptors with a 2-NN + ratio decision)",
                        descriptors=label, images=n_img, pairs=int(len(pairs)), feats_per_image=args.feats, steps=steps, ms_per_step=1e3 * m_s / steps,
                        gdist_per_s=flops / 256 * steps / m_s / 1e9, dtype=peaks[kname][1] if kname else None,
                        matches_all=int(na.sum()), matches_good=int(ng.sum()), slow_path_queries=stats["slow_path"],
                        kernels={k: v for k, v in mstats.items()},
                        roofline=dict(bound="mfma", achieved=kern_tf, peak=peak, unit="TFLOP/s", frac=(kern_tf / peak) if kern_tf else None, traffic=None,
                                      kernel=kname, avg_launch_ms=kst["total_ms"] if kst else None,
                                      note="algorithmic 2*128*M1*M2 operations per ordered pair / time of the MFMA kernel of the path"))

        m_int = run_matching(descs, "integer SIFT-like in [0,255] stored as float32 (exact int8 MFMA path)", max(1, args.match_steps))
        m_int["feature_gen_s"] = feat_s
        attach_util(m_int["roofline"], "knn_i8")
        out["mmatches_per_sec"] = m_int["value"]
        out["matching"] = m_int
        # the reference's extractors hand over non-integral floats (feature_extractor_vl_sift.cpp:202: 512.0F * x, never cast):
        # the same descriptors unit-normalised and scaled by 512
        fdescs = [(512.0 * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32) for d in descs]
        out["matching_float"] = run_matching(fdescs, "non-integral floats, 512 * unit-norm (VLFeat convention; certified shortlist + exact re-rank)", 1)
        attach_util(out["matching_float"]["roofline"], "knn_f16")
        del fdescs

    # ------------------------------------------------------------------ the reference's CALL PATTERN for bundle adjustment (round 5)
    # IncrementalSfM::Run solves a fresh problem per added image (sfm_incremental.cc:146-190): neither the resident rate above nor
    # one one-shot call is that.  scripts/ba_incremental.py replays it: config 2's cameras one at a time (partial BA per camera, a
    # full one every 5th), and - on the config 5 window run - the windows of its twenty newest cameras one after the other.
    if not args.no_extras and rank == 0 and world == 1:
        try:
            sys.path.insert(0, os.path.join(ROOT, "scripts"))
            import ba_incremental
            if win:
                out["ba_incremental_windows"] = ba_incremental.windows(ctx, 20, 20, sc)
            else:
                out["ba_incremental"] = ba_incremental.sequence(ctx, 2)
            log("incremental call pattern measured")
        except Exception as e:   # a side leg must not take the headline line down
            out["ba_incremental_error"] = repr(e)

    # ------------------------------------------------------------------ triangulation / reprojection leg (A4, A5, A11)
    if not args.no_extras and not win:
        R, t, c, fk = scene.cameras_for_tracks(sc)
        # tracks are independent: every rank takes a contiguous range balanced by observation count, no collective
        tr = shard.shard_tracks(A.TrackArrays(sc.track_offsets(), sc.obs_cam, sc.obs_xy, R, t, c, fk), rank, world)
        tlo, thi = tr.track_range
        th_ang = np.deg2rad(3.0)
        legs = {}
        for name, fn in (("midpoint", lambda: ctx.triangulate_midpoint(tr, 7.0, th_ang)), ("dlt", lambda: ctx.triangulate_dlt(tr, 7.0, th_ang)),
                         ("reproject", lambda: ctx.reproject_mse(tr, sc.point_gt[tlo:thi]))):
            fn()   # untimed first call (the first launch of a kernel loads its code)
            barrier()
            ctx.profile(True)
            ctx.profile_reset()
            t0 = time.perf_counter()
            r = fn()
            wall = max_over_ranks(time.perf_counter() - t0)
            st = ctx.profile_get()
            ctx.profile(False)
            kms = max_over_ranks(sum(v["total_ms"] for v in st.values()))
            # algorithmic bytes: per observation camera index 4 + xy 16, per track offsets 4 + X 24 (+ mse 8 + ok 1 out);
            # cameras (30 doubles each) stay in cache
            nbytes = sc.n_obs * 20 + sc.n_points * (4 + 24 + 8 + 1)
            legs[name] = dict(tracks=sc.n_points, observations=sc.n_obs, wall_ms=1e3 * wall, kernel_ms=kms,
                              tracks_per_s_kernel=(sc.n_points / (kms * 1e-3)) if kms else None, tracks_per_s_end_to_end=sc.n_points / wall,
                              roofline=dict(bound="hbm", achieved=(nbytes / (kms * 1e-3) / 1e9) if kms else None, peak=HBM_PEAK_GBS, unit="GB/s",
                                            frac=(nbytes / (kms * 1e-3) / 1e9 / HBM_PEAK_GBS) if kms else None, traffic=None,
                                            note="CSR tracks streamed once: %.1f MB" % (nbytes / 1e6)),
                              accepted=int(r[2].sum()) if isinstance(r, tuple) else None)
        log("triangulation leg done")
        out["triangulation"] = dict(note="host arrays in, host arrays out (PCIe inclusive wall time; kernel time from HIP events); th_error 7 px, "
                                         "th_angle 3 deg (sfm_incremental.cc:780-784); tracks split over %d rank(s) by shard.shard_tracks, times are the "
                                         "maximum over ranks, `accepted` is rank 0's range" % world, **legs)

    # ------------------------------------------------------------------ resident chain: codes -> verification -> tracks -> points -> BA problem
    if not args.no_extras and not args.no_matching and not win and rank == 0 and descs is not None and args.chain_images > 1:
        from metricsfm_amd import matchfiles
        n_ci = min(args.chain_images, len(descs))
        kps = [np.ascontiguousarray(sc.kp_xy[i], np.float32) for i in range(n_ci)]
        cds = ctx.descset(descs[:n_ci], keypoints=kps)
        cpairs = scene.all_pairs(n_ci)
        cres = cds.match_pairs(cpairs, 0.6, 0.85)
        Rc, tc, cc, fkc = scene.cameras_for_tracks(sc)
        Rc, tc, cc, fkc = Rc[:n_ci], tc[:n_ci], cc[:n_ci], fkc[:n_ci]
        ctx.synchronize()

        def run_chain():
            t0 = time.perf_counter()
            ch = capi.Chain(cres)
            n_m, okc, _ = ch.verify(3.0)
            t1 = time.perf_counter()
            nt, no = ch.build_tracks()
            t2 = time.perf_counter()
            nacc = ch.triangulate(Rc, tc, cc, fkc, 7.0, np.deg2rad(3.0))
            t3 = time.perf_counter()
            cba = ch.ba_create(sc.cam_pose[:n_ci], sc.cam_model, sc.cam_model_of_cam[:n_ci], min_views=3, weight_ge3=1.0)
            ctx.synchronize()
            t4 = time.perf_counter()
            out_ = dict(verify_ms=1e3 * (t1 - t0), tracks_ms=1e3 * (t2 - t1), triangulate_ms=1e3 * (t3 - t2), ba_create_ms=1e3 * (t4 - t3), total_ms=1e3 * (t4 - t0),
                        pairs_ok=int(okc.sum()), matches=int(n_m.sum()), tracks=nt, observations=no, accepted=nacc, ba_points=len(cba.track_of_point), ba_observations=cba.n_obs)
            cba.close(); ch.close()
            return out_

        def run_host():
            t0 = time.perf_counter()
            good_l, all_l = [], []
            for p in range(len(cpairs)):
                code, _, _ = cres.fetch(p)
                g, a = matchfiles.codes_to_matches(code)
                good_l.append(g); all_l.append(a)
            off_g = np.concatenate([[0], np.cumsum([len(g) for g in good_l])]).astype(np.int32)
            off_a = np.concatenate([[0], np.cumsum([len(a) for a in all_l])]).astype(np.int32)
            g1 = np.concatenate([kps[i][g[:, 0]] for (i, j), g in zip(cpairs, good_l)]); g2 = np.concatenate([kps[j][g[:, 1]] for (i, j), g in zip(cpairs, good_l)])
            a1 = np.concatenate([kps[i][a[:, 0]] for (i, j), a in zip(cpairs, all_l)]); a2 = np.concatenate([kps[j][a[:, 1]] for (i, j), a in zip(cpairs, all_l)])
            Fh, _, _, okh = ctx.fundamental_ransac(off_g, g1, g2)
            in_a = ctx.epipolar_filter_batch(off_a, a1, a2, Fh, okh, 3.0)
            fin = [all_l[p][in_a[off_a[p]:off_a[p + 1]] != 0] if okh[p] else np.zeros((0, 2), np.int32) for p in range(len(cpairs))]
            t1 = time.perf_counter()
            moff = np.concatenate([[0], np.cumsum([len(m) for m in fin])]).astype(np.int32)
            flat = (np.array([len(k) for k in kps], np.int32), A.as_c(cpairs, np.int32), moff, A.as_c(np.concatenate(fin).reshape(-1, 2), np.int32))
            off, img, feat = ctx.build_tracks(None, None, None, flat=flat)
            t2 = time.perf_counter()
            xy = np.empty((len(img), 2))
            for i in range(n_ci):
                sel = img == i
                xy[sel] = kps[i][feat[sel]]
            Xh, _, tokh = ctx.triangulate_midpoint(A.TrackArrays(off, img, xy, Rc, tc, cc, fkc), 7.0, np.deg2rad(3.0))
            t3 = time.perf_counter()
            keep = (tokh != 0) & (np.diff(off) >= 3)
            obs_sel = np.repeat(keep, np.diff(off))
            arrays = A.BaArrays(sc.cam_pose[:n_ci].copy(), sc.cam_model.copy(), sc.cam_model_of_cam[:n_ci], Xh[keep].copy(), img[obs_sel],
                                np.repeat(np.cumsum(keep) - 1, np.diff(off))[obs_sel].astype(np.int32), xy[obs_sel], np.ones(int(keep.sum())))
            hba = ctx.ba(arrays)
            ctx.synchronize()
            t4 = time.perf_counter()
            hba.close()
            return dict(verify_ms=1e3 * (t1 - t0), tracks_ms=1e3 * (t2 - t1), triangulate_ms=1e3 * (t3 - t2), ba_create_ms=1e3 * (t4 - t3), total_ms=1e3 * (t4 - t0))

        run_chain()   # untimed first pass (kernel code, pool blocks)
        ch_t = run_chain()
        host_t = run_host()
        out["resident_chain"] = dict(images=n_ci, pairs=int(len(cpairs)), feats_per_image=args.feats, device=ch_t, host_arrays=host_t,
                                     speedup=host_t["total_ms"] / ch_t["total_ms"],
                                     note="match codes -> GeoVerificationFundamental + filter -> track building -> midpoint triangulation -> msfm_ba_create, "
                                          "once with every intermediate result resident (msfm_chain_*) and once through the host-array entry points on the "
                                          "fetched results of each stage (numpy gathers included: they stand for the reference's per-pair loops); results identical "
                                          "(tests/test_gpu_chain.py)")
        cres.close(); cds.close()
        log("resident chain leg done")

    # ------------------------------------------------------------------ geometric-verification leg
    if not args.no_extras and rank == 0:
        log("verification / pose legs")
        rng = np.random.default_rng(0x4D53464D)
        n_vp, n_vm = args.verify_pairs, 256

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

        tv = [two_view(n_vm) for _ in range(64)]   # 64 distinct geometries, tiled to n_vp pairs
        v1 = np.concatenate([tv[p % 64][0] for p in range(n_vp)])
        v2 = np.concatenate([tv[p % 64][1] for p in range(n_vp)])
        voff = (np.arange(n_vp + 1) * n_vm).astype(np.int32)
        ctx.fundamental_ransac(voff, v1, v2)   # untimed first call at full size (kernel code, device blocks of the call's sizes)
        ctx.profile(True)
        ctx.profile_reset()
        t0 = time.perf_counter()
        _, _, vnin, vok = ctx.fundamental_ransac(voff, v1, v2)
        v_s = time.perf_counter() - t0
        vst = ctx.profile_get()
        ctx.profile(False)
        kms = sum(v["total_ms"] for k, v in vst.items() if k.startswith("geo_fransac"))
        out["geo_verification"] = dict(metric="pairs verified/sec", value=n_vp / v_s, unit="pairs/s", pairs=n_vp, matches_per_pair=n_vm,
                                       outlier_fraction=0.3, samples_per_pair="up to 2000 (128 scored first, the rest only for pairs whose adaptive budget is still open); scoring with lane = match, model uniform over the wave (round 4)", accepted=int(vok.sum()), mean_inliers=float(vnin.mean()),
                                       kernel_ms=kms, kernel_pairs_per_sec=(n_vp / (kms * 1e-3)) if kms else None, dtype="f64",
                                       note="host arrays in, host arrays out (PCIe inclusive); FM_RANSAC restatement, 7-point solver")
        if world == 1 and not args.no_cpu_baseline:
            from oracle import oracle as O
            t0 = time.perf_counter()
            O.fundamental_ransac(voff[:5], v1[:4 * n_vm], v2[:4 * n_vm])
            out["geo_verification"]["cpu_baseline"] = dict(value=4 / (time.perf_counter() - t0), unit="pairs/s", cores=1, kind="port",
                                                           sample="4 pairs by the sequential CPU oracle (adaptive stop active)")

    # ------------------------------------------------------------------ pose-initialiser leg
    if not args.no_extras and rank == 0:
        rng = np.random.default_rng(0x4D53464D + 3)
        n_img, n_corr = args.pose_images, 256

        def rod(a):
            th = np.linalg.norm(a)
            K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]]) / th
            return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K

        def pnp(n):
            X = np.column_stack([rng.uniform(-40, 40, n), rng.uniform(-30, 30, n), rng.uniform(-5, 5, n)])
            R = rod(np.array([np.pi, 0.0, 0.0]) + rng.normal(0, 0.05, 3))
            t = -R @ np.array([rng.uniform(-5, 5), rng.uniform(-5, 5), 100.0])
            Xc = X @ R.T + t
            return X, 4800 * Xc[:, :2] / Xc[:, 2:3] + rng.normal(0, 0.5, (n, 2))

        def rel(n):
            X = np.column_stack([rng.uniform(-40, 40, n), rng.uniform(-30, 30, n), rng.uniform(80, 120, n)])
            Xc = X @ rod(rng.normal(0, 0.05, 3)).T + np.array([10.0, 1.0, 0.5])
            return (4800 * X[:, :2] / X[:, 2:3] + rng.normal(0, 0.5, (n, 2)), 4800 * Xc[:, :2] / Xc[:, 2:3] + rng.normal(0, 0.5, (n, 2)))

        pn = [pnp(n_corr) for _ in range(64)]
        pX = np.concatenate([pn[p % 64][0] for p in range(n_img)])
        px = np.concatenate([pn[p % 64][1] for p in range(n_img)])
        rl = [rel(n_corr) for _ in range(64)]
        ra = np.concatenate([rl[p % 64][0] for p in range(n_img)])
        rb = np.concatenate([rl[p % 64][1] for p in range(n_img)])
        poff = (np.arange(n_img + 1) * n_corr).astype(np.int32)
        ctx.epnp_ransac(poff, pX, px, 4800.0)      # untimed first calls at full size
        ctx.relpose_5pt(poff, ra, rb, 4800.0, 4800.0)
        ctx.profile(True)
        ctx.profile_reset()
        t0 = time.perf_counter()
        _, _, _, pavg, _ = ctx.epnp_ransac(poff, pX, px, 4800.0)
        p_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        _, _, _, rok, rnc = ctx.relpose_5pt(poff, ra, rb, 4800.0, 4800.0)
        r_s = time.perf_counter() - t0
        pst = ctx.profile_get()
        ctx.profile(False)
        pk = sum(pst[k]["total_ms"] for k in ("pose_epnp_hyp", "pose_epnp_select") if k in pst)
        rk = sum(pst[k]["total_ms"] for k in ("pose_e5_hyp", "pose_e5_score", "pose_e5_select") if k in pst)
        out["pose_initialisers"] = dict(
            absolute=dict(metric="images localised/sec", value=n_img / p_s, unit="images/s", images=n_img, correspondences_per_image=n_corr,
                          samples_per_image=200, localised=int((pavg < 5.0).sum()), kernel_ms=pk,
                          kernel_images_per_sec=(n_img / (pk * 1e-3)) if pk else None, kernels={k: pst[k] for k in pst if k.startswith("pose_epnp")}),
            relative=dict(metric="pairs oriented/sec", value=n_img / r_s, unit="pairs/s", pairs=n_img, matches_per_pair=n_corr, samples_per_pair=100,
                          oriented=int(rok.sum()), mean_candidates=float(rnc.mean()), kernel_ms=rk,
                          kernel_pairs_per_sec=(n_img / (rk * 1e-3)) if rk else None, kernels={k: pst[k] for k in pst if k.startswith("pose_e5")}),
            dtype="f64", note="host arrays in, host arrays out (PCIe inclusive); EPnP on 4-point samples / Nister five-point, one GPU thread per sample")
        if world == 1 and not args.no_cpu_baseline:
            from oracle import oracle as O
            t0 = time.perf_counter()
            O.epnp_ransac(poff[:17], pX[:16 * n_corr], px[:16 * n_corr], 4800.0)
            out["pose_initialisers"]["absolute"]["cpu_baseline"] = dict(value=16 / (time.perf_counter() - t0), unit="images/s", cores=1, kind="port",
                                                                        sample="16 images by the sequential CPU oracle")
            t0 = time.perf_counter()
            O.relpose_5pt(poff[:17], ra[:16 * n_corr], rb[:16 * n_corr], 4800.0, 4800.0)
            out["pose_initialisers"]["relative"]["cpu_baseline"] = dict(value=16 / (time.perf_counter() - t0), unit="pairs/s", cores=1, kind="port",
                                                                        sample="16 pairs by the sequential CPU oracle")

    # ------------------------------------------------------------------ CPU baseline (rank 0, N = 1 only): 1 thread and all cores
    if world == 1 and not args.no_cpu_baseline:
        from oracle import oracle as O
        cores = O.host_cores()
        cpu_model = ""
        try:
            cpu_model = next(l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name"))
        except Exception:
            pass

        def cpu_ba(nt, iters):
            ref = A.BaArrays(full.cam_pose, full.cam_model, full.cam_model_of_cam, full.point, full.obs_cam, full.obs_pt, full.obs_xy, full.pt_weight,
                             cam_mutable=full.cam_mutable, model_mutable=full.model_mutable, pt_mutable=full.pt_mutable, gps_xyz=full.gps_xyz,
                             gps_weight=full.struct.gps_weight)
            t0 = time.perf_counter()
            r = O.ba_solve(ref, O.default_options(max_num_iterations=iters, num_threads=nt, function_tolerance=-1.0,
                                                  gradient_tolerance=-1.0, parameter_tolerance=-1.0))
            wall = time.perf_counter() - t0
            return dict(value=r["num_iterations"] / (r["solve_ms"] * 1e-3), unit="iterations/s", cores=nt, iterations=r["num_iterations"], wall_s=wall)

        cpu_iters = 3 if not win else 10
        log("CPU baseline: bundle adjustment on 1 thread")
        one = cpu_ba(1, cpu_iters)
        log("CPU baseline: bundle adjustment on %d threads" % cores)
        allc = cpu_ba(cores, cpu_iters) if cores > 1 else one
        log("CPU baseline: matching")
        cpu = dict(value=allc["value"], unit="iterations/s", cores=allc["cores"], kind="port",
                   sample="%d LM iterations of the same problem by the CPU oracle (restated reference path: Ceres 1.13 trust-region LM, dense "
                          "Schur) on %d threads, %.1f s wall; results bit-identical to the 1-thread run" % (allc["iterations"], allc["cores"], allc["wall_s"]),
                   one_thread=dict(one, note="num_threads = 1 as the SfM pipeline sets it (basic_structs.h:234 -> optimizer.cc:46)"),
                   all_cores=dict(allc, note="all cores of this job's share of the host (SLAMGPS sets num_threads = 8, slam_gps.cc:683)"),
                   host=dict(cores_available=cores, cpu_model=cpu_model))
        if descs is not None:
            # CPU matching: the reference's OpenMP loop over idx2 (fine_matching_graph.cc:87-100) with brute-force L2 (FLANN's
            # L2<float> arithmetic) on a seeded sample of the config's ordered pairs, extrapolated by pair count
            rng = np.random.default_rng(0x4D53464D + 7)
            all_pairs = scene.all_pairs(len(descs))

            def cpu_match(nt, n_sample):
                sel = rng.choice(len(all_pairs), size=min(n_sample, len(all_pairs)), replace=False)
                O.set_num_threads(nt)
                t0 = time.perf_counter()
                nq = 0
                for p in sel:
                    i, j = all_pairs[p]
                    O.knn2(descs[i], descs[j], fast=True)
                    nq += len(descs[j])
                dt = time.perf_counter() - t0
                O.set_num_threads(1)
                return dict(value=1e-6 * nq / dt, unit="Mmatches/s", cores=nt, pairs_sampled=int(len(sel)), fraction_of_pairs=len(sel) / len(all_pairs), wall_s=dt)

            m1 = cpu_match(1, 24)
            # "time a 1 % pair sample and extrapolate" - 2495 of config 3's pairs on all cores (about 25 s on 16)
            ma = cpu_match(cores, max(48, int(round(0.01 * len(all_pairs))))) if cores > 1 else m1
            cpu["matching"] = dict(value=ma["value"], unit="Mmatches/s", cores=ma["cores"],
                                   sample="seeded sample of %d of the %d ordered pairs (%.3f %%), brute-force float32 2-NN, OpenMP over queries; "
                                          "whole-config time extrapolates by pair count" % (ma["pairs_sampled"], len(all_pairs), 100 * ma["fraction_of_pairs"]),
                                   algorithm="exact brute force (the reference's FLANN kd-tree - 8 trees, 64 checks, fine_matching_graph.cc:74-77 - is "
                                             "approximate and does ~50 x less work per query; this is the exact search it approximates, not its speed)",
                                   one_thread=m1, all_cores=ma)
        out["cpu_baseline"] = cpu
        out["speedup_vs_cpu_port"] = dict(ba_vs_all_cores=it_s / allc["value"], ba_vs_one_thread=it_s / one["value"])
        if descs is not None:
            out["speedup_vs_cpu_port"]["matching_vs_all_cores"] = out["matching"]["value"] / cpu["matching"]["value"]
            out["speedup_vs_cpu_port"]["matching_note"] = "against exact brute force on the CPU, not against the reference's approximate kd-tree"

    finish(out)


if __name__ == "__main__":
    main()
