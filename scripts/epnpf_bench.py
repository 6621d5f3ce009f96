"""Timing of the EPnP focal sweep (msfm_epnpf_sweep_batch) against the only route that existed before it:
msfm_epnp_ransac_batch on the batch expanded n_steps-fold (every image repeated once per candidate focal length).

  python scripts/epnpf_bench.py [--reps 5] [--baseline-lib LIBMSFM_OF_THE_PARENT_COMMIT] [--cpu] [--out FILE]

Two workloads at the reference's options (350 candidates x 200 samples), 20 % outliers: one image of 2 000 correspondences
(the reference's own per-image call) and 16 images of 500.  Per workload and route: wall time of the call (median, min and
max of --reps after one warm-up call; the clock stops after the call's own device synchronise) and, from one further
profiled call, the kernel split of msfm_ctx_profile_get.  The expanded arrays are built outside the timed window.
Each route runs in a child process (`--route`) in the order expanded, sweep, expanded, sweep.  The expanded route binds
only the calls it needs (a library of the parent commit has no sweep symbols for metricsfm_amd.capi to bind) from
--baseline-lib, or from this tree's library without it; the sweep child also checks that both routes of its own library
agree bit for bit.
--cpu adds the CPU reference (tests/epnpf_ref.py, one thread) on the 2 000-point image.  One JSON line per result."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.twoview import make_pnp_batch  # noqa: E402

WORKLOADS = (("1x2000", 41, [2000]), ("16x500", 42, [500] * 16))
LO, HI, STEP, ITERS, F_INIT = 0.5, 4.0, 0.01, 200, 5760.0   # f_init = 1.2 * 4800: the true focal length is candidate 33


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


def expand(off, X, x, S):
    sizes = np.diff(off)
    eoff = np.concatenate([[0], np.cumsum(np.repeat(sizes, S))]).astype(np.int32)
    eX = np.concatenate([np.tile(X[off[p]:off[p + 1]], (S, 1)) for p in range(len(sizes))])
    ex = np.concatenate([np.tile(x[off[p]:off[p + 1]], (S, 1)) for p in range(len(sizes))])
    ef = np.array([(LO + i * STEP) * F_INIT for p in range(len(sizes)) for i in range(S)])
    return eoff, eX, ex, ef


class PlainContext:
    """The four calls the expanded route needs, bound by hand from any libmsfm.so."""

    def __init__(self, path):
        import ctypes as C
        from metricsfm_amd import _abi as A
        self.C, self.A, self.path = C, A, path
        L = self.L = C.CDLL(path)
        vp, i = C.c_void_p, C.c_int
        L.msfm_ctx_create.argtypes = [i, C.POINTER(vp)]
        L.msfm_ctx_destroy.argtypes = [vp]
        L.msfm_ctx_destroy.restype = None
        L.msfm_ctx_profile_enable.argtypes = [vp, i]
        L.msfm_ctx_profile_reset.argtypes = [vp]
        L.msfm_ctx_profile_get.argtypes = [vp, C.POINTER(A.KernelStat), i, C.POINTER(i)]
        L.msfm_epnp_ransac_batch.argtypes = [vp, i, A.c_int_p, A.c_double_p, A.c_double_p, A.c_double_p, i, C.c_uint64, A.c_double_p,
                                             A.c_double_p, A.c_double_p, A.c_double_p, A.c_int_p]
        self._h = vp()
        if L.msfm_ctx_create(0, C.byref(self._h)) != 0:
            raise RuntimeError("msfm_ctx_create failed: no GPU")

    def epnp_ransac(self, off, X, x, f, max_iter):
        A, n = self.A, len(off) - 1
        R = np.zeros((n, 3, 3)); t = np.zeros((n, 3)); err = np.zeros(len(X)); avg = np.zeros(n); best = np.zeros(n, np.int32)
        rc = self.L.msfm_epnp_ransac_batch(self._h, n, A.ptr(off, A.c_int_p), A.ptr(X, A.c_double_p), A.ptr(x, A.c_double_p),
                                           A.ptr(f, A.c_double_p), max_iter, 0x4D53464D50, A.ptr(R, A.c_double_p), A.ptr(t, A.c_double_p),
                                           A.ptr(err, A.c_double_p), A.ptr(avg, A.c_double_p), A.ptr(best, A.c_int_p))
        if rc != 0:
            raise RuntimeError("msfm_epnp_ransac_batch rc=%d" % rc)
        return R, t, err, avg, best

    def profile(self, on):
        self.L.msfm_ctx_profile_enable(self._h, int(on))

    def profile_reset(self):
        self.L.msfm_ctx_profile_reset(self._h)

    def profile_get(self):
        C, A = self.C, self.A
        arr = (A.KernelStat * A.MSFM_MAX_KERNEL_STATS)()
        n = C.c_int()
        self.L.msfm_ctx_profile_get(self._h, arr, A.MSFM_MAX_KERNEL_STATS, C.byref(n))
        return {arr[k].name.decode(): dict(launches=int(arr[k].launches), total_ms=float(arr[k].total_ms)) for k in range(n.value)}

    def close(self):
        self.L.msfm_ctx_destroy(self._h)


def run_route(route, reps, out, lib_path=None):
    from metricsfm_amd import capi
    lib_path = lib_path or capi.LIB_PATH
    ctx = PlainContext(lib_path) if route == "expanded" else capi.Context(0)
    S = int((HI - LO) / STEP)
    for name, seed, sizes in WORKLOADS:
        off, X, x, _, _ = make_pnp_batch(seed, sizes, outlier_frac=0.2)
        if route == "expanded":
            eoff, eX, ex, ef = (np.ascontiguousarray(v) for v in expand(off, X, x, S))
            call = lambda: ctx.epnp_ransac(eoff, eX, ex, ef, max_iter=ITERS)
        else:
            call = lambda: ctx.epnpf_sweep(off, X, x, F_INIT, LO, HI, STEP, max_iter=ITERS)
        ts, res = timed(call, reps)
        ctx.profile(True)
        ctx.profile_reset()
        call()
        prof = ctx.profile_get()
        ctx.profile(False)
        rec = dict(what="epnpf", route=route, lib=os.path.relpath(lib_path, ROOT),
                   workload=name, images=len(sizes), n_steps=S, max_iter=ITERS, wall_ms=round(float(np.median(ts)) * 1e3, 3),
                   wall_ms_min=round(min(ts) * 1e3, 3), wall_ms_max=round(max(ts) * 1e3, 3), reps=reps,
                   kernels={k: round(v["total_ms"], 3) for k, v in prof.items()} if isinstance(prof, dict) else prof)
        if route == "sweep":
            f, R, t, err, avg, bs, bi = res
            eoff, eX, ex, ef = expand(off, X, x, S)
            R1, t1, e1, a1, b1 = ctx.epnp_ransac(eoff, eX, ex, ef, max_iter=ITERS)
            q = np.arange(len(sizes)) * S + bs
            same = bool((R == R1[q]).all() and (t == t1[q]).all() and (avg == a1[q]).all() and (bi == b1[q]).all() and (f == ef[q]).all()
                        and all((err[off[p]:off[p + 1]] == e1[eoff[q[p]]:eoff[q[p] + 1]]).all() for p in range(len(sizes))))
            rec.update(best_step=bs.tolist(), f=f.tolist(), avg_error=[round(float(v), 4) for v in avg], equals_expanded_route=same)
        emit(rec, out)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--route", choices=("sweep", "expanded"), default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.route:
        return run_route(a.route, a.reps, a.out, a.baseline_lib and os.path.abspath(a.baseline_lib))
    for route in ("expanded", "sweep", "expanded", "sweep"):
        cmd = [sys.executable, os.path.abspath(__file__), "--route", route, "--reps", str(a.reps)] + (["--out", a.out] if a.out else [])
        if route == "expanded" and a.baseline_lib:
            cmd += ["--baseline-lib", a.baseline_lib]
        subprocess.run(cmd, check=True, timeout=600)
    if a.cpu:
        from oracle import oracle as O
        from tests import epnpf_ref
        O.build()
        name, seed, sizes = WORKLOADS[0]
        off, X, x, _, _ = make_pnp_batch(seed, sizes, outlier_frac=0.2)
        t0 = time.perf_counter()
        r = epnpf_ref.epnpf_sweep(O, off, X, x, F_INIT, LO, HI, STEP, max_iter=ITERS)
        emit(dict(what="epnpf", route="cpu_reference_one_thread", workload=name, s_per_image=round(time.perf_counter() - t0, 2),
                  best_step=r[5].tolist()), a.out)


if __name__ == "__main__":
    main()
