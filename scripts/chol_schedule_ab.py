#!/usr/bin/env python3
"""A/B of the Cholesky driver against a differently built libmsfm.so (the parent commit's), on one GPU.

  python scripts/chol_schedule_ab.py --baseline-lib PATH [--parts timing,outputs,sweep,trace] [--out profiles/chol_schedule_ab.jsonl]

Every measurement is a fresh child process that loads one of the two libraries through MSFM_LIB, under its own time limit; the
libraries alternate parent, new, parent, new, ...; the script stops at the first child that does not exit with 0.  It appends
one JSON record per line, each with `library`, `run` and `note`:
  timing   ms_per_step of bench.py on the three workloads, `--runs` runs per library
  outputs  bench.py --dump-outputs after 12 and 30 steps of config 3 and 30 steps of config 5's window, with and without
           MSFM_CHOL_LAUNCHES=1: parent against new, byte by byte, file by file (`same_result`)
  sweep    the scenes of tests/test_gpu_ba.py::test_chain_barriers_pair_up and the 168-camera GPS scene, MSFM_CHOL_DOMAINS 0 / 1 / 2
           x MSFM_CHOL_LAUNCHES unset / 1, four iterations: costs, poses and points of both libraries byte by byte (`same_result`)
  trace    rocprofv3 --kernel-trace --stats runs, each a process of its own with no counters: the default workload twice per
           library, the MSFM_CHOL_LAUNCHES=1 workload once: calls and average time of the kernels of chol.hip
"""
import argparse
import csv
import glob
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHOL_KERNELS = ("k_chain", "k_panel_v2", "k_corner_syrk", "k_merge_corners", "k_trinv64_full", "k_backsolve_chain", "k_backsolve_pair",
                "k_backsolve_step", "k_fill_pending")
WORKLOADS = [   # name, bench.py arguments, environment
    ("c3", [], {}),
    ("c5_window", ["--config", "5", "--window"], {}),
    ("c3_full_launches", ["--full", "--no-cpu-baseline", "--no-matching", "--no-extras"], {"MSFM_CHOL_LAUNCHES": "1"}),
]
SWEEP_CHILD = r"""
import hashlib, json, os, sys
import numpy as np
sys.path.insert(0, %(root)r)
from metricsfm_amd import _abi as A, capi, scene
ctx = capi.Context(0)
cases = [(n, d, {}) for n, d in ((21, '0'), (22, '0'), (32, '0'), (43, '0'), (64, '0'), (75, '0'), (107, '0'), (150, '0'), (150, '1'))]
cases += [(168, d, 'gps') for d in ('0', '1', '2')]
out = {}
for n_cams, dom, kind in cases:
    os.environ['MSFM_CHOL_DOMAINS'] = dom
    if kind == 'gps':
        sc = scene.make_aerial_scene(168, 6000, seed=5, gps_sigma=0.5)
        kw = dict(gps_xyz=sc.gps_xyz, gps_weight=float(sc.n_obs // sc.n_cams))
    else:
        sc = scene.make_aerial_scene(n_cams, 30 * n_cams, seed=100 + n_cams)
        kw = {}
    for launches in ('', '1'):
        if launches: os.environ['MSFM_CHOL_LAUNCHES'] = '1'
        else: os.environ.pop('MSFM_CHOL_LAUNCHES', None)
        a = A.BaArrays.from_scene(sc, **kw)
        r = ctx.ba_solve(a, capi.default_options(max_num_iterations=4))
        h = hashlib.sha256()
        for x in (r['iterations']['cost'], a.cam_pose, a.point):
            h.update(np.ascontiguousarray(x).tobytes())
        out['%%d cameras%%s, domains %%s, launches %%s' %% (n_cams, ' + GPS' if kind else '', dom, launches or 'unset')] = h.hexdigest()
ctx.close()
print('SWEEP ' + json.dumps(out))
"""


def child(cmd, lib, env_extra, limit, cwd=ROOT):
    env = dict(os.environ, MSFM_LIB=lib, **env_extra)
    r = subprocess.run(cmd, env=env, cwd=cwd, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit("child %s exited with %d (library %s): stopping" % (" ".join(cmd[:3]), r.returncode, lib))
    return r.stdout


def last_json(text):
    for line in reversed(text.splitlines()):
        if line.startswith("{"):
            return json.loads(line)
    raise SystemExit("no JSON line in the child's output")


def dir_digest(d):
    return {os.path.basename(p): hashlib.sha256(open(p, "rb").read()).hexdigest() for p in sorted(glob.glob(os.path.join(d, "*")))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", required=True)
    ap.add_argument("--new-lib", default=os.path.join(ROOT, "metricsfm_amd", "libmsfm.so"))
    ap.add_argument("--parts", default="timing,outputs,sweep,trace")
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--limit", type=int, default=240, help="time limit of one child, seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chol_schedule_ab.jsonl"))
    ap.add_argument("--note", default="")
    args = ap.parse_args()
    libs = [("parent", os.path.abspath(args.baseline_lib)), ("new", os.path.abspath(args.new_lib))]
    parts = args.parts.split(",")
    bench = [sys.executable, os.path.join(ROOT, "bench.py")]

    def emit(rec):
        rec.setdefault("note", args.note)
        with open(args.out, "a") as f:
            f.write(json.dumps(rec) + "\n")
        print(json.dumps(rec), flush=True)

    if "timing" in parts:
        for name, argv, env in WORKLOADS:
            for run in range(1, args.runs + 1):
                for label, lib in libs:
                    j = last_json(child(bench + argv, lib, env, args.limit))
                    emit({"part": "timing", "workload": name, "library": label, "run": run, "ms_per_step": j["ms_per_step"],
                          "final_cost": j.get("final_cost")})
    if "outputs" in parts:
        for name, argv in (("c3 12 steps", ["--steps", "12"]), ("c3 30 steps", ["--steps", "30"]), ("c5 window 30 steps", ["--config", "5", "--window", "--steps", "30"])):
            for launches in ("", "1"):
                env = {"MSFM_CHOL_LAUNCHES": "1"} if launches else {}
                digests = {}
                with tempfile.TemporaryDirectory() as tmp:
                    for label, lib in libs:
                        d = os.path.join(tmp, label)
                        child(bench + argv + ["--dump-outputs", d], lib, env, args.limit)
                        digests[label] = dir_digest(d)
                emit({"part": "outputs", "case": name + (", MSFM_CHOL_LAUNCHES=1" if launches else ""), "library": "parent vs new", "run": 1,
                      "files": len(digests["new"]), "same_result": bool(digests["new"]) and digests["parent"] == digests["new"]})
    if "sweep" in parts:
        got = {}
        for label, lib in libs:
            text = child([sys.executable, "-c", SWEEP_CHILD % {"root": ROOT}], lib, {"MSFM_CHAIN_FORCE": "1"}, 3 * args.limit)
            got[label] = json.loads([l for l in text.splitlines() if l.startswith("SWEEP ")][-1][6:])
        for case in got["parent"]:
            emit({"part": "sweep", "case": case, "library": "parent vs new", "run": 1, "same_result": got["parent"][case] == got["new"].get(case)})
    if "trace" in parts:
        for name, argv, env in (WORKLOADS[0], WORKLOADS[2]):
            for label, lib, run in [(label, lib, run) for run in ((1, 2) if name == "c3" else (1,)) for label, lib in libs]:
                with tempfile.TemporaryDirectory() as tmp:
                    child(["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "t", "--output-format", "csv", "--"] + bench + argv, lib, env, 2 * args.limit)
                    stats = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
                    if not stats:
                        raise SystemExit("rocprofv3 wrote no kernel_stats.csv")
                    kernels = {}
                    for row in csv.DictReader(open(stats[0])):
                        short = row["Name"].split("(")[0].replace("void ", "")
                        if short.split("<")[0] in CHOL_KERNELS:
                            kernels[short] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3}
                emit({"part": "trace", "workload": name, "library": label, "run": run, "kernels": kernels})


if __name__ == "__main__":
    main()
