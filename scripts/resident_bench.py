"""One whole round of IncrementalSfM::Run (sfm_incremental.cc:126-186) at BASELINE config 3 through the flat state and through
the resident one (msfm_recon), in one process: images 0-249 registered with every point two of them see (70 % of those, as
scripts/newpoints_bench.py draws them), image 250 the one candidate.  The round localises it, registers it, generates its new
points and runs the partial adjustment with the outlier stage, through `metricsfm_amd/incremental.py`:

  python scripts/resident_bench.py [--reps 9] [--out profiles/resident_bench.jsonl]

  flat      FlatBackend: localize_next_image, apply_localized_image, generate_new_points + apply_new_points, adjust_round +
            apply_round - every call uploads what it reads of the state, numpy writes the results back
  resident  ResidentBackend: Recon.localize, commit_camera, new_points, adjust on the arrays a Recon keeps on the device
Every repetition starts from the same state (a copy of the dict; a Recon made anew, its creation timed apart: it is paid once
per model).  One JSON line per backend with the box record the other benches write: wall time of each of the four calls and of
the round as median / min / max of --reps after a warm-up, the bytes each call sent, for the resident backend the kernel split
of msfm_ctx_profile_get from one further round, and whether both backends left the same state."""
import argparse
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from metricsfm_amd import capi, incremental, scene  # noqa: E402
from metricsfm_amd.tracks import flat_matches_from_scene  # noqa: E402
from tests import resident_data as RD  # noqa: E402

N_REGISTERED = 250
CALLS = ("localize", "commit_camera", "new_points", "adjust")


def build_round():
    sc = scene.config_scene(3)
    nf, pairs, moff, m = flat_matches_from_scene(sc)
    rng = np.random.default_rng(3)
    by_cam = np.argsort(sc.obs_cam, kind="stable")                 # feature f of image c = its f-th observation
    start = np.concatenate([[0], np.cumsum(nf)])
    seen = np.bincount(sc.obs_pt[sc.obs_cam < N_REGISTERED], minlength=sc.n_points)
    exists = (seen >= 2) & (rng.random(sc.n_points) < 0.7)
    pid = sc.obs_pt[by_cam]
    feat_pid = [pid[start[c]:start[c + 1]] for c in range(N_REGISTERED)]
    match_count = np.zeros((sc.n_cams, sc.n_cams), np.int32)      # image 250 is the one candidate
    lo, hi = np.searchsorted(pairs[:, 0], [N_REGISTERED, N_REGISTERED + 1])
    match_count[pairs[lo:hi, 1], N_REGISTERED] = np.diff(moff)[lo:hi]
    c = RD.scene_model(sc, N_REGISTERED, nf, feat_pid, sc.obs_xy[by_cam], exists, match_count)
    c["store"] = (nf, pairs, moff, m)
    return c


class Timed:
    """A backend whose four calls are timed, with the bytes each sent (resident: from Recon.size; flat: what the call reports)."""

    def __init__(self, backend):
        self.b, self.ms, self.sent = backend, {}, {}

    def __getattr__(self, name):
        fn = getattr(self.b, name)
        if name not in CALLS:
            return fn

        def call(*a, **kw):
            rec = getattr(self.b, "recon", None)
            before = rec.size()["h2d_bytes"] if rec is not None else None
            t0 = time.perf_counter()
            r = fn(*a, **kw)
            self.ms[name] = (time.perf_counter() - t0) * 1e3
            if rec is not None:
                self.sent[name] = rec.size()["h2d_bytes"] - before
            elif isinstance(r, dict) and "h2d_bytes" in r:
                self.sent[name] = int(r["h2d_bytes"])
            return r
        return call


def stats(ts):
    return dict(ms=round(float(np.median(ts)), 3), ms_min=round(min(ts), 3), ms_max=round(max(ts), 3))


def emit(rec, out):
    import json
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resident_bench.jsonl"))
    a = ap.parse_args()
    c = build_round()
    ctx = capi.Context(0)
    store = ctx.match_store(*c["store"])
    args = (ctx, store, c["state"], c["cam_pose"], c["cam_model"], c["cam_model_of_cam"])
    n_pts, n_rows = len(c["state"]["pt_bad"]), len(c["state"]["obs_point"])

    def one(kind, profile=False):
        t0 = time.perf_counter()
        if kind == "flat":
            back = incremental.FlatBackend(*args, keypoints=c["keypoints"])
        else:
            back = incremental.ResidentBackend(*args, keypoints=c["keypoints"], reserve_points=n_pts + 16384, reserve_obs=n_rows + 65536)
        create_ms = (time.perf_counter() - t0) * 1e3
        try:
            created = back.recon.size()["h2d_bytes"] if kind == "resident" else 0
            timed = Timed(back)
            if profile:
                ctx.profile(True); ctx.profile_reset()
            t0 = time.perf_counter()
            rec = incremental.run_round(timed, incremental.Book(**c["book"]))
            round_ms = (time.perf_counter() - t0) * 1e3
            prof = ctx.profile_get() if profile else None
            if profile:
                ctx.profile(False)
            return dict(ms=timed.ms, sent=timed.sent, round_ms=round_ms, create_ms=create_ms, created=created, rec=rec, state=back.fetch(), prof=prof)
        finally:
            if kind == "resident":
                back.close()

    runs = {"flat": [], "resident": []}
    one("flat"); one("resident")
    for _ in range(a.reps):
        for kind in runs:
            runs[kind].append(one(kind))
    prof = one("resident", profile=True)["prof"]
    f, r = runs["flat"][-1], runs["resident"][-1]
    same = all(np.array_equal(f["state"][k], r["state"][k]) for k in RD.FETCHED)
    # the flat localisation reports no byte count of its own: its search is one msfm_localize_candidates call on these arrays
    st = c["state"]
    cand = np.array([N_REGISTERED], np.int32)
    flat_search = ctx.localize_candidates(store, st["cam_img"], st["feat_point"], st["pt_bad"], st["pt_mse"], st["pt_views"], cand, [0],
                                          point_xyz=st["point_xyz"], keypoints=c["keypoints"])["h2d_bytes"]
    rec = f["rec"]
    shape = dict(box=socket.gethostname(), cameras=N_REGISTERED, points=n_pts, rows=n_rows, image=rec["image"], visible=len(rec["visible"]),
                 n_inliers=rec["n_inliers"], new_points=rec["n_new"], iterations=int(rec["summary"][0]["num_iterations"]), outliers=rec["count_outliers"])
    for kind in runs:
        last = runs[kind][-1]
        line = dict(what="resident_round", backend=kind, reps=a.reps, round=stats([x["round_ms"] for x in runs[kind]]),
                    calls={k: stats([x["ms"][k] for x in runs[kind]]) for k in CALLS}, h2d_bytes=dict(last["sent"]), **shape)
        if kind == "flat":
            line["h2d_bytes"]["localize_search_only"] = int(flat_search)
        else:
            line.update(create=stats([x["create_ms"] for x in runs[kind]]), create_h2d_bytes=int(last["created"]), same_state_as_flat=bool(same),
                        kernels_ms={k: round(v["total_ms"], 3) for k, v in prof.items()})
        emit(line, a.out)
    store.close(); ctx.close()


if __name__ == "__main__":
    main()
