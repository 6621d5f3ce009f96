"""Timing of the SLAM + GPS registration steps (GetAccuracy, slam_gps.cc:1573-1594; the point loop of GPSRegistration2,
:933-978; the registration as a whole, :98-119), in the shape of the other stage benches.

  python scripts/gpsreg_bench.py [--reps 9] [--out FILE] [--no-c5] [--no-chain] [--chain-images 96]

One JSON line each:
  c5 / c2   msfm_point_accuracy_batch and msfm_gps_register_points on host arrays, at config 5's track shape (2 000 cameras,
            1 M points, 6 M rows, synthetic CSR) and on config 2's scene: wall time of the call with its uploads, synchronise and
            downloads (median / min / max of --reps after a warm-up), the kernel time of msfm_ctx_profile_get over --reps calls
            and the rows' algorithmic bytes (accuracy: 20 B per row + 46 B per track; shift: 4 B per row + 49 B per track)
            over it; and the sequential restatement tests/gpsreg_ref.cpp on one host thread
  chain     on the first --chain-images images of config 3's scene (every ordered pair, bench.py's resident-chain leg):
            each chain call, metricsfm_amd.gpsreg.slam_gps_register as a whole (12 iterations), and what a caller had before:
            fetch the tracks and points, the restatement's accuracy and shift on the host, msfm_ba_solve from host arrays"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from metricsfm_amd import _abi as A  # noqa: E402
from metricsfm_amd import capi, gpsreg, scene, window  # noqa: E402
from tests import gpsreg_data as D  # noqa: E402
from tests import gpsreg_ref as G  # noqa: E402

ITER = 12


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def stats(ts):
    return dict(wall_ms=round(float(np.median(ts)), 3), wall_ms_min=round(min(ts), 3), wall_ms_max=round(max(ts), 3))


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return r, ts


def synthetic_c5(n_cams=2000, n_tracks=1000000):
    """Config 5's track shape without its scene generator: lengths 2 .. 10 in scene.py's pattern (6 rows per track), a track's
    cameras a sorted run of neighbours on a line of nadir cameras, observations = projections + 1 px of noise."""
    rng = np.random.default_rng(55)
    lens = np.array([2, 3, 4, 5, 6, 6, 7, 8, 9, 10], np.int32)[np.arange(n_tracks) % 10]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    first = rng.integers(0, n_cams - 10, n_tracks)
    track_of_row = np.repeat(np.arange(n_tracks), lens)
    cam = (first[track_of_row] + (np.arange(off[-1]) - off[track_of_row])).astype(np.int32)
    c = np.column_stack([np.arange(n_cams) * 2.0, rng.normal(0, 0.3, n_cams), np.full(n_cams, 100.0)])
    R = np.tile(np.diag([1.0, -1.0, -1.0]).reshape(9), (n_cams, 1))
    t = -np.einsum("nij,nj->ni", R.reshape(-1, 3, 3), c)
    fk = np.tile([4800.0, 0.0, 0.0], (n_cams, 1))
    X = np.column_stack([2.0 * first + rng.uniform(0, 18, n_tracks), rng.uniform(-30, 30, n_tracks), rng.uniform(-5, 5, n_tracks)])
    uv, depth = scene.project_Rt(R[cam].reshape(-1, 3, 3), t[cam], fk[cam], X[track_of_row])
    assert (depth > 0).all()
    xy = uv + rng.normal(0, 1.0, uv.shape)
    gps = c + rng.normal(0, 0.5, c.shape)
    return A.TrackArrays(off, cam, xy, R, t, c, fk), X, np.ones(n_tracks, np.uint8), gps


def scene_c2():
    sc = scene.config_scene(2)
    R, t, c, fk = scene.cameras_for_tracks(sc)
    gps = c + np.random.default_rng(2).normal(0, 0.5, c.shape)
    return A.TrackArrays(sc.track_offsets(), sc.obs_cam, sc.obs_xy, R, t, c, fk), sc.point_gt.copy(), np.ones(sc.n_points, np.uint8), gps


def host_array_leg(ctx, L, name, T, X, ok, gps, reps, out):
    n, rows = T.struct.n_tracks, int(T.track_off[-1])
    shape = dict(what="gpsreg", part=name, cameras=len(T.cam_t), tracks=n, rows=rows)
    acc = lambda: ctx.point_accuracy(T, X, ok)  # noqa: E731
    a, ts = timed(acc, reps)
    emit(dict(shape, call="msfm_point_accuracy_batch", outliers=a[4], inliers=a[5], **stats(ts)), out)
    reg = lambda: ctx.gps_register_points(T.track_off, T.track_cam, a[3], T.cam_c, gps, X)  # noqa: E731
    Xs, ts = timed(reg, reps)
    emit(dict(shape, call="msfm_gps_register_points", **stats(ts)), out)
    # kernel time from the library's event pairs
    kern = {}
    ctx.profile(True)
    for _ in range(reps):
        ctx.profile_reset()
        acc(), reg()
        for k, v in ctx.profile_get().items():
            if k.startswith("gps_"):
                kern.setdefault(k, []).append(v["total_ms"] / max(1, v["launches"]))
    ctx.profile(False)
    bytes_ = dict(gps_accuracy=20 * rows + 46 * n, gps_register=4 * rows + 49 * n)
    ms = {k: float(np.median(v)) for k, v in kern.items()}
    emit(dict(shape, kernel_ms={k: round(v, 4) for k, v in ms.items()},
              algorithmic_GBps={k: round(bytes_[k] / (ms[k] * 1e-3) * 1e-9, 1) for k in ms if k in bytes_ and ms[k] > 0}), out)
    # the sequential restatement, one thread
    r, ts = timed(lambda: G.point_accuracy(L, T, X, ok), min(reps, 3))
    emit(dict(shape, call="restatement accuracy, one thread", same_bits=bool(all(np.array_equal(p, q) for p, q in zip(r, a))), **stats(ts)), out)
    r, ts = timed(lambda: G.register_points(L, T.track_off, T.track_cam, a[3], T.cam_c, gps, X), min(reps, 3))
    emit(dict(shape, call="restatement shift, one thread", same_bits=bool(np.array_equal(r, Xs)), **stats(ts)), out)


def chain_leg(ctx, L, n_img, reps, out):
    sc = scene.config_scene(3)
    scene.add_features(sc, 4096, images=range(n_img))
    kps = [np.ascontiguousarray(sc.kp_xy[i], np.float32) for i in range(n_img)]
    ds = ctx.descset([sc.desc[i] for i in range(n_img)], keypoints=kps)
    res = ds.match_pairs(scene.all_pairs(n_img), 0.6, 0.85)
    R, t, c, fk = (x[:n_img] for x in scene.cameras_for_tracks(sc))
    moc = sc.cam_model_of_cam[:n_img]
    gps = D.PLANTED_SCALE * c @ D.rodrigues(D.PLANTED_AA).T + D.PLANTED_T + np.random.default_rng(9).normal(0, D.GPS_NOISE, c.shape)
    opts = capi.default_options(max_num_iterations=ITER)
    o = capi.gps_orient_global(R, c, gps)
    _, _, pose = gpsreg.set_ac_pose(o["cam_aa"], o["gps"])

    def fresh():
        ch = capi.Chain(res)
        ch.verify(3.0)
        ch.build_tracks()
        return ch

    laps = {k: [] for k in ("orient_host", "triangulate", "accuracy", "gps_register", "ba_create_gps", "ba_run", "store_points", "accuracy_adjusted")}
    whole, before = [], []
    shape = None
    for rep in range(reps + 1):
        ch = fresh()
        lap = {}
        t0 = time.perf_counter(); capi.gps_orient_global(R, c, gps); lap["orient_host"] = time.perf_counter() - t0
        t0 = time.perf_counter(); ch.triangulate(o["cam_R"], o["cam_t"], o["cam_c"], fk, 3.0, gpsreg.TH_TRI_ANGLE); lap["triangulate"] = time.perf_counter() - t0
        t0 = time.perf_counter(); counts = ch.accuracy(o["cam_R"], o["cam_t"], fk); lap["accuracy"] = time.perf_counter() - t0
        t0 = time.perf_counter(); ch.gps_register(o["cam_c"], o["gps"]); lap["gps_register"] = time.perf_counter() - t0
        t0 = time.perf_counter(); ba = ch.ba_create(pose, sc.cam_model_gt, moc, gps_xyz=o["gps"]); lap["ba_create_gps"] = time.perf_counter() - t0
        t0 = time.perf_counter(); r = ba.run(opts); lap["ba_run"] = time.perf_counter() - t0
        t0 = time.perf_counter(); ch.store_points(ba); lap["store_points"] = time.perf_counter() - t0
        pose_adj, model_adj, _ = ba.download()
        R2, t2 = gpsreg.pose_cameras(pose_adj)
        t0 = time.perf_counter(); counts2 = ch.accuracy(R2, t2, model_adj[moc]); lap["accuracy_adjusted"] = time.perf_counter() - t0
        shape = dict(images=n_img, tracks=ch.n_tracks, rows=ch.n_obs, ba_points=len(ba.track_of_point), ba_rows=ba.n_obs, iterations=r["num_iterations"],
                     outliers=counts[0], outliers_adjusted=counts2[0])
        ba.close(); ch.close()
        # the driver as a whole
        ch = fresh()
        t0 = time.perf_counter()
        rec = gpsreg.slam_gps_register(ch, R, c, sc.cam_model_gt, moc, gps, options=opts)
        dt_whole = time.perf_counter() - t0
        rec["ba"].close(); ch.close()
        # before: leave the chain after the triangulation
        ch = fresh()
        ch.triangulate(o["cam_R"], o["cam_t"], o["cam_c"], fk, 3.0, gpsreg.TH_TRI_ANGLE)
        t0 = time.perf_counter()
        off, img, feat = ch.fetch_tracks()
        X0, _, ok0 = ch.fetch_points()
        xy = np.empty((len(img), 2))
        for i in range(n_img):
            sel = img == i
            xy[sel] = kps[i][feat[sel]]
        tr = A.TrackArrays(off, img, xy, o["cam_R"], o["cam_t"], o["cam_c"], fk)
        a = G.point_accuracy(L, tr, X0, ok0)
        X2 = G.register_points(L, off, img, a[3], o["cam_c"], o["gps"], X0)
        lens = np.diff(off)
        keep = (a[3] != 0) & (lens >= 3)
        sel = np.repeat(keep, lens)
        arrays = A.BaArrays(pose.copy(), sc.cam_model_gt.copy(), moc, X2[keep].copy(), img[sel], np.repeat(np.cumsum(keep) - 1, lens)[sel].astype(np.int32),
                            xy[sel], np.ones(int(keep.sum())), gps_xyz=o["gps"], gps_weight=window.gps_weight(int(sel.sum()), n_img))
        r_h = ctx.ba_solve(arrays, opts)
        X3 = X2.copy()
        X3[keep] = arrays.point
        R2, t2 = gpsreg.pose_cameras(arrays.cam_pose)
        G.point_accuracy(L, A.TrackArrays(off, img, xy, R2, t2, o["cam_c"], arrays.cam_model[moc]), X3, a[3])
        dt_before = time.perf_counter() - t0
        same = bool(np.array_equal(r_h["iterations"]["cost"], rec["summary"]["iterations"]["cost"]))
        ch.close()
        if rep:   # (the first pass warms up)
            for k, v in lap.items():
                laps[k].append(1e3 * v)
            whole.append(1e3 * dt_whole); before.append(1e3 * dt_before)
    emit(dict(what="gpsreg", part="chain", **shape, reps=reps, steps_ms={k: round(float(np.median(v)), 3) for k, v in laps.items()},
              slam_gps_register=stats(whole), host_arrays_from_the_triangulated_chain=stats(before), same_cost_trajectory=same), out)
    res.close(); ds.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-c5", action="store_true")
    ap.add_argument("--no-chain", action="store_true")
    ap.add_argument("--chain-images", type=int, default=96)
    ap.add_argument("--c5-tracks", type=int, default=1000000)
    a = ap.parse_args()
    ctx = capi.Context(0)
    with tempfile.TemporaryDirectory() as tmp:
        L = G.build_ref(tmp)
        host_array_leg(ctx, L, "c2", *scene_c2(), a.reps, a.out)
        if not a.no_c5:
            host_array_leg(ctx, L, "c5", *synthetic_c5(n_tracks=a.c5_tracks), a.reps, a.out)
        if not a.no_chain:
            chain_leg(ctx, L, a.chain_images, a.reps, a.out)
    ctx.close()


if __name__ == "__main__":
    main()
