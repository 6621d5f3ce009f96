"""Cases of the seed-pair tests: small match stores whose image pairs are synthetic two-view scenes, the hypothesis lists over
them, and the expected answer - the poses from oracle.relpose_5pt and tests/relposef_ref.cpp on the "other arm is empty"
batches msfm_seed_hypotheses is defined by, everything else from the sequential restatement tests/seed_ref.cpp."""
import numpy as np

from tests import relposef_data as RF
from tests import seed_ref as SR
from tests.twoview import rodrigues

F = 4800.0
SEED_E5, SEED_F8 = 0x4D53464D45, 0x4D53464D38     # the defaults of Context.relpose_5pt / relpose_8pt
OPTS = dict(th_mse_reprojection=3.0, th_angle_small=3.0 / 180.0 * 3.1415, th_seedpair_structures=20, ransac_times_5pt=100,
            ransac_times_8pt=200, seed_5pt=SEED_E5, seed_8pt=SEED_F8)


def pair_points(rng, n, baseline=10.0, noise=0.5, outlier_frac=0.1, f=(F, F), depth=(80.0, 120.0), far=0, rot=0.002):
    """tests/twoview.make_relpose_batch's pair: n points at depth 80..120 seen by two cameras `baseline` apart (10 at depth 100
    is a 5.7 degree angle: passes the 3 degree gate; 2 is 1.1 degrees: fails it).  The last `far` points lie at depth 4000..6000
    instead: they agree with the pair's geometry and fail the angle gate.  The rotation is small (sigma `rot` rad per axis, where
    make_relpose_batch has 0.05): the t the estimators return is -R^T u3 of the decomposition
    (relative_pose_from_essential_matrix.cc:51-54), which :334 then uses as the translation, so a pair reconstructs below
    th_mse_reprojection only while R^T t is close to t.  Returns x1, x2 (float32 centred pixels), R, t, X."""
    X = np.column_stack([rng.uniform(-40, 40, n), rng.uniform(-30, 30, n), rng.uniform(depth[0], depth[1], n)])
    if far:
        X[n - far:] *= 50.0
    R = rodrigues(rng.normal(0, rot, 3))
    t = np.array([baseline, 0.1 * baseline, 0.05 * baseline]) + rng.normal(0, 0.05 * baseline, 3)
    x1 = f[0] * X[:, :2] / X[:, 2:3] + rng.normal(0, 1.0, (n, 2)) * noise
    Xc = X @ R.T + t
    x2 = f[1] * Xc[:, :2] / Xc[:, 2:3] + rng.normal(0, 1.0, (n, 2)) * noise
    nout = int(round(outlier_frac * n))
    if nout:
        bad = rng.choice(n, nout, replace=False)
        x2[bad] = np.column_stack([rng.uniform(-2000, 2000, nout), rng.uniform(-1500, 1500, nout)])
    return x1.astype(np.float32), x2.astype(np.float32), R, t, X


def generic_points(rng, n, noise=0.5, outlier_frac=0.0, **kw):
    """tests/relposef_data.make_pair: a second view whose axis neither parallels nor meets the first's (Hartley's focal lengths
    exist), f = 4800 / 4200, baseline about 42."""
    x1, x2, R, t, X = RF.make_pair(rng, n, noise=noise, outlier_frac=outlier_frac, **kw)
    return x1.astype(np.float32), x2.astype(np.float32), R, t, X


def build_case(specs, seed):
    """specs: one dict per hypothesis -
         n        matches of the pair;  absent=True: the pair is not in the store at all
         f        (f1, f2) handed to the call, 0.0 = unknown;  k = ((k1, k2), (k1, k2)) distortion, default zeros
         same     same_model
         kind     "calib" (pair_points; its keywords in `kw`) or "generic" (generic_points)
         dup      True: match 3 once more at the end of the list (a feature in two matches; a wrong partner would be a gross
                  outlier, and the estimators' Sampson sum is not robust to one)
       Every hypothesis owns two images; image 1's features are the matches in order plus 5 unmatched ones, image 2's are a
       permutation.  Two spare images without any pair close the store: (n_images - 2, n_images - 1) is always absent.
       Returns a dict with the store (n_features, pairs, match_off, matches), keypoints (flat float32), hyp_img, cam_fk,
       same_model and `truth` (R, t, X per hypothesis, None where there is none)."""
    rng = np.random.default_rng(seed)
    n_features, kps, pairs, counts, matches, hyp, fk, same, truth = [], [], [], [], [], [], [], [], []
    for h, s in enumerate(specs):
        n = s["n"]
        i1, i2 = 2 * h, 2 * h + 1
        if s.get("kind", "calib") == "generic":
            x1, x2, R, t, X = generic_points(rng, n, **s.get("kw", {}))
        else:
            x1, x2, R, t, X = pair_points(rng, n, **s.get("kw", {}))
        extra = rng.uniform(-1500, 1500, (5, 2)).astype(np.float32)
        perm = rng.permutation(n)
        k2 = np.zeros((n, 2), np.float32)
        k2[perm] = x2                                   # feature perm[j] of image 2 is match j's point
        kps += [np.concatenate([x1, extra]), np.concatenate([k2, extra])]
        n_features += [n + 5, n + 5]
        m = np.column_stack([np.arange(n), perm]).astype(np.int32)
        if s.get("dup"):
            m = np.concatenate([m, np.array([[3, perm[3]]], np.int32)])
        if not s.get("absent"):
            pairs.append((i1, i2)); counts.append(len(m)); matches.append(m)
        hyp.append((i1, i2))
        kk = s.get("k", ((0.0, 0.0), (0.0, 0.0)))
        fk.append([[s["f"][0], *kk[0]], [s["f"][1], *kk[1]]])
        same.append(1 if s.get("same") else 0)
        truth.append(None if s.get("absent") else (R, t, X))
    for _ in range(2):
        kps.append(np.zeros((1, 2), np.float32)); n_features.append(1)
    return dict(n_features=np.array(n_features, np.int32), pairs=np.array(pairs, np.int32).reshape(-1, 2),
                match_off=np.concatenate([[0], np.cumsum(counts)]).astype(np.int32),
                matches=np.concatenate(matches) if matches else np.zeros((0, 2), np.int32),
                keypoints=np.concatenate(kps), hyp_img=np.array(hyp, np.int32).reshape(-1, 2),
                cam_fk=np.array(fk, np.float64).reshape(-1, 2, 3), same_model=np.array(same, np.uint8), truth=truth)


def store_args(c):
    return c["n_features"], c["pairs"], c["match_off"], c["matches"]


def absent_pair(c):
    n = len(c["n_features"])
    return (n - 2, n - 1)


# the mixed batch of tests/test_gpu_seed.py: match counts 0 (pair not in the store), 4, 5, 9, 10 (five-point arm: fails below 5,
# all matches at once up to 9, sampled from 10), 7, 8, 15, 16 (eight-point arm likewise around 8 and 16), 300 and 1500
K1 = ((1e-4, 0.0), (0.0, -2e-4))
# the eight-point arm needs optical axes that neither parallel nor meet, the reconstruction a small rotation (pair_points): this
# rotation with relposef_data's centre (38, -14, 9) gives both - focal lengths to 1e-5, most points below th_mse_reprojection
SMALL_ROT = dict(rot=np.array([0.004, -0.006, 0.003]), jitter=0.0, noise=0.1)
MIXED = [
    dict(n=40, f=(F, F), absent=True),
    dict(n=4, f=(F, F), kw=dict(outlier_frac=0.0)),
    dict(n=5, f=(F, F), kw=dict(outlier_frac=0.0)),
    dict(n=9, f=(F, F), same=True, kw=dict(outlier_frac=0.0)),
    dict(n=10, f=(F, F), kw=dict(outlier_frac=0.0)),
    dict(n=7, f=(0.0, 0.0), kind="generic"),
    dict(n=8, f=(0.0, 0.0), kind="generic"),
    dict(n=15, f=(F, 0.0), kind="generic"),                       # a known f beside an unknown one: eight-point arm, both replaced
    dict(n=16, f=(0.0, 0.0), same=True, kind="generic"),
    dict(n=300, f=(F, F), same=True, dup=True, k=K1, kw=dict(outlier_frac=0.0)),   # 301 matches, feature 3 in two of them
    dict(n=1500, f=(0.0, 4200.0), kind="generic", kw=SMALL_ROT, k=K1),
    dict(n=300, f=(0.0, 0.0), same=True, kind="generic", kw=dict(f_cur=4800.0, **SMALL_ROT)),   # both f become (f1 + f2) / 2
    dict(n=1500, f=(F, F), kw=dict(outlier_frac=0.0)),
    dict(n=300, f=(F, F), kw=dict(outlier_frac=0.1)),             # gross outliers: the Sampson SUM (:333-349) is not robust to them
]
MIXED_COUNTS = [0, 4, 5, 9, 10, 7, 8, 15, 16, 301, 1500, 300, 1500, 300]

# the gates (:380-381) with exact geometry: no noise, no outliers; points beyond depth 4000 fail the 3 degree angle gate
EXACT = dict(noise=0.0, outlier_frac=0.0)
GATES = [
    dict(n=100, f=(F, F), kw=dict(baseline=2.0, **EXACT)),        # every angle under 3 degrees: no point at all
    dict(n=29, f=(F, F), kw=dict(far=10, **EXACT)),               # 19 points: one short of th_seedpair_structures
    dict(n=30, f=(F, F), kw=dict(far=10, **EXACT)),               # 20 points: passes (30 / 5 = 6)
    dict(n=150, f=(F, F), kw=dict(far=125, **EXACT)),             # 25 points >= 20, but 150 / 5 = 30 decides
    dict(n=129, f=(F, F), kw=dict(far=104, **EXACT)),             # 25 points, 129 / 5 = 25 (integer division): passes
]
GATES_POINTS = [0, 19, 20, 25, 25]
GATES_PASS = [0, 0, 1, 0, 1]


def arm_batches(hyp_arm, n_matches, pts1, pts2):
    """The two calls msfm_seed_hypotheses is defined by: offsets over ALL hypotheses, the other arm's segments empty."""
    off_all = np.concatenate([[0], np.cumsum(n_matches)])
    out = {}
    for arm in (5, 8):
        cnt = np.where(hyp_arm == arm, n_matches, 0)
        off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
        sel = [np.arange(off_all[h], off_all[h + 1]) for h in range(len(cnt)) if hyp_arm[h] == arm]
        sel = np.concatenate(sel).astype(np.int64) if sel else np.zeros(0, np.int64)
        out[arm] = (off, np.ascontiguousarray(pts1[sel]), np.ascontiguousarray(pts2[sel]))
    return out


def merge_poses(hyp_arm, five, eight):
    """five = (E, R, t, ok, nc) of relpose_5pt, eight = (F, f1, f2, E, R, t, ok, ...) of relpose_8pt -> pose_ok, R, t, f8 per hypothesis"""
    is5 = hyp_arm == 5
    pose_ok = np.where(is5, five[3], eight[6]).astype(np.uint8)
    R = np.where(is5[:, None, None], five[1], eight[4])
    t = np.where(is5[:, None], five[2], eight[5])
    f8 = np.column_stack([eight[1], eight[2]])
    return pose_ok, R, t, f8


def expected(O, L8, LS, c, hyp_img=None, cam_fk=None, same_model=None, **opts):
    """The whole answer for case c (optionally another hypothesis list over its store).  O: oracle module, L8 / LS: the loaded
    tests/relposef_ref.cpp / tests/seed_ref.cpp."""
    o = dict(OPTS, **opts)
    hyp = c["hyp_img"] if hyp_img is None else np.asarray(hyp_img, np.int32).reshape(-1, 2)
    fk = c["cam_fk"] if cam_fk is None else np.asarray(cam_fk, np.float64).reshape(-1, 2, 3)
    same = c["same_model"] if same_model is None else np.asarray(same_model, np.uint8)
    nm, p1, p2 = SR.gather(LS, *store_args(c), c["keypoints"], hyp)
    arm = np.where((fk[:, 0, 0] != 0) & (fk[:, 1, 0] != 0), 5, 8)
    b = arm_batches(arm, nm, p1, p2)
    five = O.relpose_5pt(*b[5], fk[:, 0, 0], fk[:, 1, 0], ransac_times=o["ransac_times_5pt"], seed=o["seed_5pt"])
    eight = RF.ref_relpose_8pt(L8, *b[8], ransac_times=o["ransac_times_8pt"], seed=o["seed_8pt"])
    pose_ok, R, t, f8 = merge_poses(arm, five, eight)
    return SR.reconstruct(LS, *store_args(c), c["keypoints"], hyp, fk, same, pose_ok, R, t, f8, o["th_mse_reprojection"],
                          o["th_angle_small"], o["th_seedpair_structures"])


def two_view_tracks(c, r, hyp_img=None):
    """The accepted and rejected matches of result r alike as two-view tracks for triangulate_midpoint: per hypothesis with a
    pose two cameras (2h: [I|0], 2h + 1: the returned pose), one track per match.  Returns (TrackArrays arguments, hypothesis
    of every track, match index of every track)."""
    hyp = c["hyp_img"] if hyp_img is None else np.asarray(hyp_img, np.int32).reshape(-1, 2)
    first = np.concatenate([[0], np.cumsum(c["n_features"])])
    kp = c["keypoints"].astype(np.float64)
    store = {tuple(p): k for k, p in enumerate(c["pairs"].tolist())}
    n = len(hyp)
    cam_R = np.tile(np.eye(3), (2 * n, 1, 1)); cam_t = np.zeros((2 * n, 3)); cam_c = np.zeros((2 * n, 3)); cam_fk = np.zeros((2 * n, 3))
    cam_fk[:, 0] = 1.0
    xy, cam, th, tm = [], [], [], []
    for h in range(n):
        cam_fk[2 * h, 0], cam_fk[2 * h + 1, 0] = r["f"][h]
        cam_fk[2 * h, 1:], cam_fk[2 * h + 1, 1:] = c["cam_fk"][h, 0, 1:], c["cam_fk"][h, 1, 1:]
        if not r["pose_ok"][h]:
            continue
        cam_R[2 * h + 1], cam_t[2 * h + 1], cam_c[2 * h + 1] = r["R"][h], r["t"][h], r["c"][h]
        k = store.get(tuple(hyp[h].tolist()))
        if k is None:
            continue
        m = c["matches"][c["match_off"][k]:c["match_off"][k + 1]]
        a, b = kp[first[hyp[h, 0]] + m[:, 0]], kp[first[hyp[h, 1]] + m[:, 1]]
        xy.append(np.stack([a, b], axis=1).reshape(-1, 2))
        cam.append(np.tile([2 * h, 2 * h + 1], len(m)))
        th.append(np.full(len(m), h)); tm.append(np.arange(len(m)))
    xy, cam, th, tm = np.concatenate(xy), np.concatenate(cam).astype(np.int32), np.concatenate(th), np.concatenate(tm)
    off = (2 * np.arange(len(th) + 1)).astype(np.int32)
    return (off, cam, xy, cam_R, cam_t, cam_c, cam_fk), th, tm


def host_check_command(exe):
    """The compiler call for tests/seed_host_check.cc against this tree's library."""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "metricsfm_amd")
    return ["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(root, "host"), "-I", os.path.join(root, "include"),
            os.path.join(root, "tests", "seed_host_check.cc"), os.path.join(root, "host", "objectsfm.cc"), "-o", str(exe),
            "-L" + lib, "-lmsfm", "-Wl,-rpath," + lib, "-Wl,-rpath-link,/opt/rocm/lib"]


def write_image_set(path, c, image_focal, image_model, seed_chunk):
    """An image set in the byte layout tests/seed_host_check.cc reads."""
    with open(path, "wb") as fh:
        for x in ([len(c["n_features"])], c["n_features"], [len(c["pairs"])], c["pairs"], c["match_off"], c["matches"], image_model, [seed_chunk]):
            np.ascontiguousarray(np.asarray(x, dtype=np.int32)).tofile(fh)
        np.ascontiguousarray(image_focal, dtype=np.float64).tofile(fh)
        np.ascontiguousarray(c["keypoints"], dtype=np.float32).tofile(fh)


def read_seed_result(path):
    """What seed_host_check.cc wrote, as a dict."""
    raw = open(path, "rb").read()
    head = np.frombuffer(raw, np.int32, 6)
    found, i1, i2, visited, P, n_models = (int(v) for v in head)
    pos = 24
    gid = np.frombuffer(raw, np.int32, 2 * P, pos).reshape(-1, 2); pos += 8 * P
    f = np.frombuffer(raw, np.float64, n_models, pos); pos += 8 * n_models
    out = dict(found=bool(found), images=(i1, i2), n_visited=visited, global_ids=gid, f=f)
    if found:
        pose = np.frombuffer(raw, np.float64, 15, pos); pos += 120
        out.update(R=pose[:9].reshape(3, 3), t=pose[9:12], c=pose[12:15])
    out["X"] = np.frombuffer(raw, np.float64, 3 * P, pos).reshape(-1, 3); pos += 24 * P
    out["mse"] = np.frombuffer(raw, np.float64, P, pos); pos += 8 * P
    assert pos == len(raw)
    return out


GOLDEN = [MIXED[2], MIXED[4], MIXED[6], MIXED[8], MIXED[11], GATES[2]]
GOLDEN_INPUTS = ("n_features", "pairs", "match_off", "matches", "keypoints", "hyp_img", "cam_fk", "same_model")


def write_golden(path, O, L8, LS):
    """tests/golden/seed_golden.npz: a six-hypothesis case and the restatement's answer (python -c "..." from the repository root;
    tests/test_gpu_seed.py::test_golden_fixture reads it)."""
    c = build_case(GOLDEN, 41)
    want = expected(O, L8, LS, c)
    np.savez_compressed(path, **{k: c[k] for k in GOLDEN_INPUTS}, **{"want_" + k: np.asarray(v) for k, v in want.items()})
