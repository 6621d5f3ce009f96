"""The tail of SLAMGPS::FeatureMatching step 2 (SfM/src/slam_gps.cc:503-541, geo_verification.cc:30-58) restated
sequentially on the codes of one pair, for tests/test_slam_chain_ref.py and tests/test_gpu_slam_chain.py.  Imports numpy and
the CPU oracle only, never the product.

Also the planted pairs both tests run on: a small world of 3-D points seen by eight cameras, images assembled feature by
feature so that the query count, the survivor count and the inlier count of every pair are chosen, not found."""
import numpy as np

from oracle import oracle as O

MIN_POINTS = 30      # geo_verification.cc:33
MIN_INLIERS = 30     # geo_verification.cc:53


def survivors(code):
    """pts1_init / pts2_init / matches[j] (slam_gps.cc:504-506): the walk over m, (train feature, query feature m)."""
    out = []
    for m in range(len(code)):
        if code[m] >= 0:
            out.append((int(code[m]), m))
    return np.array(out, dtype=np.int32).reshape(-1, 2)


def verify(pairs, codes, kps, **fransac):
    """Per pair: GeoVerificationFundamental on all survivors (:513), then matches[j] = {matches[j][inliers[k]]} whatever it
    returned (:514-518).  Fewer than 30 survivors: the function returns before RANSAC, `inliers` is empty, nothing is kept.
    Otherwise the mask of oracle.fundamental_ransac on the pair list (pair p = sampler index p) selects, verdict or not.
    Returns (kept matches per pair, n_matches, ok, F)."""
    n = len(pairs)
    surv = [survivors(c) for c in codes]
    off = np.zeros(n + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(s) for s in surv])
    if off[n] == 0:
        return [s[:0] for s in surv], np.zeros(n, np.int32), np.zeros(n, np.uint8), np.zeros((n, 3, 3))
    p1 = np.concatenate([np.asarray(kps[i], np.float32).reshape(-1, 2)[s[:, 0]] for (i, j), s in zip(pairs, surv)])
    p2 = np.concatenate([np.asarray(kps[j], np.float32).reshape(-1, 2)[s[:, 1]] for (i, j), s in zip(pairs, surv)])
    F, inl, nin, ok = O.fundamental_ransac(off, p1, p2, min_points=MIN_POINTS, min_inliers=MIN_INLIERS, **fransac)
    kept = []
    for p in range(n):
        s = surv[p]
        if len(s) < MIN_POINTS:
            kept.append(s[:0])
            continue
        sel = [k for k in range(len(s)) if inl[off[p] + k]]
        kept.append(s[sel].reshape(-1, 2))
    n_m = np.array([len(k) for k in kept], dtype=np.int32)
    assert (n_m == nin).all()
    return kept, n_m, ok, F


def tracks(pairs, kept):
    """The data association of SLAMGPS::Triangulation (:565-635) on the kept matches, pairs in order."""
    return O.build_tracks([(int(i), int(j)) for i, j in pairs], kept)


def match_graph(n_images, pairs, kept):
    g = np.zeros((n_images, n_images), dtype=np.int64)
    for (i, j), k in zip(pairs, kept):
        g[int(i), int(j)] = len(k)      # :540
    return g


def oracle_codes(descs, kps, pairs, F, H, th_ratio=0.80, th_epipolar=2.0, th_distance=5.0):
    """The three checks of step 2 (:469-503) per pair through oracle.knn2 + oracle.slam_gate.  A pair without query features
    has no codes."""
    codes = []
    for p, (i, j) in enumerate(pairs):
        if len(descs[j]) == 0:
            codes.append(np.zeros(0, np.int32))
            continue
        ids, sqd = O.knn2(descs[i], descs[j])
        code, _, _ = O.slam_gate(ids, sqd, kps[i], kps[j], F[p], H[p], th_ratio, th_epipolar, th_distance)
        codes.append(code)
    return codes


# ---------------------------------------------------------------------------------------------------------------------
# Planted pairs
# ---------------------------------------------------------------------------------------------------------------------
N_WORLD = 400
LOOSE = 1.0e9        # thresholds of the two prior gates where only the verification is under test
TH_RATIO = 0.5       # ratio check of the planted pairs: a planted survivor is an exact copy (ratio 0); of two random 128-d
                     # descriptors among a few hundred, the nearer is now and then below 0.80 of the next (squared distances),
                     # never below 0.5 - so the survivor counts are the planned ones


def _world(rng):
    X = np.column_stack([rng.uniform(-20, 20, N_WORLD), rng.uniform(-15, 15, N_WORLD), rng.uniform(30, 70, N_WORLD)])
    D = np.rint(rng.uniform(0, 255, (N_WORLD, 128))).astype(np.float32)
    return X, D


def _project(X, cam):
    """Centred pixels of a camera at c = (2.5 cam, 0.4 cam, 0) turned a little about y, focal length 1200."""
    a = 0.03 * (cam - 3)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    Xc = (X - np.array([2.5 * cam, 0.4 * cam, 0.0])) @ R.T
    return 1200.0 * Xc[:, :2] / Xc[:, 2:3]


def _image(rng, X, D, cam, n_feat, true_w, false_w=(), place=None):
    """An image of n_feat features: the world points true_w at their projections (+ 0.3 px), the world points false_w with
    their descriptors at random positions (survivors of the ratio check that no geometry explains), noise features (random
    descriptor, random position) for the rest.  place: the feature indices of the world points, in the order true_w +
    false_w (default: a random choice)."""
    w = list(true_w) + list(false_w)
    assert len(w) <= n_feat
    desc = np.rint(rng.uniform(0, 255, (n_feat, 128))).astype(np.float32)
    xy = np.column_stack([rng.uniform(-900, 900, n_feat), rng.uniform(-600, 600, n_feat)])
    slot = np.asarray(place if place is not None else rng.choice(n_feat, len(w), replace=False), dtype=np.int64)
    assert len(slot) == len(w) and len(set(slot.tolist())) == len(w)
    wid = np.full(n_feat, -1, dtype=np.int64)
    if len(w):
        desc[slot] = D[w]
        wid[slot] = w
        nt = len(true_w)
        xy[slot[:nt]] = _project(X[list(true_w)], cam) + rng.normal(0, 0.3, (nt, 2))
    return desc, np.ascontiguousarray(xy, dtype=np.float32), wid


def planted_pairs(seed=21):
    """Eight images and eleven (train, query) pairs.  Returns a dict: descs, kps, wid (world point of a feature or -1), pairs,
    want (the survivor count planned for each pair), F / H (loose priors: identity)."""
    rng = np.random.default_rng(seed)
    X, D = _world(rng)
    r = lambda a, b: list(range(a, b))
    imgs = [
        _image(rng, X, D, 0, 600, r(0, 300)),                                          # 0: the train image of most pairs
        _image(rng, X, D, 1, 600, r(0, 180), r(180, 200)),                             # 1: 200 survivors against 0, 20 of them false
        _image(rng, X, D, 2, 257, r(0, 31)),                                           # 2: 31 survivors
        (np.zeros((0, 128), np.float32), np.zeros((0, 2), np.float32), np.zeros(0, np.int64)),   # 3: no features
        _image(rng, X, D, 4, 256, r(40, 70)),                                          # 4: 30 survivors
        _image(rng, X, D, 5, 255, r(100, 129)),                                        # 5: 29 survivors
        _image(rng, X, D, 6, 1, r(7, 8)),                                              # 6: one feature, a survivor
        _image(rng, X, D, 7, 600, [], r(200, 240), place=512 + rng.choice(88, 40, replace=False)),   # 7: 40 false survivors, all in the last 256-chunk
    ]
    pairs = np.array([[0, 1], [0, 2], [0, 3], [0, 4], [0, 5], [0, 6], [0, 7], [1, 0], [2, 1], [5, 4], [4, 1]], dtype=np.int32)
    want = [200, 31, 0, 30, 29, 1, 40, 200, 31, 0, 30]
    n = len(pairs)
    return dict(descs=[i[0] for i in imgs], kps=[i[1] for i in imgs], wid=[i[2] for i in imgs], pairs=pairs, want=want,
                F=np.tile(np.eye(3), (n, 1, 1)), H=np.tile(np.eye(3), (n, 1, 1)))


def planted_reference(pl, **fransac):
    """codes, kept matches, n_matches, ok, F and tracks of the planted pairs by the restatement."""
    codes = oracle_codes(pl["descs"], pl["kps"], pl["pairs"], pl["F"], pl["H"], TH_RATIO, LOOSE, LOOSE)
    kept, n_m, ok, F = verify(pl["pairs"], codes, pl["kps"], **fransac)
    return dict(codes=codes, kept=kept, n_matches=n_m, ok=ok, F=F, tracks=tracks(pl["pairs"], kept))
