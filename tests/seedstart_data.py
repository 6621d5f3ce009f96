"""Cases for the start of a model (msfm_recon_create_from_seed, msfm_recon_normalize, incremental.start_model / reconstruct):
seed-pair stores of tests/seed_data.py in which the winner ranks behind a pair that fails, planted point clouds whose sums
depend on their order, and a store of two disjoint strips of images for whole models."""
import numpy as np

from metricsfm_amd import scene, seed
from tests import seed_data as D


def failing(n):
    """A pair with more matches than the winner, so SortImagePairs ranks it first, and no angle above 3 degrees: no point."""
    return dict(n=n, f=(D.F, D.F), kw=dict(baseline=2.0, **D.EXACT))


# name -> (specs, seed): hypothesis 0 fails, hypothesis 1 wins
SEED_CASES = {
    "gates": ([D.GATES[0], D.GATES[2]], 23),          # 20 points of 30 matches (the first 20: the features differ, pt_match does not)
    "dup": ([failing(400), D.MIXED[9]], 5),           # 301 matches, feature 3 in two of them; more points than one workgroup of 256
    "eight": ([failing(1800), D.MIXED[10]], 5),       # eight-point arm, two models, k1 / k2 not zero, about 1500 points
    "shared": ([failing(400), D.MIXED[11]], 5),       # one shared model: both f become the mean
}


def seed_case(name):
    specs, s = SEED_CASES[name]
    c = D.build_case(specs, s)
    n = len(c["n_features"])
    graph = np.zeros((n, n), np.int32)
    graph[c["pairs"][:, 0], c["pairs"][:, 1]] = np.diff(c["match_off"])
    f_of_image, k12 = np.zeros(n), np.zeros((n, 2))
    model_of_image = np.arange(n)
    for h, (i1, i2) in enumerate(c["hyp_img"].tolist()):
        f_of_image[[i1, i2]] = c["cam_fk"][h, :, 0]
        k12[[i1, i2]] = c["cam_fk"][h, :, 1:]
        if c["same_model"][h]:
            model_of_image[i2] = model_of_image[i1]
    by_pair = {tuple(p): c["matches"][c["match_off"][k]:c["match_off"][k + 1]] for k, p in enumerate(c["pairs"].tolist())}
    c.update(graph=graph, f_of_image=f_of_image, k12_of_image=k12, model_of_image=model_of_image, by_pair=by_pair)
    return c


def find(ctx, st, c, **kw):
    """seed.find_seed_pair on a seed_case; the ranked list is the case's hypothesis list."""
    n = len(c["n_features"])
    assert seed.sort_image_pairs(c["graph"], np.zeros(n, bool)).tolist() == c["hyp_img"].tolist()
    return seed.find_seed_pair(ctx, st, c["graph"], np.zeros(n, bool), c["f_of_image"], c["model_of_image"], keypoints=c["keypoints"],
                               k12_of_image=c["k12_of_image"], **kw)


def planted_points(P, s=7):
    """P points of order 1 to 10, a third of them shifted by +1e8 or -1e8 in equal numbers: the shifts cancel, and what is left
    of the small values depends on the order of the additions."""
    rng = np.random.default_rng(s)
    x = rng.normal(0.0, 5.0, (P, 3))
    k = P // 6
    idx = rng.permutation(P)[:2 * k]
    x[idx[:k]] += 1e8
    x[idx[k:]] -= 1e8
    return x


def chain_pairs(ctx, specs, s):
    """A store made from a chain - the keypoints inside it - for seed_data.pair_points pairs (specs: n and the keywords `kw`):
    pair h is images (2h, 2h + 1), SIFT-like descriptors per point, matched and verified on the device.  Returns the store,
    the chain (for its fetch_matches), the verified counts per pair, the host keypoints per image and `close`, which releases
    store, chain, match result and descriptor set in that order."""
    from metricsfm_amd import capi
    rng = np.random.default_rng(s)
    descs, kps = [], []
    for h, sp in enumerate(specs):
        x1, x2, _, _, _ = D.pair_points(rng, sp["n"], **sp.get("kw", {}))
        base = scene._sift_like(np.random.Generator(np.random.PCG64([s, h])), sp["n"]).astype(np.int16)
        d2 = np.clip(base + rng.integers(-4, 5, size=base.shape), 0, 255)
        descs += [base.astype(np.float32), d2.astype(np.float32)]
        kps += [np.ascontiguousarray(x1), np.ascontiguousarray(x2)]
    ds = ctx.descset(descs, keypoints=kps)
    res = ds.match_pairs(np.array([[2 * h, 2 * h + 1] for h in range(len(specs))], np.int32), 0.6, 0.85)
    ch = capi.Chain(res)
    n_m, _, _ = ch.verify(3.0, seed=5)
    st = capi.MatchStore.from_chain(ch)

    def close():
        st.close(); ch.close(); res.close(); ds.close()
    return st, ch, np.asarray(n_m, np.int32), kps, close


# ---- whole models: two strips of nadir images, 300 points each, no match between the strips.  7 images per strip: the seed's two
# and five more, the fewest at which images_added_total % 5 == 0 (sfm_incremental.cc:179-180) brings a full adjustment ----
STRIP_IMAGES, STRIP_POINTS, STRIP_F = 7, 300, 4800.0


def strips_case(s=3, noise=0.3):
    """Strip k: cameras 12 apart along x at height 0 looking along +z with rotations of about 0.002 rad (seed_data.pair_points
    says why the reference's seed needs that), points at depth 80..120 (adjacent images: 6.9 degrees), every point seen by every
    image of its strip: feature j of an image is point j of the strip.  Every pair of a strip is matched in both directions,
    without wrong matches: the Sampson sum the reference's five-point RANSAC scores with is not robust to gross outliers
    (seed_data.MIXED[13]).  Returns the store arrays, keypoints, the matches by pair and the settings of an incremental.Book."""
    rng = np.random.default_rng(s)
    n_img, P = 2 * STRIP_IMAGES, STRIP_POINTS
    kps, by_pair = [], {}
    for k in range(2):
        X = np.column_stack([rng.uniform(-30, 90, P), rng.uniform(-30, 30, P), rng.uniform(80.0, 120.0, P)])
        for i in range(STRIP_IMAGES):
            R = scene.angle_axis_to_R(rng.normal(0, 0.002, (1, 3)))[0]
            c = np.array([12.0 * i, 1.0 * (i % 2), 0.5 * (i % 3)]) + rng.normal(0, 0.3, 3)
            Xc = (X - c) @ R.T
            kps.append((STRIP_F * Xc[:, :2] / Xc[:, 2:3] + rng.normal(0, noise, (P, 2))).astype(np.float32))
        for i in range(STRIP_IMAGES):
            for j in range(i + 1, STRIP_IMAGES):
                m = np.column_stack([np.arange(P), np.arange(P)]).astype(np.int32)
                keep = rng.uniform(size=P) < 0.9 - 0.08 * (j - i)          # fewer matches over longer baselines
                a, b = k * STRIP_IMAGES + i, k * STRIP_IMAGES + j
                by_pair[(a, b)] = np.ascontiguousarray(m[keep])
                by_pair[(b, a)] = np.ascontiguousarray(m[keep][:, ::-1])   # the localisation reads (candidate, registered)
    order = sorted(by_pair)                                                # idx1 ascending, idx2 ascending
    pairs = np.array(order, np.int32)
    matches = [by_pair[p] for p in order]
    counts = [len(m) for m in matches]
    moff = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    match_count = np.zeros((n_img, n_img), np.int32)
    match_count[pairs[:, 0], pairs[:, 1]] = counts
    opts = dict(localize_opts=dict(max_tries=2), round_opts=dict(partial_options=dict(max_num_iterations=4), full_options=dict(max_num_iterations=4)))
    return dict(store=(np.full(n_img, P, np.int32), pairs, moff, np.concatenate(matches)), keypoints=np.concatenate(kps), by_pair=by_pair,
                book=dict(match_count=match_count, image_f=np.full(n_img, STRIP_F), image_f_init=np.full(n_img, STRIP_F), **opts))
