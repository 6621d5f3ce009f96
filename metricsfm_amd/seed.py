"""IncrementalSfM::FindSeedPairThenReconstruct (sfm_incremental.cc:224-415), Python host side: the order in which the image
pairs are tried (`sort_image_pairs`, SortImagePairs :1790-1829), the hypotheses of a list in one msfm_seed_hypotheses call on
a resident match store (`seed_hypotheses`), and the walk down the ranked list in chunks until one reconstructs
(`find_seed_pair`), which hands back the seed model in the layout `_abi.BaArrays` takes."""
import math

import numpy as np

from . import capi, scene


def sort_image_pairs(match_graph, processed):
    """:1790-1829, literally.  match_graph [n][n] = graph_.match_graph_ (int), processed [n] = is_img_processed_.
    strength_i = (float)log(row sum + 2.0), the row sum accumulated in binary32 left to right (math::sum, basic_funcs.h:50-57);
    pair strength = (float)((float)(s_i * s_j) * log((double)n_ij)) over i < j, neither processed, n_ij != 0; descending.
    std::sort leaves ties open: here they go to the lower i * n + j.  The C library's log (math.log), not numpy's vectorised
    one, so that the C++ host gets the same order.  Returns an int32 array [n_hyp][2] of (id_img1, id_img2)."""
    g = np.asarray(match_graph)
    n = len(g)
    processed = np.asarray(processed, dtype=bool)
    f32 = np.float32
    strength = []
    for i in range(n):
        s = f32(0.0)
        for j in range(n):
            s = f32(s + f32(g[i, j]))
        strength.append(f32(math.log(float(s) + 2.0)))
    pairs = []
    for i in range(n - 1):
        if processed[i]:
            continue
        for j in range(i + 1, n):
            nij = int(g[i, j])
            if not nij or processed[j]:
                continue
            st = f32(float(f32(strength[i] * strength[j])) * math.log(float(nij)))
            pairs.append((i * n + j, st))
    pairs.sort(key=lambda p: (-float(p[1]), p[0]))
    return np.array([(k // n, k % n) for k, _ in pairs], dtype=np.int32).reshape(-1, 2)


def seed_hypotheses(ctx: capi.Context, store, hyp_img, cam_fk, same_model, keypoints=None, **opts):
    """`Context.seed_hypotheses`: a dict of arrays, one row per hypothesis (include/msfm.h, msfm_seed_hypotheses)."""
    return ctx.seed_hypotheses(store, hyp_img, cam_fk, same_model, keypoints=keypoints, **opts)


def find_seed_pair(ctx: capi.Context, store, match_graph, processed, f_of_image, model_of_image, k=64, keypoints=None,
                   k12_of_image=None, pair_matches=None, image_keypoints=None, keep=False, **opts):
    """FindSeedPairThenReconstruct up to and including its gates (:224-390).  The ranked pairs go to the device in chunks of
    `k` until a chunk has a winner; every chunk is a call of its own, so a hypothesis' sample key is its index in its chunk.
    f_of_image [n] (0 = unknown), model_of_image [n] (ids of CameraAssociateCameraModel; two images with the same id share
    a model), k12_of_image [n][2] (default zeros), keypoints: flat float [sum of n_features][2] for a store not made from a chain.
    The observations of the winner - and only of the winner - are read on the host: pair_matches(i1, i2) -> int [n][2], the
    stored matches of that pair (e.g. `Chain.fetch_matches` of its pair index), image_keypoints(i) -> float [n_features][2];
    with `keypoints` given, image_keypoints defaults to its rows.  Without pair_matches the observation arrays are left out.
    Returns None when no pair passes, else a dict:
      images (id_img1, id_img2); n_visited = hypotheses the reference's loop would have visited (the winner included);
      cam_pose [2][6] (angle-axis, t), cam_model [n_models][3] (f, k1, k2), cam_model_of_cam [2], cam_R, cam_t, cam_c;
      point [P][3], mse [P], obs_cam / obs_pt [2P], obs_xy [2P][2] (camera 0's observation of a point first), obs_feature [2P]
      (feature index inside its image), pt_match [P]: what `_abi.BaArrays(cam_pose, cam_model, cam_model_of_cam, point, obs_cam,
      obs_pt, obs_xy)` takes; hypotheses = the chunk's full answer.
    keep=True: the winning chunk's `capi.SeedSet` stays alive under "set" (the caller closes it), so `capi.Recon.from_seed` makes
    the model's state on the device and no pair_matches callback is needed."""
    if k < 1:
        raise ValueError("k must be at least 1")
    hyps = sort_image_pairs(match_graph, processed)
    f_of_image = np.asarray(f_of_image, dtype=np.float64)
    model_of_image = np.asarray(model_of_image)
    k12 = np.zeros((len(f_of_image), 2)) if k12_of_image is None else np.asarray(k12_of_image, dtype=np.float64).reshape(-1, 2)
    for c0 in range(0, len(hyps), k):
        chunk = hyps[c0:c0 + k]
        fk = np.zeros((len(chunk), 2, 3))
        fk[:, :, 0] = f_of_image[chunk]
        fk[:, :, 1:] = k12[chunk]
        same = model_of_image[chunk[:, 0]] == model_of_image[chunk[:, 1]]
        r = ctx.seed_hypotheses(store, chunk, fk, same, keypoints=keypoints, keep=keep, **opts)
        w = r["winner"]
        if w < 0:
            if keep:
                r.pop("set").close()
            continue
        i1, i2 = (int(v) for v in chunk[w])
        b, e = r["pt_off"][w], r["pt_off"][w + 1]
        P = int(e - b)
        shared = bool(same[w])
        R1, t1 = r["R"][w], r["t"][w]
        cam_model = np.array([[r["f"][w, 0], *k12[i1]]]) if shared else np.array([[r["f"][w, 0], *k12[i1]], [r["f"][w, 1], *k12[i2]]])
        out = dict(images=(i1, i2), n_visited=c0 + w + 1,
                   cam_pose=np.array([np.zeros(6), np.concatenate([scene.R_to_angle_axis(R1)[0], t1])]),
                   cam_model=cam_model, cam_model_of_cam=np.array([0, 0 if shared else 1], np.int32),
                   cam_R=np.array([np.eye(3), R1]), cam_t=np.array([np.zeros(3), t1]), cam_c=np.array([np.zeros(3), r["c"][w]]),
                   point=r["X"][b:e].copy(), mse=r["mse"][b:e].copy(), pt_match=r["pt_match"][b:e].copy(), hypotheses=r)
        if keep:
            out["set"] = r["set"]
        if pair_matches is not None:
            if image_keypoints is None:
                if keypoints is None:
                    raise ValueError("pair_matches needs image_keypoints or keypoints")
                kp = np.asarray(keypoints).reshape(-1, 2)
                first = np.concatenate([[0], np.cumsum(store.n_features)])
                image_keypoints = lambda i: kp[first[i]:first[i + 1]]   # noqa: E731
            m = np.asarray(pair_matches(i1, i2), dtype=np.int32).reshape(-1, 2)[out["pt_match"]]
            xy = np.stack([np.asarray(image_keypoints(i1), dtype=np.float64)[m[:, 0]],
                           np.asarray(image_keypoints(i2), dtype=np.float64)[m[:, 1]]], axis=1)    # [P][2][2], camera 0 first
            out.update(obs_cam=np.tile(np.array([0, 1], np.int32), P), obs_pt=np.repeat(np.arange(P, dtype=np.int32), 2),
                       obs_xy=xy.reshape(-1, 2), obs_feature=m.reshape(-1))
        return out
    return None
