"""The search of IncrementalSfM::FindImageToLocalize (sfm_incremental.cc:440-562) restated as a literal walk with Python
dicts - `dict.setdefault` stands for `std::map::insert` - on the flat arrays msfm_localize_candidates takes.  The yardstick
of tests/test_gpu_localize.py; its own quirks are pinned by tests/test_localize_ref.py.

Where the reference's std::sort leaves the order open this restatement fixes it the way the library documents it: equal mse ->
lower feature first (NaN last), equal score -> lower image id first."""
import math

import numpy as np


def localize_ref(n_features, pairs, match_off, matches, cam_img, feat_point, pt_bad, pt_mse, pt_views, cand_img, fail_times,
                 point_xyz=None, keypoints=None):
    """Returns the dict of `Context.localize_candidates` (without h2d_bytes): rank, corr_off, corr_feat, corr_point, vis_off,
    vis_cam [, pts_w, pts_2d]; row r of the CSR arrays belongs to candidate rank[r]."""
    n_features = [int(x) for x in n_features]
    n_images = len(n_features)
    pair_at = {(int(a), int(b)): p for p, (a, b) in enumerate(np.asarray(pairs).reshape(-1, 2))}
    cam_of, fp_start, at = {}, [], 0
    for c, im in enumerate(cam_img):            # img_cam_map_; camera c's slice of feat_point
        cam_of[int(im)] = c
        fp_start.append(at)
        at += n_features[int(im)]
    per_cand = []
    for i in (int(x) for x in cand_img):
        corres, info, visible = {}, {}, []
        for j in range(n_images):                                        # :452
            if j not in cam_of or (i, j) not in pair_at:                 # :457-464
                continue
            p = pair_at[(i, j)]
            if match_off[p + 1] == match_off[p]:                         # :470-474
                continue
            cam, count = cam_of[j], 0
            for m in range(int(match_off[p]), int(match_off[p + 1])):    # :480
                f_i, f_j = int(matches[m][0]), int(matches[m][1])
                pt = int(feat_point[fp_start[cam] + f_j])
                if pt >= 0 and not pt_bad[pt]:                           # :486-487
                    corres.setdefault(f_i, pt)                           # :489
                    info.setdefault(f_i, float(pt_mse[pt]) + (3.0 if pt_views[pt] <= 2 else 0.0))   # :491-496
                    count += 1                                           # :497
            if count > 5:                                                # :503
                visible.append(cam)
        order = sorted(info, key=lambda f: (math.isnan(info[f]), 0.0 if math.isnan(info[f]) else info[f], f))   # :524
        per_cand.append(([(f, corres[f]) for f in order], visible))
    score = [len(per_cand[k][0]) // (5 + int(fail_times[k])) for k in range(len(per_cand))]   # :543
    rank = sorted((k for k in range(len(per_cand)) if score[k] > 0), key=lambda k: (-score[k], k))   # :545, :552
    out = dict(rank=np.array(rank, np.int32), corr_off=[0], corr_feat=[], corr_point=[], vis_off=[0], vis_cam=[])
    for k in rank:
        out["corr_feat"] += [f for f, _ in per_cand[k][0]]
        out["corr_point"] += [p for _, p in per_cand[k][0]]
        out["corr_off"].append(len(out["corr_feat"]))
        out["vis_cam"] += per_cand[k][1]
        out["vis_off"].append(len(out["vis_cam"]))
    out = {k: np.asarray(v, np.int32) for k, v in out.items()}
    if point_xyz is not None:                                            # :592-600
        feat_start = np.concatenate([[0], np.cumsum(n_features)])
        row = np.concatenate([feat_start[int(cand_img[k])] + out["corr_feat"][out["corr_off"][r]:out["corr_off"][r + 1]]
                              for r, k in enumerate(rank)] + [np.zeros(0, np.int64)]).astype(np.int64)
        out["pts_w"] = np.asarray(point_xyz, np.float64).reshape(-1, 3)[out["corr_point"]]
        out["pts_2d"] = np.asarray(keypoints, np.float32).reshape(-1, 2)[row].astype(np.float64)
    return out
