"""Literal restatements for the start of a model (sfm_incremental.cc:290-374, optimizer.cc:155-232): the two-camera state of a
seed result with Camera::AddPoints as the std::map::insert it is, and BundleAdjuster::Normalize / Perturb on the points as
sequential loops over Python floats (IEEE binary64, one rounding per operation, no fused multiply-add)."""
import numpy as np

from metricsfm_amd import adjust


def state_from_seed(seed, n_features):
    """The flat state (metricsfm_amd/newpoints.py) of the model `seed.find_seed_pair(pair_matches=...)` returns."""
    i1, i2 = seed["images"]
    nf = [int(n_features[i1]), int(n_features[i2])]
    P = len(seed["point"])
    side = adjust.point_side_from_seed(seed)
    pts = [dict(), dict()]                                  # Camera::pts_ of the two cameras
    for row in range(2 * P):
        cam, feat, p = int(side["obs_cam"][row]), int(side["obs_feat"][row]), int(side["obs_point"][row])
        if feat not in pts[cam]:                            # std::map::insert: the first point keeps the feature
            pts[cam][feat] = p
    fp = np.full(nf[0] + nf[1], -1, np.int32)
    for cam, base in ((0, 0), (1, nf[0])):
        for feat, p in pts[cam].items():
            fp[base + feat] = p
    w = seed["hypotheses"]["winner"]
    model, moc = np.asarray(seed["cam_model"], np.float64), np.asarray(seed["cam_model_of_cam"], np.int32)
    fk = np.array([[seed["hypotheses"]["f"][w][c], model[moc[c], 1], model[moc[c], 2]] for c in range(2)])
    return dict(side, cam_img=np.array([i1, i2], np.int32), feat_point=fp, point_xyz=np.array(seed["point"], np.float64),
                pt_bad=np.zeros(P, np.uint8), pt_mse=np.array(seed["mse"], np.float64), pt_views=np.full(P, 2, np.int32),
                pt_new_added=np.ones(P, np.uint8), cam_R=np.array(seed["cam_R"], np.float64), cam_t=np.array(seed["cam_t"], np.float64),
                cam_c=np.array(seed["cam_c"], np.float64), cam_fk=fk, cam_pose=np.array(seed["cam_pose"], np.float64), cam_model=model,
                cam_model_of_cam=moc)


def normalize(point_xyz, noise=None, target_deviation=100.0, point_sigma=0.5):
    """optimizer.cc:157-188 and :204-209, line for line.  Returns (mid [3], scale, points [n][3])."""
    x = [[float(v) for v in row] for row in np.asarray(point_xyz, np.float64).reshape(-1, 3)]
    n = len(x)
    mid = [0.0, 0.0, 0.0]
    for i in range(n):
        mid[0] += x[i][0]
        mid[1] += x[i][1]
        mid[2] += x[i][2]
    mid = [m / n for m in mid]
    mad = 0.0
    for i in range(n):
        mad += abs(x[i][0] - mid[0]) + abs(x[i][1] - mid[1]) + abs(x[i][2] - mid[2])
    mad /= n
    if mad == 0.0:                                          # (Python raises where C++ divides: 100.0 / 0 is inf, nothing is written)
        return np.array(mid), float("inf"), None
    scale = target_deviation / mad
    out = np.zeros((n, 3))
    for i in range(n):
        for k in range(3):
            v = scale * (x[i][k] - mid[k])
            if noise is not None:
                v = v + float(noise[i][k]) * point_sigma
            out[i, k] = v
    return np.array(mid), scale, out


def pairwise_mid(point_xyz):
    """The same mean with a tree-shaped sum (halves, recursively): what a parallel reduction would give."""
    x = np.asarray(point_xyz, np.float64).reshape(-1, 3)

    def tree(v):
        return float(v[0]) if len(v) == 1 else tree(v[:len(v) // 2]) + tree(v[len(v) // 2:])
    return np.array([tree(x[:, k]) / len(x) for k in range(3)])
