"""A literal walk of what msfm_round_adjust keeps of the reference (include/msfm.h), on dicts in the place of the std::maps:
  Point3D::AddObservation                     structure.cc:132-140    cams_ / pts2d_ keyed by (image, feature), insert keeps the first
  ImmutableCamsPoints / MutableCamsPoints     sfm_incremental.cc:1865-1893
  PartialBundleAdjustment's masks             :919-945
  BundleAdjuster::RunOptimizetion's gather    optimizer.cc:59-129, compact as window.gather(compact=True) defines it
  Point3D::Reprojection / RemovePointOutliers structure.cc:267-300 / sfm_incremental.cc:1831-1863
The cameras of the outlier walk (cam_R, cam_t, cam_fk) are inputs.  Every sum is formed in numpy float64 scalars, one operation
at a time: + - * / sqrt in doubles, nothing fused."""
import numpy as np


def feature_offsets(case):
    nf = np.asarray(case["n_features"], dtype=np.int64)
    return np.concatenate([[0], np.cumsum(nf)]), np.concatenate([[0], np.cumsum(nf[np.asarray(case["cam_img"], dtype=np.int64)])])


def camera_side(case):
    """Camera::pts_ of every camera: {feature: point}."""
    _, cam_fo = feature_offsets(case)
    fp = np.asarray(case["feat_point"])
    return [{f: int(p) for f, p in enumerate(fp[cam_fo[c]:cam_fo[c + 1]]) if p >= 0} for c in range(len(case["cam_img"]))]


def point_side(case):
    """Point3D::cams_ of every point: {(image, feature): (camera, feature)}, std::map::insert - the first row of a key stays."""
    cams = [dict() for _ in range(len(case["pt_bad"]))]
    img = np.asarray(case["cam_img"])
    for p, c, f in zip(case["obs_point"], case["obs_cam"], case["obs_feat"]):
        cams[int(p)].setdefault((int(img[c]), int(f)), (int(c), int(f)))
    return cams


def views(case):
    return np.array([len(m) for m in point_side(case)], np.int32)


def free_cameras(case, new_cam, visible):
    """The cameras PartialBundleAdjustment(new_cam) frees: those of its model (:922-925), then its visible ones (:934-937)."""
    moc = np.asarray(case["cam_model_of_cam"])
    free = [int(c) for c in range(len(moc)) if moc[c] == moc[new_cam]]
    return free + [int(c) for c in visible]


def masks(case, stage, new_cam=-1, visible=(), pt_mutable=None):
    """(cam_mutable, pt_mutable) after the mask loops of stage "partial" or "full", starting from pt_mutable (default: the case's)."""
    pts_ = camera_side(case)
    nc = len(pts_)
    mut = [int(v) for v in (case["pt_mutable"] if pt_mutable is None else pt_mutable)]
    bad = np.asarray(case["pt_bad"])
    if stage == "partial":
        cam_mut = [0] * nc
        for c in range(nc):                          # ImmutableCamsPoints
            for p in pts_[c].values():
                mut[p] = 0
        for c in free_cameras(case, new_cam, visible):
            cam_mut[c] = 1
            for p in pts_[c].values():
                if not bad[p]:
                    mut[p] = 1
    else:
        cam_mut = [1] * nc                           # MutableCamsPoints
        for c in range(nc):
            for p in pts_[c].values():
                mut[p] = 1
    return np.array(cam_mut, np.uint8), np.array(mut, np.uint8)


def keypoint(case, image, feature):
    feat_off, _ = feature_offsets(case)
    return np.asarray(case["keypoints"], dtype=np.float32).reshape(-1, 2)[feat_off[image] + feature].astype(np.float64)


def gather(case, cam_mut, pt_mut, weight, point_xyz=None):
    """The compact problem of one solve."""
    cams_ = point_side(case)
    xyz = np.asarray(case["point_xyz"] if point_xyz is None else point_xyz, dtype=np.float64).reshape(-1, 3)
    kept, obs_cam, obs_pt, obs_xy, w = [], [], [], [], []
    for p in range(len(cams_)):
        if case["pt_bad"][p]:
            continue
        rows = [(c, f, image) for (image, _), (c, f) in sorted(cams_[p].items()) if cam_mut[c] or pt_mut[p]]
        if not rows:
            continue
        for c, f, image in rows:
            obs_cam.append(c)
            obs_pt.append(len(kept))
            obs_xy.append(keypoint(case, image, f))
        n = len(cams_[p])
        w.append(1.0 if n == 2 else (weight if n >= 3 else 1.0))
        kept.append(p)
    kept = np.array(kept, np.int32)
    return dict(kept=kept, obs_cam=np.array(obs_cam, np.int32), obs_pt=np.array(obs_pt, np.int32), obs_xy=np.array(obs_xy, np.float64).reshape(-1, 2),
                pt_weight=np.array(w, np.float64), cam_mutable=np.asarray(cam_mut, np.uint8), pt_mutable=np.asarray(pt_mut, np.uint8)[kept],
                point=xyz[kept].copy())


def reprojection(case, cams_p, X, cam_R, cam_t, cam_fk):
    """Point3D::Reprojection of one point: its mse."""
    f8 = np.float64
    X = [f8(v) for v in X]
    mse, count = f8(0.0), 0
    for (image, _), (c, f) in sorted(cams_p.items()):
        R, t, fk = np.asarray(cam_R[c], f8).reshape(9), np.asarray(cam_t[c], f8), np.asarray(cam_fk[c], f8)
        pc = [R[3 * r] * X[0] + R[3 * r + 1] * X[1] + R[3 * r + 2] * X[2] + t[r] for r in range(3)]
        if pc[2] < 0:
            return f8(100000.0)
        x, y = pc[0] / pc[2], pc[1] / pc[2]
        r2 = x * x + y * y
        distortion = f8(1.0) + r2 * (fk[1] + fk[2] * r2)
        u, v = fk[0] * distortion * x, fk[0] * distortion * y
        kp = keypoint(case, image, f)
        du, dv = u - kp[0], v - kp[1]
        mse = mse + (du * du + dv * dv)
        count += 1
    return mse / f8(count)


def remove_outliers(case, cam_R, cam_t, cam_fk, th=1.0, point_xyz=None, pt_bad=None):
    """RemovePointOutliers.  Returns pt_mse, pt_bad, pt_new_added and the three counts."""
    cams_ = point_side(case)
    xyz = np.asarray(case["point_xyz"] if point_xyz is None else point_xyz, dtype=np.float64).reshape(-1, 3)
    bad = np.array(case["pt_bad"] if pt_bad is None else pt_bad, np.uint8)
    mse = np.array(case["pt_mse"], np.float64)
    added = np.array(case["pt_new_added"], np.uint8) if case.get("pt_new_added") is not None else np.zeros(len(bad), np.uint8)
    count_outliers = count_new_add = count_outliers_new_add = 0
    with np.errstate(all="ignore"):
        for p in range(len(bad)):
            if bad[p]:
                continue
            if added[p]:
                count_new_add += 1
            mse[p] = reprojection(case, cams_[p], xyz[p], cam_R, cam_t, cam_fk)
            if np.sqrt(mse[p]) > th:
                bad[p] = 1
                count_outliers += 1
                if added[p]:
                    count_outliers_new_add += 1
            added[p] = 0
    return dict(pt_mse=mse, pt_bad=bad, pt_new_added=added, count_outliers=count_outliers, count_new_add=count_new_add,
                count_outliers_new_add=count_outliers_new_add)
