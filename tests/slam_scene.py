"""A small aerial scene whose observations serve as the SLAM points of SLAMGPS::FeatureMatching step 1, with planted cases
so that every verdict of msfm_slam_priors occurs: a planar block (flat ground under cameras 0-2: the homography explains
the pairs among them as well as F -> H gate), a camera that sees few points (camera 15: < 20 shared -> skipped) and a
camera whose observations are mostly outliers (camera 7 -> F gate)."""
import numpy as np

from metricsfm_amd import scene


def planted_scene(n_cams=16, n_points=3000, seed=41):
    sc = scene.make_aerial_scene(n_cams, n_points, seed=seed)
    rng = np.random.default_rng(seed)
    # planar block: points on the ground z = 0 wherever the first cameras look
    flat = sc.point_gt[:, 1] < 45.0
    sc.point_gt[flat, 2] = 0.0
    R = scene.angle_axis_to_R(sc.cam_pose_gt[:, :3])
    o = np.nonzero(flat[sc.obs_pt])[0]
    uv, _ = scene.project_Rt(R[sc.obs_cam[o]], sc.cam_pose_gt[sc.obs_cam[o], 3:], sc.cam_model_gt[sc.cam_model_of_cam[sc.obs_cam[o]]],
                             sc.point_gt[sc.obs_pt[o]])
    sc.obs_xy[o] = uv + rng.standard_normal(uv.shape) * 0.5
    # camera 7: 70 % of its observations replaced by random positions
    o7 = np.nonzero(sc.obs_cam == 7)[0]
    bad = rng.choice(o7, int(0.7 * len(o7)), replace=False)
    sc.obs_xy[bad] = np.column_stack([rng.uniform(-scene.IMG_W / 2, scene.IMG_W / 2, len(bad)),
                                      rng.uniform(-scene.IMG_H / 2, scene.IMG_H / 2, len(bad))])
    # camera 15: only its first 12 points stay
    o15 = np.nonzero(sc.obs_cam == n_cams - 1)[0]
    keep = np.ones(sc.n_obs, bool)
    keep[o15[12:]] = False
    sc.obs_cam, sc.obs_pt, sc.obs_xy = sc.obs_cam[keep], sc.obs_pt[keep], sc.obs_xy[keep]
    toff = sc.track_offsets()
    return sc, toff, sc.obs_cam.copy(), sc.obs_xy.copy()
