"""Registering the SLAM model on its GPS track on a resident chain: SLAMGPS::Run between `AbsoluteOrientationWithGPSGlobal`
and the second `GetAccuracy` (SfM/src/slam_gps.cc:98-119), in the reference's order, on the steps of include/msfm.h's
"SLAM + GPS registration" section."""
import numpy as np

from . import capi, scene

TH_OUTLIER = 3.0                      # th_outlier of Triangulation and GetAccuracy (slam_gps.cc:1587)
TH_TRI_ANGLE = 3.0 / 180.0 * np.pi    # th_tri_angle (slam_gps.cc:638)


def set_ac_pose(cam_aa, cam_c):
    """Camera::SetACPose (camera.cc:67-77): the angle-axis vector stays, R from it, t = -R c.  Returns (R [n][9], t, pose [n][6])."""
    aa, c = np.asarray(cam_aa, dtype=np.float64).reshape(-1, 3), np.asarray(cam_c, dtype=np.float64).reshape(-1, 3)
    R = scene.angle_axis_to_R(aa).reshape(-1, 3, 3)
    t = -np.einsum("nij,nj->ni", R, c)
    return R.reshape(-1, 9).copy(), t, np.concatenate([aa, t], axis=1)


def pose_cameras(cam_pose):
    """Camera::UpdatePoseFromData (camera.cc:113-137): R from the angle-axis half of the pose block, t its other half."""
    pose = np.asarray(cam_pose, dtype=np.float64).reshape(-1, 6)
    return scene.angle_axis_to_R(pose[:, :3]).reshape(-1, 9).copy(), pose[:, 3:].copy()


def slam_gps_register(chain, cam_R, cam_c, cam_model, cam_model_of_cam, gps, *, min_views=3, th_outlier=TH_OUTLIER, th_angle=TH_TRI_ANGLE,
                      window=20, clip_deg=80.0, weight_ge3=1.0, gps_weight=0.0, options=None, cam_dc=None):
    """slam_gps.cc:98-119 on a chain whose tracks are built (`chain.build_tracks()`):

        AbsoluteOrientationWithGPSGlobal   capi.gps_orient_global: the cameras (cam_R [n][9], cam_c [n][3], in the model's
                                           own frame) onto `gps` [n][3], everything re-centred on the offset           (:98)
        Triangulation                      chain.triangulate with the transformed cameras, then GetAccuracy:
                                           chain.accuracy                                                    (:108, :638-665)
        GPSRegistration2                   chain.gps_register, then every camera onto its GPS position (SetACPose) (:112)
        FullBundleAdjustment               chain.ba_create with the GPS rows (weight: gps_weight, <= 0 the rule of :824),
                                           run with max_num_iterations = 200 unless `options` says otherwise, and
                                           chain.store_points                                                       (:116)
        GetAccuracy                        chain.accuracy with the adjusted cameras                                 (:119)

    The chain holds only the points made from the matches - the reference's `use_slam_pt_ == false` branch (:659-661), where
    pts_ = pts_new_; the SLAM map points are out of scope.  cam_model [n_models][3] = f, k1, k2; cam_dc [n][2] = dcx, dcy per
    camera, None = 0.  Returns a record: the orientation (scale, err, offset, Rg, tg, weight, gps as shifted), n_accepted,
    the counts of both GetAccuracy calls, the BA summary, gps_weight_used, n_points / n_obs of the problem, the adjusted
    cam_pose / cam_model, and the open BaResident under "ba" (the caller closes it)."""
    cam_model = np.asarray(cam_model, dtype=np.float64).reshape(-1, 3)
    moc = np.asarray(cam_model_of_cam, dtype=np.int32)
    fk = cam_model[moc]
    o = capi.gps_orient_global(cam_R, cam_c, gps, window=window, clip_deg=clip_deg)
    n_accepted = chain.triangulate(o["cam_R"], o["cam_t"], o["cam_c"], fk, th_outlier, th_angle)
    n_out1, n_in1 = chain.accuracy(o["cam_R"], o["cam_t"], fk, cam_dc, min_views, th_outlier)
    chain.gps_register(o["cam_c"], o["gps"])
    _, _, pose = set_ac_pose(o["cam_aa"], o["gps"])
    ba = chain.ba_create(pose, cam_model, moc, min_views=min_views, weight_ge3=weight_ge3, gps_xyz=o["gps"], gps_weight=gps_weight)
    summary = ba.run(options or capi.default_options(max_num_iterations=200))
    chain.store_points(ba)
    pose_adj, model_adj, _ = ba.download()
    R2, t2 = pose_cameras(pose_adj)
    n_out2, n_in2 = chain.accuracy(R2, t2, model_adj[moc], cam_dc, min_views, th_outlier)
    return dict(scale=o["scale"], err=o["err"], offset=o["offset"], Rg=o["Rg"], tg=o["tg"], weight=o["weight"], gps=o["gps"],
                n_accepted=n_accepted, n_outliers=n_out1, n_inliers=n_in1, n_outliers_adjusted=n_out2, n_inliers_adjusted=n_in2,
                summary=summary, gps_weight_used=ba.gps_weight_used, n_points=len(ba.track_of_point), n_obs=ba.n_obs,
                cam_pose=pose_adj, cam_model=model_adj, ba=ba)
