"""IncrementalSfM::GenerateNew3DPoints (sfm_incremental.cc:755-915), Python host side: the new two-view points of a localised
camera through one msfm_new_points call on a resident match store (`generate_new_points`), and their insertion into the flat
state the next round reads (`apply_new_points`, :899-910).

The flat state is a dict in the layout `localize.find_images_to_localize` and `window.partial_bundle_adjustment_problem` read:
  n_features [n_images]; cam_img [n_cams]; feat_point (camera c starts at the sum of n_features[cam_img[c']] over c' < c;
  local feature -> point id or -1); cam_R [n_cams][3][3], cam_t, cam_c, cam_fk [n_cams][3]; point_xyz [n_points][3], pt_bad,
  pt_mse, pt_views [n_points].
Optional keys, the point side (the state above keeps only the camera side, Camera::pts_; `adjust.adjust_round` needs both):
  obs_point, obs_cam, obs_feat [n_obs] int32: Point3D::cams_ / pts2d_, one row per Point3D::AddObservation in call order -
  point id, camera index, local feature.  The two sides differ wherever a Camera::AddPoints insert did not take (takes1 /
  takes2 below): the observation exists, the feat_point entry belongs to an earlier point.
  pt_mutable [n_points] uint8: Point3D::is_mutable_, 1 for a new point (structure.cc:34).
`adjust.point_side_from_seed` makes them from a seed result; `apply_new_points` and `localize.apply_localized_image` keep them up
to date when the state has them, and behave as before when it has not.  pt_new_added [n_points] (is_new_added_) is optional too."""
from collections import namedtuple

import numpy as np

from . import adjust, capi

NewPoints = namedtuple("NewPoints", "X mse cam2 feat1 feat2 takes1 takes2")


def generate_new_points(ctx: capi.Context, store, state, new_cam, visible, keypoints=None, **opts):
    """:755-897 for camera `new_cam` with the visible cameras `visible` (its visible_cams_, in that order).  Returns what
    `tracks.generate_new_points` returns - X [n][3], mse [n], cam2, feat1, feat2 [n] in the order the reference appends the
    points to pts_ - plus takes1 / takes2 [n]: whether Camera::AddPoints of the new camera / of cam2 took the point (:908-909).
    opts: fields of msfm_new_points_options."""
    visible = np.asarray(visible, dtype=np.int32).reshape(-1)
    r = ctx.new_points(store, state["cam_img"], state["feat_point"], len(state["pt_mse"]), state["cam_R"], state["cam_t"], state["cam_c"],
                       state["cam_fk"], [new_cam], [0, len(visible)], visible, keypoints=keypoints, **opts)
    return NewPoints(r["X"], r["mse"], r["cam2"], r["feat1"], r["feat2"], r["takes1"], r["takes2"])


def apply_new_points(state, result, new_cam=None):
    """:899-910 on the flat state, in place: every point is appended (id = its position behind the existing ones, two views,
    its mse, not bad), and feat_point gets the inserts that took.  new_cam: the camera the points were generated for (default:
    the newest one, cams_.size() - 1 as in the reference).  Returns the ids of the new points."""
    r = NewPoints(*result)
    cam_img = np.asarray(state["cam_img"], dtype=np.int64)
    c1 = len(cam_img) - 1 if new_cam is None else int(new_cam)
    cam_fo = np.concatenate([[0], np.cumsum(np.asarray(state["n_features"], dtype=np.int64)[cam_img])])
    n0, n = len(state["pt_mse"]), len(r.mse)
    ids = np.arange(n0, n0 + n, dtype=np.int32)
    fp = np.array(state["feat_point"], dtype=np.int32)
    t1, t2 = np.asarray(r.takes1, dtype=bool), np.asarray(r.takes2, dtype=bool)
    fp[cam_fo[c1] + np.asarray(r.feat1, dtype=np.int64)[t1]] = ids[t1]
    fp[cam_fo[np.asarray(r.cam2, dtype=np.int64)[t2]] + np.asarray(r.feat2, dtype=np.int64)[t2]] = ids[t2]
    state["feat_point"] = fp
    state["point_xyz"] = np.concatenate([np.asarray(state["point_xyz"], dtype=np.float64).reshape(-1, 3), np.asarray(r.X).reshape(-1, 3)])
    state["pt_mse"] = np.concatenate([np.asarray(state["pt_mse"], dtype=np.float64), r.mse])
    state["pt_views"] = np.concatenate([np.asarray(state["pt_views"], dtype=np.int32), np.full(n, 2, np.int32)])
    state["pt_bad"] = np.concatenate([np.asarray(state["pt_bad"], dtype=np.uint8), np.zeros(n, np.uint8)])
    if "obs_point" in state:   # Point3D::AddObservation of both views (:810-821), whether or not the camera-side inserts took
        adjust.append_observations(state, np.repeat(ids, 2), np.column_stack([np.full(n, c1, np.int32), r.cam2]), np.column_stack([r.feat1, r.feat2]))
    if "pt_new_added" in state:   # is_new_added_ = true, :819
        state["pt_new_added"] = np.concatenate([np.asarray(state["pt_new_added"], dtype=np.uint8), np.ones(n, np.uint8)])
    if "pt_mutable" in state:
        state["pt_mutable"] = np.concatenate([np.asarray(state["pt_mutable"], dtype=np.uint8), np.ones(n, np.uint8)])
    return ids
