"""The second half of a round of IncrementalSfM::Run (sfm_incremental.cc:172-186), Python host side: PartialBundleAdjustment
(:917-1014), every fifth image FullBundleAdjustment (:1016-1026) and RemovePointOutliers (:1831-1863) through one
msfm_round_adjust call on the flat state `newpoints.py` documents (`adjust_round`), the result written back in place
(`apply_round`), and the point side of that state made from a seed result (`point_side_from_seed`)."""
import numpy as np

from . import capi

POINT_SIDE = ("obs_point", "obs_cam", "obs_feat", "pt_mutable")


def point_side_from_seed(seed):
    """The point side of the flat state for the model `seed.find_seed_pair` returns (with its observation arrays): two rows
    per point, camera 0's first - the order FindSeedPairThenReconstruct calls Point3D::AddObservation in - and every point
    mutable (structure.cc:34).  Returns a dict of the four keys to merge into the state."""
    if "obs_feature" not in seed:
        raise ValueError("the seed result has no observation arrays (find_seed_pair needs pair_matches for them)")
    return dict(obs_point=np.asarray(seed["obs_pt"], dtype=np.int32).copy(), obs_cam=np.asarray(seed["obs_cam"], dtype=np.int32).copy(),
                obs_feat=np.asarray(seed["obs_feature"], dtype=np.int32).copy(), pt_mutable=np.ones(len(seed["point"]), np.uint8))


def append_observations(state, point, cam, feat):
    """One row per Point3D::AddObservation, in call order, on a state that has the point side; a state without it is left alone."""
    if "obs_point" not in state:
        return
    for key, rows in (("obs_point", point), ("obs_cam", cam), ("obs_feat", feat)):
        state[key] = np.concatenate([np.asarray(state[key], dtype=np.int32), np.asarray(rows, dtype=np.int32).reshape(-1)])


def adjust_round(ctx: capi.Context, store, state, cam_pose, cam_model, cam_model_of_cam, new_cam, visible, full=False, outliers=True,
                 keypoints=None, **opts):
    """Run :174-186 for the camera `new_cam` just localised, with `visible` = its visible_cams_ (itself first, what
    `localize.apply_localized_image` returns): the partial adjustment, with `full` the full one behind it, with `outliers`
    RemovePointOutliers.  The state needs its point side (obs_point / obs_cam / obs_feat / pt_mutable); cam_pose [n_cams][6]
    (angle-axis, t), cam_model [n_models][3] and cam_model_of_cam are the solver's parameter blocks, which the state does not
    keep.  opts: `partial=False` leaves the partial stage out, the rest are fields of msfm_round_options (`partial_options` /
    `full_options`: dicts of msfm_ba_options fields).  Returns the dict of `Context.round_adjust`."""
    missing = [k for k in POINT_SIDE if k not in state]
    if missing:
        raise KeyError("the state has no point side: %s (adjust.point_side_from_seed makes it from a seed result)" % ", ".join(missing))
    opts = dict(opts)
    partial = opts.pop("partial", True)
    return ctx.round_adjust(store, state["cam_img"], state["feat_point"], state["obs_point"], state["obs_cam"], state["obs_feat"], cam_pose,
                            cam_model, cam_model_of_cam, state["point_xyz"], state["pt_bad"], state["pt_mse"], state["pt_mutable"],
                            pt_new_added=state.get("pt_new_added"), new_cam=new_cam, visible=visible, partial=partial, full=full,
                            outliers=outliers, keypoints=keypoints, **opts)


def apply_round(state, result):
    """BundleAdjuster::UpdateParameters and RemovePointOutliers on the flat state, in place: the point arrays and flags, and
    cam_R / cam_t / cam_c / cam_fk as Camera::UpdatePoseFromData keeps them.  Returns (cam_pose, cam_model) for the next round."""
    for k in ("point_xyz", "pt_bad", "pt_mse", "pt_mutable", "pt_new_added", "cam_R", "cam_t", "cam_c", "cam_fk"):
        state[k] = np.array(result[k])
    return np.array(result["cam_pose"]), np.array(result["cam_model"])
