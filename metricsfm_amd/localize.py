"""IncrementalSfM::FindImageToLocalize (sfm_incremental.cc:417-563), Python host side: which unregistered images touch the
model (`candidate_images`, :423-438) and, through one msfm_localize_candidates call on a resident match store, their 2D-3D
correspondences and visible cameras in the reference's output order (`find_images_to_localize`, :440-562)."""
import numpy as np

from . import capi

TH_MAX_FAILURE_LOCALIZATION = 5   # basic_structs.h:176


def candidate_images(match_count, processed, fail_times, th_max_failure=TH_MAX_FAILURE_LOCALIZATION):
    """:423-438.  match_count [n][n] = match_graph_; processed [n] = is_img_processed_; fail_times [n] = localize_fail_times_.
    Image j is a candidate when some registered image r has match_count[r, j] > 0 - row r, the direction opposite to the one the
    search reads its matches in (:457, :469 use (j, r)) - and j is neither registered nor failed th_max_failure times.
    Returns the image ids ascending without repeats (math::unique_vector)."""
    match_count = np.asarray(match_count)
    processed = np.asarray(processed, dtype=bool)
    touched = (match_count[processed] > 0).any(axis=0) if processed.any() else np.zeros(len(processed), bool)
    return np.nonzero(touched & ~processed & (np.asarray(fail_times) < th_max_failure))[0].astype(np.int32)


def find_images_to_localize(ctx: capi.Context, store, match_count, cam_img, feat_point, pt_bad, pt_mse, pt_views, fail_times,
                            th_max_failure=TH_MAX_FAILURE_LOCALIZATION, point_xyz=None, keypoints=None, arrays=False):
    """FindImageToLocalize on flat arrays.  cam_img [n_cams] = the image of every camera; feat_point / pt_* / point_xyz /
    keypoints as `Context.localize_candidates` takes them; fail_times [n_images].
    Returns (image_ids, corres_2d3d, visible_cams): the images in the order the loop should try them, per image an int array
    [n][2] of (feature, point) in ascending-mse order, per image the visible camera indices.
    arrays=True adds the library's flat result (corr_off / pts_w / pts_2d ... rows in the same order) as a fourth item:
    with point_xyz it goes to `ctx.epnp_ransac(r["corr_off"], r["pts_w"], r["pts_2d"], f)` as it is."""
    cam_img = np.asarray(cam_img, dtype=np.int32)
    fail_times = np.asarray(fail_times, dtype=np.int32)
    processed = np.zeros(len(fail_times), bool)
    processed[cam_img] = True
    cand = candidate_images(match_count, processed, fail_times, th_max_failure)
    r = ctx.localize_candidates(store, cam_img, feat_point, pt_bad, pt_mse, pt_views, cand, fail_times[cand], point_xyz=point_xyz,
                                keypoints=keypoints)
    co, vo = r["corr_off"], r["vis_off"]
    image_ids = [int(cand[k]) for k in r["rank"]]
    corres = [np.column_stack([r["corr_feat"][co[i]:co[i + 1]], r["corr_point"][co[i]:co[i + 1]]]) for i in range(len(image_ids))]
    visible = [r["vis_cam"][vo[i]:vo[i + 1]].copy() for i in range(len(image_ids))]
    return (image_ids, corres, visible, r) if arrays else (image_ids, corres, visible)
