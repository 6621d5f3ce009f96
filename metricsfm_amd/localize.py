"""IncrementalSfM::FindImageToLocalize (sfm_incremental.cc:417-563), Python host side: which unregistered images touch the
model (`candidate_images`, :423-438) and, through one msfm_localize_candidates call on a resident match store, their 2D-3D
correspondences and visible cameras in the reference's output order (`find_images_to_localize`, :440-562); the tries of
Run :143-164 around LocalizeImage (:565-753) through one msfm_localize_poses call per chunk on the set that search leaves on the
device (`localize_next_image`), and LocalizeImage's state changes on the flat state (`apply_localized_image`)."""
import numpy as np

from . import adjust, capi

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


def localize_next_image(ctx: capi.Context, store, state, match_count, fail_times, image_f, image_f_init, keypoints=None,
                        th_max_failure=TH_MAX_FAILURE_LOCALIZATION, **opts):
    """One pass of IncrementalSfM::Run :126-164 on the flat state `newpoints.py` documents (plus the optional pt_new_added
    [n_points], is_new_added_): FindImageToLocalize, then the tries of :146-159 through msfm_localize_poses on the resident
    correspondence set, in chunks of max_tries rows (first_row / next_row) until a row passes or the rows run out.
    image_f [n_images] = the focal length a new camera of that image would start with (0.0 = unknown: the sweep around
    image_f_init [n_images], sfm_incremental.cc:675).  opts: fields of msfm_localize_pose_options.
    Returns a dict: image (-1: no image localised), row, image_ids (the ranked candidates), failed_images (the tried rows ahead
    of the winner - all tried rows without one -, whose localize_fail_times_ the reference increments, :650 / :681), n_calls and,
    with a winner, f, R, t, avg_error, n_inliers, corr_feat / corr_point / corr_state / errors of its row, visible (its
    visible_cams).  `fail_times` is not written."""
    cam_img = np.asarray(state["cam_img"], dtype=np.int32)
    fail_times = np.asarray(fail_times, dtype=np.int32)
    n_points = len(state["pt_mse"])
    processed = np.zeros(len(fail_times), bool)
    processed[cam_img] = True
    cand = candidate_images(match_count, processed, fail_times, th_max_failure)
    out = dict(image=-1, row=-1, image_ids=[], failed_images=[], n_calls=0)
    st = ctx.localize_set(store, cam_img, state["feat_point"], state["pt_bad"], state["pt_mse"], state["pt_views"], cand, fail_times[cand],
                          point_xyz=state["point_xyz"], keypoints=keypoints)
    try:
        loc = st.fetch()
        ids = cand[loc["rank"]] if len(loc["rank"]) else np.zeros(0, np.int32)
        out["image_ids"] = [int(i) for i in ids]
        row_f = np.asarray(image_f, dtype=np.float64)[ids]
        row_fi = np.asarray(image_f_init, dtype=np.float64)[ids]
        opts = dict(opts)
        row = int(opts.pop("first_row", 0))
        while row >= 0 and len(ids):
            r = st.poses(row_f, row_f_init=row_fi, n_points=n_points, pt_new_added=state.get("pt_new_added"), first_row=row, **opts)
            out["n_calls"] += 1
            tried = np.nonzero(r["tried"])[0]
            w = r["winner"]
            out["failed_images"] += [int(ids[k]) for k in tried if w < 0 or k < w]
            if w >= 0:
                b, e = loc["corr_off"][w], loc["corr_off"][w + 1]
                vb, ve = loc["vis_off"][w], loc["vis_off"][w + 1]
                out.update(image=int(ids[w]), row=int(w), f=float(r["f"][w]), R=r["R"][w].copy(), t=r["t"][w].copy(),
                           avg_error=float(r["avg_error"][w]), n_inliers=int(r["n_inliers"][w]), corr_feat=loc["corr_feat"][b:e].copy(),
                           corr_point=loc["corr_point"][b:e].copy(), corr_state=r["corr_state"][b:e].copy(), errors=r["errors"][b:e].copy(),
                           visible=loc["vis_cam"][vb:ve].copy())
                break
            row = r["next_row"]
    finally:
        st.close()
    return out


def apply_localized_image(state, result, k1=0.0, k2=0.0):
    """LocalizeImage :705-748 on the flat state, in place, for a `localize_next_image` result with a winner: the camera is
    appended (cam_img; a feat_point row of -1 with the state-2 features set, Camera::AddPoints :725; cam_R, cam_t, cam_c = -R^T t
    as SetRTPose keeps it; cam_fk = (f, k1, k2)), the state-1 points become bad (:715), the state-2 points gain a view and
    is_new_added_ (:723-724; pt_new_added is created when the state has none).  Returns the new camera's visible list as
    UpdateVisibleGraph (:1895-1903) builds it: itself, then the visible cameras - what `newpoints.generate_new_points` takes.
    A state with the point side (obs_point / obs_cam / obs_feat, `newpoints.py`) gets one row per state-2 correspondence, in
    correspondence order (Point3D::AddObservation, :723)."""
    if result["image"] < 0:
        raise ValueError("no image was localised")
    im = int(result["image"])
    nf = int(np.asarray(state["n_features"])[im])
    st = np.asarray(result["corr_state"])
    feat, pt = np.asarray(result["corr_feat"], dtype=np.int64), np.asarray(result["corr_point"], dtype=np.int64)
    row = np.full(nf, -1, np.int32)
    row[feat[st == 2]] = pt[st == 2]
    new_cam = len(state["cam_img"])
    R, t = np.asarray(result["R"], dtype=np.float64).reshape(3, 3), np.asarray(result["t"], dtype=np.float64).reshape(3)
    state["cam_img"] = np.concatenate([np.asarray(state["cam_img"], dtype=np.int32), [im]]).astype(np.int32)
    state["feat_point"] = np.concatenate([np.asarray(state["feat_point"], dtype=np.int32), row])
    state["cam_R"] = np.concatenate([np.asarray(state["cam_R"], dtype=np.float64).reshape(-1, 3, 3), R[None]])
    state["cam_t"] = np.concatenate([np.asarray(state["cam_t"], dtype=np.float64).reshape(-1, 3), t[None]])
    c = -((R[0] * t[0] + R[1] * t[1]) + R[2] * t[2])   # Camera::SetRTPose: -(R^T t), the products summed in row order
    state["cam_c"] = np.concatenate([np.asarray(state["cam_c"], dtype=np.float64).reshape(-1, 3), c[None]])
    state["cam_fk"] = np.concatenate([np.asarray(state["cam_fk"], dtype=np.float64).reshape(-1, 3), [[result["f"], k1, k2]]])
    bad = np.array(state["pt_bad"], dtype=np.uint8)
    bad[pt[st == 1]] = 1
    state["pt_bad"] = bad
    views = np.array(state["pt_views"], dtype=np.int32)
    views[pt[st == 2]] += 1
    state["pt_views"] = views
    added = np.array(state["pt_new_added"], dtype=np.uint8) if "pt_new_added" in state else np.zeros(len(bad), np.uint8)
    added[pt[st == 2]] = 1
    state["pt_new_added"] = added
    adjust.append_observations(state, pt[st == 2], np.full(int((st == 2).sum()), new_cam, np.int32), feat[st == 2])
    return [new_cam] + [int(c) for c in result["visible"]]
