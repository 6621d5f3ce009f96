"""The rounds of IncrementalSfM::Run (sfm_incremental.cc:126-186) behind the seed pair, driven through either of two backends:
`FlatBackend` - the flat state dict of `newpoints.py` with `localize.localize_next_image` / `apply_localized_image`,
`newpoints.generate_new_points` / `apply_new_points`, `adjust.adjust_round` / `apply_round` as they stand - and `ResidentBackend`
- a `capi.Recon`, whose state stays on the device: localize, commit_camera, new_points, adjust.  What is host knowledge in both
lives here once, so that both backends are fed identical values: the candidate list and the `fail_times` bookkeeping (:650 /
:681), the winner's rotation as an angle-axis block (`scene.R_to_angle_axis`, SetRTPose), the image-to-model map, and the full
adjustment on every fifth camera (:176-181)."""
import numpy as np

from . import adjust, localize, newpoints, scene


class Book:
    """The host-side bookkeeping of a model: match_count [n][n], fail_times [n] (written by `run_round`), image_f / image_f_init
    [n] (image_f 0.0: unknown, the sweep), image_model [n] (the camera model a new camera of that image joins; -1: one of its
    own, (f, 0, 0)), and the option dicts of the three calls."""

    def __init__(self, match_count, image_f, image_f_init, image_model=None, fail_times=None, localize_opts=None, new_points_opts=None, round_opts=None):
        n = len(image_f)
        self.match_count = np.asarray(match_count)
        self.image_f, self.image_f_init = np.asarray(image_f, np.float64), np.asarray(image_f_init, np.float64)
        self.image_model = np.full(n, -1, np.int32) if image_model is None else np.array(image_model, np.int32)
        self.fail_times = np.zeros(n, np.int32) if fail_times is None else np.array(fail_times, np.int32)
        self.localize_opts, self.new_points_opts, self.round_opts = dict(localize_opts or {}), dict(new_points_opts or {}), dict(round_opts or {})


class FlatBackend:
    def __init__(self, ctx, store, state, cam_pose, cam_model, cam_model_of_cam, keypoints=None):
        self.ctx, self.store, self.keypoints = ctx, store, keypoints
        self.state = {k: np.array(v) for k, v in state.items()}
        self.cam_pose, self.cam_model = np.array(cam_pose, np.float64).reshape(-1, 6), np.array(cam_model, np.float64).reshape(-1, 3)
        self.cam_model_of_cam = np.array(cam_model_of_cam, np.int32)

    def cam_img(self):
        return np.asarray(self.state["cam_img"], np.int32)

    def localize(self, book, cand):
        self._loc = localize.localize_next_image(self.ctx, self.store, self.state, book.match_count, book.fail_times, book.image_f, book.image_f_init,
                                                 keypoints=self.keypoints, **book.localize_opts)
        return self._loc

    def commit_camera(self, pose6, model, cam_model3):
        if model == len(self.cam_model):
            self.cam_model = np.concatenate([self.cam_model, np.asarray(cam_model3, np.float64)[None]])
        k1, k2 = self.cam_model[model, 1:]
        visible = localize.apply_localized_image(self.state, self._loc, k1=k1, k2=k2)
        self.cam_pose = np.concatenate([self.cam_pose, np.asarray(pose6, np.float64)[None]])
        self.cam_model_of_cam = np.concatenate([self.cam_model_of_cam, [model]]).astype(np.int32)
        return visible

    def new_points(self, book, new_cam, visible):
        r = newpoints.generate_new_points(self.ctx, self.store, self.state, new_cam, visible, keypoints=self.keypoints, **book.new_points_opts)
        newpoints.apply_new_points(self.state, r, new_cam)
        self.last_new_points = r          # (takes1 / takes2: which inserts took)
        return len(r.mse)

    def adjust(self, book, new_cam, visible, full):
        r = adjust.adjust_round(self.ctx, self.store, self.state, self.cam_pose, self.cam_model, self.cam_model_of_cam, new_cam, visible,
                                full=full, keypoints=self.keypoints, **book.round_opts)
        self.cam_pose, self.cam_model = adjust.apply_round(self.state, r)
        return r

    def fetch(self):
        return dict(self.state, cam_pose=self.cam_pose, cam_model=self.cam_model, cam_model_of_cam=self.cam_model_of_cam)

    def n_models(self):
        return len(self.cam_model)


class ResidentBackend:
    def __init__(self, ctx, store, state, cam_pose, cam_model, cam_model_of_cam, keypoints=None, **reserve):
        self.recon = ctx.recon(store, state, cam_pose, cam_model, cam_model_of_cam, keypoints=keypoints, **reserve)
        self._cam_img = [int(i) for i in np.asarray(state["cam_img"]).reshape(-1)]

    def cam_img(self):
        return np.array(self._cam_img, np.int32)

    def localize(self, book, cand):
        self._loc = self.recon.localize(cand, book.fail_times[cand], book.image_f[cand], book.image_f_init[cand], **book.localize_opts)
        return self._loc

    def commit_camera(self, pose6, model, cam_model3):
        visible = self.recon.commit_camera(pose6, model, cam_model3)
        self._cam_img.append(self._loc["image"])
        return visible

    def new_points(self, book, new_cam, visible):
        return self.recon.new_points(new_cam, visible, **book.new_points_opts)

    def adjust(self, book, new_cam, visible, full):
        return self.recon.adjust(new_cam, visible, full=full, **book.round_opts)

    def fetch(self):
        return self.recon.fetch()

    def n_models(self):
        return self.recon.size()["n_models"]

    def close(self):
        self.recon.close()


def run_round(backend, book):
    """One pass of :126-186.  Returns the round's record: image (-1: none localised, nothing else ran), f, R, t, avg_error,
    failed_images, visible, n_new, count_outliers / count_new_add / count_outliers_new_add, solved, summary, full."""
    cam_img = backend.cam_img()
    processed = np.zeros(len(book.fail_times), bool)
    processed[cam_img] = True
    cand = localize.candidate_images(book.match_count, processed, book.fail_times)
    loc = backend.localize(book, cand)
    for im in loc["failed_images"]:
        book.fail_times[im] += 1                  # :650 / :681
    rec = dict(image=loc["image"], failed_images=list(loc["failed_images"]), image_ids=list(loc["image_ids"]))
    if loc["image"] < 0:
        return rec
    im = loc["image"]
    pose6 = np.concatenate([scene.R_to_angle_axis(loc["R"]).reshape(3), np.asarray(loc["t"], np.float64).reshape(3)])   # SetRTPose
    model = int(book.image_model[im])
    cam_model3 = None
    if model < 0 or model >= backend.n_models():
        model, cam_model3 = backend.n_models(), np.array([loc["f"], 0.0, 0.0])
        book.image_model[im] = model
    visible = backend.commit_camera(pose6, model, cam_model3)
    new_cam = visible[0]
    n_new = backend.new_points(book, new_cam, visible)
    full = (len(cam_img) + 1) % 5 == 0            # :176-181: every fifth camera
    r = backend.adjust(book, new_cam, visible, full)
    rec.update(f=loc["f"], R=np.array(loc["R"]), t=np.array(loc["t"]), avg_error=loc["avg_error"], n_inliers=loc["n_inliers"], visible=[int(v) for v in visible],
               n_new=int(n_new), full=bool(full), solved=np.array(r["solved"]), summary=r["summary"],
               **{k: r[k] for k in ("count_outliers", "count_new_add", "count_outliers_new_add")})
    return rec


def run_rounds(backend, book, n_rounds):
    return [run_round(backend, book) for _ in range(n_rounds)]
