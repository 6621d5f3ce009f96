"""The rounds of IncrementalSfM::Run (sfm_incremental.cc:126-186) behind the seed pair, driven through either of two backends:
`FlatBackend` - the flat state dict of `newpoints.py` with `localize.localize_next_image` / `apply_localized_image`,
`newpoints.generate_new_points` / `apply_new_points`, `adjust.adjust_round` / `apply_round` as they stand - and `ResidentBackend`
- a `capi.Recon`, whose state stays on the device: localize, commit_camera, new_points, adjust.  What is host knowledge in both
lives here once, so that both backends are fed identical values: the candidate list and the `fail_times` bookkeeping (:650 /
:681), the winner's rotation as an angle-axis block (`scene.R_to_angle_axis`, SetRTPose), the image-to-model map, and the full
adjustment on every fifth camera (:176-181).

`start_model` is the rest of FindSeedPairThenReconstruct behind its gates (:290-410) - the two-camera state of the winning
pair, BundleAdjuster::Normalize and Perturb (optimizer.cc:155-232), the initial full adjustment and the outlier stage - and
`reconstruct` the outer loop of Run (:99-220): one model after another on the images that are still unprocessed."""
import numpy as np

from . import _abi as A
from . import adjust, capi, localize, newpoints, scene
from . import seed as seedpair

ROTATION_SIGMA, TRANSLATION_SIGMA = 0.1, 0.5     # optimizer.cc:199-200 (point_sigma is msfm_recon_normalize's argument)


class Book:
    """The host-side bookkeeping of a model: match_count [n][n], fail_times [n] (written by `run_round`), image_f / image_f_init
    [n] (image_f 0.0: unknown, the sweep), image_model [n] (the camera model a new camera of that image joins; -1: one of its
    own, (f, 0, 0)), processed [n] (is_img_processed_: images of this and of earlier models; default all false), image_group [n]
    (CameraAssociateCameraModel: images with equal ids share a camera model when a model is started from them; default every
    image its own), and the option dicts of the calls."""

    def __init__(self, match_count, image_f, image_f_init, image_model=None, fail_times=None, localize_opts=None, new_points_opts=None, round_opts=None,
                 processed=None, image_group=None, seed_opts=None):
        n = len(image_f)
        self.match_count = np.asarray(match_count)
        self.image_f, self.image_f_init = np.asarray(image_f, np.float64), np.asarray(image_f_init, np.float64)
        self.image_model = np.full(n, -1, np.int32) if image_model is None else np.array(image_model, np.int32)
        self.fail_times = np.zeros(n, np.int32) if fail_times is None else np.array(fail_times, np.int32)
        self.localize_opts, self.new_points_opts, self.round_opts = dict(localize_opts or {}), dict(new_points_opts or {}), dict(round_opts or {})
        self.processed = np.zeros(n, bool) if processed is None else np.array(processed, bool)
        self.image_group = np.arange(n) if image_group is None else np.array(image_group)
        self.seed_opts = dict(seed_opts or {})


def state_from_seed(seed, n_features):
    """The flat state of the two-camera model `seed.find_seed_pair` returns with its observation arrays (:290-374): camera 0
    is [I|0], camera 1 the winning pose, cam_fk = (the hypothesis' f, the model's k1, k2); every point has two views and is
    new and mutable (structure.cc:30-37); Camera::AddPoints is a std::map::insert, so a feature that occurs in two accepted
    matches belongs to the first point while both points keep both rows."""
    side = adjust.point_side_from_seed(seed)
    i1, i2 = seed["images"]
    n_features = np.asarray(n_features, np.int32)
    nf1, P = int(n_features[i1]), len(seed["point"])
    fp = np.full(nf1 + int(n_features[i2]), -1, np.int32)
    feat = side["obs_feat"].reshape(-1, 2)
    for c, base in ((0, 0), (1, nf1)):
        u, first = np.unique(feat[:, c], return_index=True)     # the first point of a feature keeps it
        fp[base + u] = first
    w = seed["hypotheses"]["winner"]
    moc = np.asarray(seed["cam_model_of_cam"], np.int32)
    fk = np.column_stack([seed["hypotheses"]["f"][w], np.asarray(seed["cam_model"], np.float64)[moc, 1:]])
    return dict(side, n_features=n_features.copy(), cam_img=np.array([i1, i2], np.int32), feat_point=fp, point_xyz=np.array(seed["point"], np.float64),
                pt_bad=np.zeros(P, np.uint8), pt_mse=np.array(seed["mse"], np.float64), pt_views=np.full(P, 2, np.int32),
                pt_new_added=np.ones(P, np.uint8), cam_R=np.array(seed["cam_R"], np.float64), cam_t=np.array(seed["cam_t"], np.float64),
                cam_c=np.array(seed["cam_c"], np.float64), cam_fk=fk)


def normalize_points(point_xyz, noise=None, target_deviation=100.0, point_sigma=0.5):
    """The arithmetic of msfm_recon_normalize (include/msfm.h) in numpy: add.accumulate sums left to right, as the loops of
    BundleAdjuster::Normalize do.  Returns (mid, scale, the new points); a scale that is not finite raises as the library does."""
    x = np.asarray(point_xyz, np.float64).reshape(-1, 3)
    n = len(x)
    if n == 0:
        raise capi.MsfmError(A.MSFM_E_INVAL, "normalize_points: the state has no point")
    mid = np.add.accumulate(np.concatenate([np.zeros((1, 3)), x]), axis=0)[-1] / n
    d = (np.abs(x[:, 0] - mid[0]) + np.abs(x[:, 1] - mid[1])) + np.abs(x[:, 2] - mid[2])
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = np.float64(target_deviation) / (np.add.accumulate(np.concatenate([[0.0], d]))[-1] / n)
    if not (np.isfinite(scale) and np.isfinite(mid).all()):
        raise capi.MsfmError(A.MSFM_E_NUMERIC, "normalize_points: scale is not finite")
    out = scale * (x - mid)
    if noise is not None:
        out = out + np.asarray(noise, np.float64).reshape(-1, 3) * point_sigma
    return mid, float(scale), out


def _matvec(M, v):
    return np.array([(M[r, 0] * v[0] + M[r, 1] * v[1]) + M[r, 2] * v[2] for r in range(3)])


def normalize_cameras(cam_pose, cam_c, mid, scale, noise=None):
    """The camera side of Normalize and Perturb (optimizer.cc:190-194, :212-231), per camera: SetACPose(a, scale (c - mid)), then
    with noise [n_cams][2][3] (rotation, translation draws) SetACPose(a + 0.1 n_r, c) and SetRTPose(R, t + 0.5 n_t).  Returns
    cam_pose, cam_R, cam_t, cam_c."""
    pose = np.array(cam_pose, np.float64).reshape(-1, 6)
    nc = len(pose)
    R, t, c = np.zeros((nc, 3, 3)), np.zeros((nc, 3)), np.zeros((nc, 3))
    for i in range(nc):
        a = pose[i, :3].copy()
        c[i] = scale * (np.asarray(cam_c, np.float64).reshape(-1, 3)[i] - mid)
        R[i] = scene.angle_axis_to_R(a[None])[0]
        t[i] = -_matvec(R[i], c[i])                               # SetACPose
        if noise is not None:
            nz = np.asarray(noise, np.float64).reshape(nc, 2, 3)
            a = a + nz[i, 0] * ROTATION_SIGMA
            R[i] = scene.angle_axis_to_R(a[None])[0]
            t[i] = -_matvec(R[i], c[i])                           # SetACPose(a + noise, c)
            t[i] = t[i] + nz[i, 1] * TRANSLATION_SIGMA
            a = scene.R_to_angle_axis(R[i]).reshape(3)            # SetRTPose(R, t + noise)
            c[i] = -_matvec(R[i].T, t[i])
        pose[i] = np.concatenate([a, t[i]])
    return pose, R, t, c


class FlatBackend:
    def __init__(self, ctx, store, state, cam_pose, cam_model, cam_model_of_cam, keypoints=None):
        self.ctx, self.store, self.keypoints = ctx, store, keypoints
        self.state = {k: np.array(v) for k, v in state.items()}
        self.cam_pose, self.cam_model = np.array(cam_pose, np.float64).reshape(-1, 6), np.array(cam_model, np.float64).reshape(-1, 3)
        self.cam_model_of_cam = np.array(cam_model_of_cam, np.int32)

    needs_matches, keeps_set = True, False      # what `start_model` asks of seed.find_seed_pair for this backend

    @classmethod
    def from_seed(cls, ctx, store, seed, keypoints=None):
        return cls(ctx, store, state_from_seed(seed, store.n_features), seed["cam_pose"], seed["cam_model"], seed["cam_model_of_cam"], keypoints=keypoints)

    def normalize(self, noise=None):
        mid, scale, self.state["point_xyz"] = normalize_points(self.state["point_xyz"], noise)
        return mid, scale

    def set_cameras(self, cam_pose, cam_R, cam_t, cam_c):
        self.cam_pose = np.array(cam_pose, np.float64)
        self.state.update(cam_R=np.array(cam_R, np.float64), cam_t=np.array(cam_t, np.float64), cam_c=np.array(cam_c, np.float64))

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

    def adjust(self, book, new_cam, visible, full, partial=True):
        r = adjust.adjust_round(self.ctx, self.store, self.state, self.cam_pose, self.cam_model, self.cam_model_of_cam, new_cam, visible,
                                full=full, partial=partial, keypoints=self.keypoints, **book.round_opts)
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

    needs_matches, keeps_set = False, True

    @classmethod
    def from_seed(cls, ctx, store, seed, keypoints=None, **reserve):
        """The model of the winner of seed["set"] (find_seed_pair(keep=True)); the set is closed."""
        b = cls.__new__(cls)
        with seed["set"] as st:
            b.recon = capi.Recon.from_seed(ctx, store, st, seed["cam_pose"], seed["cam_model"], seed["cam_model_of_cam"], keypoints=keypoints, **reserve)
        b._cam_img = [int(i) for i in seed["images"]]
        return b

    def normalize(self, noise=None):
        return self.recon.normalize(noise)

    def set_cameras(self, cam_pose, cam_R, cam_t, cam_c):
        self.recon.set_cameras(cam_pose, cam_R, cam_t, cam_c)

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

    def adjust(self, book, new_cam, visible, full, partial=True):
        return self.recon.adjust(new_cam, visible, partial=partial, full=full, **book.round_opts)

    def fetch(self):
        return self.recon.fetch()

    def n_models(self):
        return self.recon.size()["n_models"]

    def close(self):
        self.recon.close()


def run_round(backend, book, full=None):
    """One pass of :126-186.  Returns the round's record: image (-1: none localised, nothing else ran), f, R, t, avg_error,
    failed_images, visible, n_new, count_outliers / count_new_add / count_outliers_new_add, solved, summary, full.
    full: whether the full adjustment runs (None: on every fifth camera of the model)."""
    cam_img = backend.cam_img()
    processed = np.array(book.processed, bool)
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
    if full is None:
        full = (len(cam_img) + 1) % 5 == 0        # :176-181: every fifth camera
    r = backend.adjust(book, new_cam, visible, full)
    rec.update(f=loc["f"], R=np.array(loc["R"]), t=np.array(loc["t"]), avg_error=loc["avg_error"], n_inliers=loc["n_inliers"], visible=[int(v) for v in visible],
               n_new=int(n_new), full=bool(full), solved=np.array(r["solved"]), summary=r["summary"],
               **{k: r[k] for k in ("count_outliers", "count_new_add", "count_outliers_new_add")})
    return rec


def run_rounds(backend, book, n_rounds):
    return [run_round(backend, book) for _ in range(n_rounds)]


def start_model(backend_cls, ctx, store, book, noise_seed=None, keypoints=None, pair_matches=None, k=64):
    """FindSeedPairThenReconstruct (:224-410) on the images `book.processed` leaves: the ranked pairs in chunks of k until one
    passes the gates, the backend made from it, Normalize and Perturb - the noise from np.random.default_rng(noise_seed)
    .standard_normal in the reference's draw order, points, then rotation and translation per camera; None: no noise - the full
    adjustment and the outlier stage; both images are marked processed and join their groups' camera models.  pair_matches
    (i1, i2) -> the stored matches, for a backend that assembles the state on the host.  Returns (backend, record) or None
    when no pair passes; record: images, n_visited, n_points, fail_times (as the model starts), mid, scale, visible, solved,
    summary and the outlier counts."""
    seed = seedpair.find_seed_pair(ctx, store, book.match_count, book.processed, book.image_f, book.image_group, k=k, keypoints=keypoints,
                                   pair_matches=pair_matches if backend_cls.needs_matches else None, keep=backend_cls.keeps_set, **book.seed_opts)
    if seed is None:
        return None
    backend = backend_cls.from_seed(ctx, store, seed, keypoints=keypoints)
    P = len(seed["point"])
    noise_p = noise_c = None
    if noise_seed is not None:
        rng = np.random.default_rng(noise_seed)
        noise_p = rng.standard_normal((P, 3))
        noise_c = rng.standard_normal((2, 2, 3))
    mid, scale = backend.normalize(noise_p)
    backend.set_cameras(*normalize_cameras(seed["cam_pose"], seed["cam_c"], mid, scale, noise_c))
    r = backend.adjust(book, -1, [], True, partial=False)       # FullBundleAdjustment, RemovePointOutliers (:393-396)
    i1, i2 = seed["images"]
    book.processed[[i1, i2]] = True
    book.image_model[:] = -1                                     # the models of this model: the seed's one or two
    moc = np.asarray(seed["cam_model_of_cam"])
    book.image_model[book.image_group == book.image_group[i2]] = moc[1]
    book.image_model[book.image_group == book.image_group[i1]] = moc[0]
    rec = dict(images=(int(i1), int(i2)), n_visited=seed["n_visited"], n_points=P, fail_times=np.array(book.fail_times), mid=np.array(mid),
               scale=float(scale), visible=[[0, 1], [1, 0]], solved=np.array(r["solved"]), summary=r["summary"],
               **{k: r[k] for k in ("count_outliers", "count_new_add", "count_outliers_new_add")})
    return backend, rec


def reconstruct(backend_cls, ctx, store, book, noise_seed=None, keypoints=None, pair_matches=None, k=64, on_round=None):
    """IncrementalSfM::Run :99-220: models are started (`start_model`) until no pair of unprocessed images passes; each is
    grown by `run_round` until a round localises nothing, the full adjustment on every images_added_total % 5 == 0 with the
    count at 0 behind the seed (:101, :179-180); ClearModel resets fail_times, processed images stay processed.
    on_round(model index, backend): called behind the seed and behind every round that localised an image.
    Returns a list of models: dict(seed = the record of start_model, rounds = the records of run_round, state = the fetched state)."""
    models = []
    while True:
        started = start_model(backend_cls, ctx, store, book, noise_seed=noise_seed, keypoints=keypoints, pair_matches=pair_matches, k=k)
        if started is None:
            return models
        backend, rec0 = started
        if on_round:
            on_round(len(models), backend)
        rounds, added = [], 0
        while True:
            rec = run_round(backend, book, full=(added + 1) % 5 == 0)
            rounds.append(rec)
            if rec["image"] < 0:
                break
            added += 1
            book.processed[rec["image"]] = True
            if on_round:
                on_round(len(models), backend)
        models.append(dict(seed=rec0, rounds=rounds, state=backend.fetch()))
        if hasattr(backend, "close"):
            backend.close()
        book.fail_times[:] = 0                                   # ClearModel
