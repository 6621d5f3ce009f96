"""Cases for msfm_round_adjust (PartialBundleAdjustment / FullBundleAdjustment / RemovePointOutliers on the flat state,
sfm_incremental.cc:172-186), in the pattern of tests/newpoints_data.py: a small world of cameras looking down +z at points 60-80
units away, observed with a fraction of a pixel of noise; the state's points sit a little off the truth, so that a solve moves
them and the reprojection errors straddle the 1 px outlier gate.  Shared by tests/test_round_ref.py (CPU), tests/test_gpu_round.py
and scripts/round_bench.py."""
import numpy as np

F = 2400.0
SEED_MAIN, SEED_OUTLIERS = 5, 11      # seeds for which tests/test_round_ref.py asserts the margins
STATE = ("n_features", "cam_img", "feat_point", "obs_point", "obs_cam", "obs_feat", "point_xyz", "pt_bad", "pt_mse", "pt_mutable", "pt_new_added")


def _roty(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


class World:
    """cams: list of (centre, rotation about y); cam_img: the image of every camera (n_images >= the largest + 1);
    cam_model_of_cam and models [n_models][3] = f, k1, k2."""

    def __init__(self, seed, cams, cam_img, n_images, cam_model_of_cam, models):
        self.rng = np.random.Generator(np.random.PCG64(seed))
        self.C = [np.asarray(c, dtype=np.float64) for c, _ in cams]
        self.yaw = [float(a) for _, a in cams]
        self.R = [_roty(a) for a in self.yaw]
        self.cam_img = list(cam_img)
        self.moc = list(cam_model_of_cam)
        self.models = np.array(models, np.float64).reshape(-1, 3)
        self.kp = [[] for _ in range(n_images)]
        self.held = {}                       # (camera, feature) -> the point Camera::pts_ holds there
        self.rows = []                       # (point, camera, feature): Point3D::AddObservation in call order
        self.X, self.bad, self.mut, self.added = [], [], [], []

    def project(self, c, X):
        pc = self.R[c] @ (np.asarray(X) - self.C[c])
        f, k1, k2 = self.models[self.moc[c]]
        x, y = pc[0] / pc[2], pc[1] / pc[2]
        r2 = x * x + y * y
        d = 1.0 + r2 * (k1 + k2 * r2)
        return np.array([f * d * x, f * d * y])

    def feature(self, c, xy):
        k = self.kp[self.cam_img[c]]
        k.append(np.asarray(xy, dtype=np.float32))
        return len(k) - 1

    def observe(self, c, X, noise):
        a = self.rng.uniform(0, 2 * np.pi)
        return self.feature(c, self.project(c, X) + noise * np.array([np.cos(a), np.sin(a)]))

    def filler(self, c, n):
        for _ in range(n):
            self.feature(c, self.rng.uniform(-900, 900, 2))

    def place(self):
        return np.array([self.rng.uniform(-15, 15), self.rng.uniform(-15, 15), self.rng.uniform(60, 80)])

    def point(self, X, off=0.03, bad=0, mutable=1, added=0):
        """A new point of the state, `off` units away from X in a random direction.  Returns its id."""
        d = self.rng.normal(size=3)
        self.X.append(np.asarray(X, dtype=np.float64) + off * d / np.linalg.norm(d))
        self.bad.append(bad); self.mut.append(mutable); self.added.append(added)
        return len(self.X) - 1

    def row(self, p, c, f, takes=True):
        """Point3D::AddObservation(cams_[c], .., f); with `takes` Camera::AddPoints took too."""
        self.rows.append((p, c, f))
        if takes:
            assert (c, f) not in self.held
            self.held[(c, f)] = p

    def track(self, cams, X=None, noise=0.3, **kw):
        """A point seen by `cams`, a new feature in each, every insert taking."""
        X = self.place() if X is None else X
        p = self.point(X, **kw)
        for c in cams:
            self.row(p, c, self.observe(c, X, noise))
        return p

    def case(self, new_cam, visible, shuffle=True, mse_seed=1):
        nf = np.array([len(k) for k in self.kp], np.int32)
        kp = np.array([p for k in self.kp for p in k], np.float32).reshape(-1, 2)
        cam_img = np.array(self.cam_img, np.int32)
        cam_fo = np.concatenate([[0], np.cumsum(nf[cam_img])])
        fp = np.full(cam_fo[-1], -1, np.int32)
        for (c, f), p in self.held.items():
            fp[cam_fo[c] + f] = p
        rows = np.array(self.rows, np.int32).reshape(-1, 3)
        if shuffle:
            rows = rows[self.rng.permutation(len(rows))]
        R = np.array(self.R).reshape(-1, 3, 3)
        C = np.array(self.C).reshape(-1, 3)
        pose = np.zeros((len(self.C), 6))
        pose[:, 1] = self.yaw                          # angle-axis (0, a, 0) is the rotation about y
        pose[:, 3:] = -np.einsum("nij,nj->ni", R, C)
        n = len(self.X)
        return dict(n_features=nf, keypoints=kp, cam_img=cam_img, feat_point=fp, obs_point=rows[:, 0].copy(), obs_cam=rows[:, 1].copy(),
                    obs_feat=rows[:, 2].copy(), cam_pose=pose, cam_model=self.models.copy(), cam_model_of_cam=np.array(self.moc, np.int32),
                    point_xyz=np.array(self.X, np.float64).reshape(-1, 3), pt_bad=np.array(self.bad, np.uint8),
                    pt_mse=np.random.default_rng(mse_seed).uniform(0.0, 0.5, n), pt_mutable=np.array(self.mut, np.uint8),
                    pt_new_added=np.array(self.added, np.uint8), new_cam=int(new_cam), visible=np.array(visible, np.int32))


def store_args(c):
    """A match store over the case's images (the call reads n_features of it, nothing else): one pair with one match."""
    two = [i for i in range(len(c["n_features"])) if c["n_features"][i] > 0][:2]
    if len(two) < 2:
        return c["n_features"], np.zeros((0, 2), np.int32), np.zeros(1, np.int32), np.zeros((0, 2), np.int32)
    return c["n_features"], np.array([two], np.int32), np.array([0, 1], np.int32), np.zeros((1, 2), np.int32)


def call_args(c):
    """Positional arguments of Context.round_adjust behind the store."""
    return [c[k] for k in ("cam_img", "feat_point", "obs_point", "obs_cam", "obs_feat", "cam_pose", "cam_model", "cam_model_of_cam", "point_xyz",
                           "pt_bad", "pt_mse", "pt_mutable")]


# ---- the main case: 8 cameras in two models, camera index order unlike image order; new camera 7 with the visible list [7, 2] ----
MAIN_CAMS = [((-9, -3, 0), 0.02), ((-6, 4, 0), -0.01), ((-2, -5, 0.5), 0.0), ((1, 3, 0), 0.03), ((4, -2, 0), -0.02), ((7, 5, -0.5), 0.01),
             ((9, -4, 0), 0.0), ((3, 0, 0), -0.03)]
MAIN_IMG = [5, 2, 9, 0, 7, 3, 8, 1]        # images 4 and 6 have no camera
MAIN_MODEL = [0, 0, 0, 0, 0, 1, 1, 1]
MAIN_MODELS = [[F, 1e-3, 0.0], [0.98 * F, -2e-3, 1e-4]]
MAIN_NEW, MAIN_VISIBLE = 7, [7, 2]
MAIN_FREE = [2, 5, 6, 7]                    # model 1 and the visible cameras
MAIN_FROZEN = [0, 1, 3, 4]


def main_world(seed=SEED_MAIN):
    w = World(seed, MAIN_CAMS, MAIN_IMG, 10, MAIN_MODEL, MAIN_MODELS)
    rng = w.rng
    for c in (0, 3, 6):
        w.filler(c, 3)
    tag = {}
    for k in range(270):                    # tracks of 2, 3 and 5 views over all cameras
        n = (2, 3, 5)[k % 3]
        w.track(rng.choice(8, n, replace=False).tolist(), added=int(k % 7 == 0))
    tag["frozen_only"] = [w.track([0, 1]), w.track([4, 3, 1]), w.track([3, 0, 4, 1])]       # held only by frozen cameras
    tag["bad_inside"] = [w.track([7, 2], bad=1, added=1), w.track([5, 0, 6], bad=1)]         # bad, in the window
    tag["bad_outside"] = [w.track([0, 4], bad=1), w.track([1, 3, 4], bad=1, added=1)]        # bad, outside it
    tag["bad_far"] = [w.track([7, 5, 2], off=2.0, bad=1)]
    # points whose Camera::AddPoints did not take: the feature belongs to an earlier point (msfm_new_points' takes1 / takes2 = 0)
    held = {c: [f for (cc, f) in w.held if cc == c] for c in range(8)}

    def untaken(c1, c2, fail1, fail2, mutable):
        X = w.place()
        p = w.point(X, mutable=mutable, added=1)
        for c, fail in ((c1, fail1), (c2, fail2)):
            if fail:
                w.row(p, c, held[c][int(rng.integers(len(held[c])))], takes=False)
            else:
                w.row(p, c, w.observe(c, X, 0.3))
        return p
    tag["takes1_failed"] = [untaken(7, 2, True, False, 1), untaken(7, 0, True, False, 1)]
    tag["takes2_failed"] = [untaken(7, 5, False, True, 1), untaken(6, 1, False, True, 0)]
    # no camera holds these: the incoming flag decides (rows on free cameras with 0 and 1, rows on frozen cameras with 0 and 1)
    tag["unheld"] = [untaken(7, 2, True, True, 0), untaken(7, 6, True, True, 1), untaken(0, 1, True, True, 0), untaken(3, 4, True, True, 1)]
    for p in (3, 10, 77, tag["unheld"][1]):   # duplicate rows: the same observation added again
        first = next(r for r in w.rows if r[0] == p)
        w.rows.append(first)
    w.tag = tag
    return w


def main_case(seed=SEED_MAIN):
    w = main_world(seed)
    c = w.case(MAIN_NEW, MAIN_VISIBLE)
    c["tag"] = w.tag
    return c


# ---- sizes: n_points tracks of 2 or 3 views over four cameras of one model ----
SIZE_CAMS = [((-6, 0, 0), 0.01), ((-2, 2, 0), 0.0), ((2, -2, 0), -0.01), ((6, 1, 0), 0.02)]


def sized_case(n_points, n_rows=None, seed=3, all_bad=False):
    """n_points points; with n_rows, two-view tracks only and duplicate rows up to exactly n_rows rows."""
    w = World(seed, SIZE_CAMS, [2, 0, 3, 1], 4, [0, 0, 0, 0], [[F, 0.0, 0.0]])
    for k in range(n_points):
        n = 2 if n_rows is not None else 2 + k % 2
        w.track(w.rng.choice(4, n, replace=False).tolist(), bad=int(all_bad), added=k % 2)
    if n_rows is not None:
        assert n_rows >= len(w.rows)
        for k in range(n_rows - len(w.rows)):
            w.rows.append(w.rows[5 * k])
    return w.case(3, [3, 0])


def long_track_case(seed=4):
    """72 cameras on a line, one track of 70 views (longer than a wave) among short ones."""
    cams = [((-18 + 0.5 * k, (k % 3) - 1.0, 0), 0.001 * (k % 5)) for k in range(72)]
    img = np.random.default_rng(seed).permutation(72).tolist()
    w = World(seed, cams, img, 72, [0] * 72, [[F, 0.0, 0.0]])
    for k in range(20):
        w.track(w.rng.choice(72, 2 + k % 3, replace=False).tolist())
    long = w.track(w.rng.choice(72, 70, replace=False).tolist(), added=1)
    for k in range(20):
        w.track(w.rng.choice(72, 2 + k % 3, replace=False).tolist())
    c = w.case(71, [71, 0, 5])
    c["long"] = long
    return c


def empty_case():
    """Cameras and features, no point and no observation."""
    w = World(1, SIZE_CAMS, [2, 0, 3, 1], 4, [0, 0, 0, 0], [[F, 0.0, 0.0]])
    for c in range(4):
        w.filler(c, 5)
    return w.case(3, [3])


# ---- outliers alone, on a hand-set state: the answer does not pass through a solve ----
OUT_CAMS = [((0, 0, 0), 0.0), ((8, 0, 0), -0.02), ((-7, 2, 0), 0.03), ((2, -6, 0), 0.0), ((0, 0, 150), np.pi)]   # camera 4 looks back
OUT_IMG = [3, 1, 4, 0, 2]                   # key order of a point's rows: cameras 3, 1, 4, 0, 2
OUT_NOISE = [0.1, 0.3, 0.5, 0.7, 0.9, 1.2, 1.5, 2.0, 3.0, 6.0]


def outlier_world(seed=SEED_OUTLIERS):
    w = World(seed, OUT_CAMS, OUT_IMG, 5, [0, 0, 1, 1, 0], [[F, 1e-3, 0.0], [1.1 * F, 0.0, 1e-4]])
    tag = {}
    tag["spread"] = [w.track(w.rng.choice(4, 2 + k % 3, replace=False).tolist(), noise=OUT_NOISE[k % 10], off=0.0, added=k % 2) for k in range(60)]
    Xf = np.array([1.0, -2.0, 170.0])      # in front of cameras 0-3, behind camera 4, which looks back from z = 150
    # behind the SECOND camera of its key order - camera 3 (image 0), camera 4 (image 2), camera 0 (image 3): the first row's
    # error, tens of pixels, is discarded and the third row is never reached
    p = w.point(Xf, off=0.0, added=1)
    w.row(p, 0, w.observe(0, Xf, 30.0))
    w.row(p, 4, w.feature(4, (3.0, 4.0)))
    w.row(p, 3, w.observe(3, Xf, 30.0))
    tag["behind_second"] = p
    # behind the first - camera 4 (image 2), camera 0 (image 3), camera 2 (image 4)
    p = w.point(Xf, off=0.0)
    w.row(p, 2, w.observe(2, Xf, 0.2))
    w.row(p, 4, w.feature(4, (-8.0, 1.0)))
    w.row(p, 0, w.observe(0, Xf, 0.2))
    tag["behind_first"] = p
    tag["back_view"] = w.track([4, 3, 0], X=np.array([2.0, 1.0, 70.0]), noise=0.2, off=0.0)    # in front of camera 4 too
    X = np.array([2.0, 1.0, 70.0])
    tag["nan"] = w.track([0, 1, 2], added=1)
    w.X[tag["nan"]] = np.array([np.nan, 1.0, 70.0])
    tag["no_rows"] = w.point(X, added=1)
    tag["bad"] = [w.track([0, 1], noise=9.0, bad=1, added=1), w.track([2, 3, 1], noise=0.1, bad=1, added=0)]
    w.tag = tag
    return w


def outlier_case(seed=SEED_OUTLIERS):
    w = outlier_world(seed)
    c = w.case(-1, [])
    c["tag"] = w.tag
    return c


# ---- a state derived from a scene.Scene: camera index = image id, every observation a feature of its own, every insert taking ----
def scene_state(sc, bad=None):
    """The flat state of a Scene whose obs_xy was rounded to float32 first (the state keeps keypoints as floats)."""
    n_cams, n_obs = sc.n_cams, len(sc.obs_cam)
    nf = np.bincount(sc.obs_cam, minlength=n_cams).astype(np.int32)
    order = np.argsort(sc.obs_cam, kind="stable")
    feat = np.empty(n_obs, np.int32)
    start = np.concatenate([[0], np.cumsum(nf)])
    feat[order] = (np.arange(n_obs) - start[sc.obs_cam[order]]).astype(np.int32)
    fp = sc.obs_pt[order].astype(np.int32)
    kp = sc.obs_xy[order].astype(np.float32)
    return dict(n_features=nf, keypoints=kp, cam_img=np.arange(n_cams, dtype=np.int32), feat_point=fp, obs_point=sc.obs_pt.astype(np.int32),
                obs_cam=sc.obs_cam.astype(np.int32), obs_feat=feat, cam_pose=sc.cam_pose.copy(), cam_model=sc.cam_model.copy(),
                cam_model_of_cam=sc.cam_model_of_cam.astype(np.int32), point_xyz=sc.point.copy(),
                pt_bad=np.zeros(sc.n_points, np.uint8) if bad is None else np.asarray(bad, np.uint8), pt_mse=np.zeros(sc.n_points),
                pt_mutable=np.ones(sc.n_points, np.uint8), pt_new_added=np.zeros(sc.n_points, np.uint8))


def points_without_rows_case(seed=6):
    """Points and cameras that hold none of them, and not one observation row: every segment is empty."""
    w = World(seed, SIZE_CAMS, [2, 0, 3, 1], 4, [0, 0, 0, 0], [[F, 0.0, 0.0]])
    for c in range(4):
        w.filler(c, 5)
    for k in range(300):
        w.point(w.place(), mutable=k % 2, added=k % 3 == 0, bad=int(k % 11 == 0))
    return w.case(3, [3, 1])


# ---- the host mirror's driver, tests/round_host_check.cc ----
def host_check_command(exe):
    """The compiler call for tests/round_host_check.cc against this tree's library."""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "metricsfm_amd")
    return ["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(root, "host"), "-I", os.path.join(root, "include"),
            os.path.join(root, "tests", "round_host_check.cc"), os.path.join(root, "host", "objectsfm.cc"), "-o", str(exe),
            "-L" + lib, "-lmsfm", "-Wl,-rpath," + lib, "-Wl,-rpath-link,/opt/rocm/lib"]


def write_model(path, c):
    """A model in the byte layout tests/round_host_check.cc reads."""
    i32 = lambda x: np.ascontiguousarray(np.asarray(x, dtype=np.int32).reshape(-1))
    f64 = lambda x: np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1))
    with open(path, "wb") as fh:
        for a in ([len(c["n_features"])], c["n_features"], [len(c["cam_img"])], c["cam_img"], c["feat_point"], [len(c["pt_bad"]), len(c["obs_point"])],
                  c["obs_point"], c["obs_cam"], c["obs_feat"], [len(c["cam_model"])], c["cam_model_of_cam"], [c["new_cam"], len(c["visible"])],
                  c["visible"], c["pt_bad"], c["pt_mutable"], c["pt_new_added"]):
            fh.write(i32(a).tobytes())
        for a in (c["cam_pose"], c["cam_model"], c["point_xyz"], c["pt_mse"]):
            fh.write(f64(a).tobytes())
        fh.write(np.ascontiguousarray(c["keypoints"], dtype=np.float32).tobytes())


def read_host_result(path, c):
    raw = open(path, "rb").read()
    nc, nm, n = len(c["cam_img"]), len(c["cam_model"]), len(c["pt_bad"])
    at = 0

    def take(dtype, count, shape):
        nonlocal at
        a = np.frombuffer(raw, dtype, count, at).reshape(shape)
        at += a.nbytes
        return a
    out = dict(cam_pose=take(np.float64, 6 * nc, (nc, 6)), cam_model=take(np.float64, 3 * nm, (nm, 3)), point_xyz=take(np.float64, 3 * n, (n, 3)),
               pt_mse=take(np.float64, n, (n,)))
    for k in ("pt_bad", "pt_mutable", "pt_new_added"):
        out[k] = take(np.int32, n, (n,)).astype(np.uint8)
    out["counts"], out["adjust"], out["solved"] = take(np.int32, 3, (3,)), take(np.int32, 4, (2, 2)), take(np.int32, 2, (2,))
    return out
