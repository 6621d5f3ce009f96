"""Cases for msfm_new_points (IncrementalSfM::GenerateNew3DPoints, sfm_incremental.cc:755-915): small worlds in which every
point of a pair (c1, c2) sits on the bisecting plane of the two centres, so its triangulation angle is known exactly -
2 atan((b / 2) / r) - and pixel noise of 1-2 px per view spreads the truncated mse over a few integers (ties exist) without
ever reaching the 3 px gate.  Shared by tests/test_newpoints_ref.py (CPU), tests/test_gpu_newpoints.py,
tests/test_gpu_newpoints_host.py and tests/golden/make_newpoints_golden.py."""
import numpy as np

F = 2400.0
N_POINTS = 1000          # pts_.size() of the handed state: the id base of the new points
# the seeds of walk_case / claims_case / degenerate_case for which the generated data keeps the margins that
# tests/test_newpoints_ref.py asserts
SEED_WALK, SEED_CLAIMS, SEED_DEGENERATE = 13, 12, 13
INPUTS = ("n_features", "pairs", "match_off", "matches", "keypoints", "cam_img", "feat_point", "n_points", "cam_R", "cam_t", "cam_c", "cam_fk",
          "new_cam", "vis_off", "vis_cam")


def _roty(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


class World:
    """cams: list of (centre, rotation about y, k1); cam_img: the image of every camera; n_images >= the largest + 1."""

    def __init__(self, seed, cams, cam_img, n_images):
        self.rng = np.random.Generator(np.random.PCG64(seed))
        self.C = [np.asarray(c, dtype=np.float64) for c, _, _ in cams]
        self.R = [_roty(a) for _, a, _ in cams]
        self.fk = [np.array([F, k1, 0.0]) for _, _, k1 in cams]
        self.cam_img = list(cam_img)
        self.kp = [[] for _ in range(n_images)]
        self.pairs = {}                      # (image 1, image 2) -> matches in stored order
        self.done = {}                       # (camera, feature) -> point id it already holds
        self.new_cam, self.visible = [], []

    def place(self, c1, c2, angle_deg, phi):
        """A point on the bisecting plane of the two centres whose rays meet at exactly angle_deg."""
        d = self.C[c2] - self.C[c1]
        b = np.linalg.norm(d)
        u = d / b
        z = np.array([0.0, 0.0, 1.0]) - u[2] * u
        z /= np.linalg.norm(z)
        y = np.cross(z, u)
        r = (b / 2) / np.tan(np.radians(angle_deg) / 2)
        return (self.C[c1] + self.C[c2]) / 2 + r * (np.cos(phi) * z + np.sin(phi) * y)

    def project(self, c, X):
        pc = self.R[c] @ (np.asarray(X) - self.C[c])
        return F * pc[:2] / pc[2]          # (through the centre for a point behind the camera: the same line)

    def observe(self, c, X, noise=None):
        """A new feature of camera c's image at the projection of X; noise: None = 1-2 px in a random direction, or (dx, dy)."""
        if noise is None:
            a, m = self.rng.uniform(0, 2 * np.pi), self.rng.uniform(1.0, 2.0)
            noise = (m * np.cos(a), m * np.sin(a))
        return self.feature(c, self.project(c, X) + np.asarray(noise))

    def feature(self, c, xy):
        k = self.kp[self.cam_img[c]]
        k.append(np.asarray(xy, dtype=np.float32))
        return len(k) - 1

    def filler(self, c, n):
        for _ in range(n):
            self.feature(c, self.rng.uniform(-900, 900, 2))

    def match(self, c1, c2, f1, f2):
        self.pairs.setdefault((self.cam_img[c1], self.cam_img[c2]), []).append((f1, f2))

    def points(self, c1, c2, n, angle_deg, noise=None, behind=False):
        """n matches of the pair (c1, c2), each a new point at that angle with a new feature in both images."""
        out = []
        for _ in range(n):
            X = self.place(c1, c2, angle_deg, self.rng.uniform(-0.3, 0.3))
            if behind:                       # mirrored through the baseline: the two lines meet behind both cameras
                X = self.C[c1] + self.C[c2] - X
            f1, f2 = self.observe(c1, X, noise), self.observe(c2, X, noise)
            self.match(c1, c2, f1, f2)
            out.append((f1, f2))
        return out

    def image_pair(self, i1, i2, n):
        """n matches between two images whatever they show (pairs no walk touches)."""
        while len(self.kp[i1]) < n:
            self.kp[i1].append(self.rng.uniform(-900, 900, 2).astype(np.float32))
        while len(self.kp[i2]) < n:
            self.kp[i2].append(self.rng.uniform(-900, 900, 2).astype(np.float32))
        self.pairs.setdefault((i1, i2), []).extend((j, n - 1 - j) for j in range(n))

    def mark(self, c, f):
        self.done[(c, f)] = int(self.rng.integers(0, N_POINTS))

    def new(self, c1, visible):
        self.new_cam.append(c1)
        self.visible.append(list(visible))

    def case(self):
        nf = np.array([len(k) for k in self.kp], np.int32)
        keys = sorted(self.pairs)
        pairs = np.array(keys, np.int32).reshape(-1, 2)
        moff = np.concatenate([[0], np.cumsum([len(self.pairs[k]) for k in keys])]).astype(np.int32)
        matches = np.array([m for k in keys for m in self.pairs[k]], np.int32).reshape(-1, 2)
        kp = np.array([p for k in self.kp for p in k], np.float32).reshape(-1, 2)
        cam_img = np.array(self.cam_img, np.int32)
        cam_fo = np.concatenate([[0], np.cumsum(nf[cam_img])])
        fp = np.full(cam_fo[-1], -1, np.int32)
        for (c, f), p in self.done.items():
            fp[cam_fo[c] + f] = p
        R = np.array(self.R)
        C = np.array(self.C)
        t = -np.einsum("nij,nj->ni", R, C)
        voff = np.concatenate([[0], np.cumsum([len(v) for v in self.visible])]).astype(np.int32)
        vcam = np.array([c for v in self.visible for c in v], np.int32)
        return dict(n_features=nf, pairs=pairs, match_off=moff, matches=matches, keypoints=kp, cam_img=cam_img, feat_point=fp,
                    n_points=np.int32(N_POINTS), cam_R=R, cam_t=t, cam_c=C, cam_fk=np.array(self.fk), new_cam=np.array(self.new_cam, np.int32),
                    vis_off=voff, vis_cam=vcam)


def sub(c, ks):
    """The case with only the new cameras `ks` of c."""
    ks = list(ks)
    vis = [c["vis_cam"][c["vis_off"][k]:c["vis_off"][k + 1]] for k in ks]
    d = dict(c)
    d["new_cam"] = c["new_cam"][ks].astype(np.int32)
    d["vis_off"] = np.concatenate([[0], np.cumsum([len(v) for v in vis])]).astype(np.int32)
    d["vis_cam"] = np.concatenate(vis + [np.zeros(0, np.int32)]).astype(np.int32)
    return d


def store_args(c):
    return c["n_features"], c["pairs"], c["match_off"], c["matches"]


def ref_args(c):
    """Positional arguments of tests/newpoints_ref.py::new_points behind the library handle."""
    return [c[k] for k in ("n_features", "pairs", "match_off", "matches", "keypoints", "cam_img", "feat_point", "cam_R", "cam_t", "cam_c", "cam_fk",
                           "new_cam", "vis_off", "vis_cam")]


def call_args(c):
    """Positional arguments of Context.new_points behind the store."""
    return [c[k] for k in ("cam_img", "feat_point", "n_points", "cam_R", "cam_t", "cam_c", "cam_fk", "new_cam", "vis_off", "vis_cam")]


def legacy_args(c, k=0):
    """The arguments of tracks.generate_new_points / oracle.generate_new_points for new camera k: per-camera lists."""
    nf, ci = c["n_features"], c["cam_img"]
    fo = np.concatenate([[0], np.cumsum(nf)])
    cam_fo = np.concatenate([[0], np.cumsum(nf[ci])])
    kp = [c["keypoints"][fo[i]:fo[i + 1]] for i in ci]
    fp = [c["feat_point"][cam_fo[j]:cam_fo[j + 1]] >= 0 for j in range(len(ci))]
    where = {(int(a), int(b)): p for p, (a, b) in enumerate(c["pairs"])}
    c1 = int(c["new_cam"][k])
    vis = [int(v) for v in c["vis_cam"][c["vis_off"][k]:c["vis_off"][k + 1]]]
    mpc = []
    for c2 in vis:
        p = where.get((int(ci[c1]), int(ci[c2])))
        mpc.append(np.zeros((0, 2), np.int32) if p is None or c2 == c1 else c["matches"][c["match_off"][p]:c["match_off"][p + 1]])
    return c1, vis, mpc, fp[c1], [fp[c2] for c2 in vis], kp, c["cam_R"], c["cam_t"], c["cam_c"], c["cam_fk"]


# ---- the walk: new camera 0 with the visible list [itself, a camera whose pair the store lacks, 500, 501, 257, 5 matches] ----
WALK_VISIBLE = [0, 1, 2, 3, 4, 5]
WALK_N_MATCHES = [0, 0, 500, 501, 257, 5]
WALK_LARGE = [0, 0, 0, 1, 0, 0]
WALK_BLOCK = 200                      # points at 4 degrees in the pairs of 500 and 501 matches: between the two thresholds
# 257: matches 10..19 have f1 triangulated, 20..24 f2, match 256 repeats match 3; 30 of the candidates sit at 1.5 degrees
WALK_N_CANDIDATES = [0, 0, 500, 501, 242, 5]
WALK_N_ACCEPTED = [0, 0, 500, 301, 212, 5]
WALK_CAMS = [((0, 0, 0), 0.0, 0.0), ((3, 0, 0), 0.01, 0.0), ((10, 0, 0), -0.02, 0.0), ((-8, 1, 0), 0.03, 0.0), ((6, -2, 0.5), 0.0, 1e-3),
             ((0, 7, 0), -0.01, 0.0), ((5, 5, 0), 0.0, 0.0)]
WALK_IMG = [4, 0, 6, 2, 7, 1, 5]      # images 3 and 8 have no camera


def walk_world(seed):
    w = World(seed, WALK_CAMS, WALK_IMG, 9)
    for c, n in ((0, 3), (2, 1), (4, 5)):
        w.filler(c, n)
    for c2 in (2, 3):
        w.points(0, c2, WALK_BLOCK, 4.0)
        w.points(0, c2, 300 + (c2 == 3), 8.0)
    m = w.points(0, 4, 40, 8.0) + w.points(0, 4, 30, 1.5) + w.points(0, 4, 186, 8.0)
    for f1, _ in m[10:20]:
        w.mark(0, f1)
    for _, f2 in m[20:25]:
        w.mark(4, f2)
    w.match(0, 4, *m[3])
    w.points(0, 5, 5, 8.0)
    # other rows of the store, and what makes cameras 3 and 5 new cameras of their own (independence)
    w.points(3, 0, 40, 8.0)
    w.points(3, 2, 33, 7.0)
    w.points(5, 3, 21, 9.0)
    w.points(5, 0, 10, 6.0)
    w.points(6, 0, 12, 8.0)
    w.image_pair(3, 8, 50)
    w.new(0, WALK_VISIBLE)
    w.new(3, [0, 2, 3])
    w.new(5, [3, 0, 0])               # (a camera listed twice is walked twice)
    return w


def walk_case(seed):
    return walk_world(seed).case()


def with_unrelated(c, n, seed=1):
    """The store of c with n more matches in pairs between the two images without a camera (3 and 8)."""
    rng = np.random.default_rng(seed)
    d = {(int(a), int(b)): c["matches"][c["match_off"][p]:c["match_off"][p + 1]] for p, (a, b) in enumerate(c["pairs"])}
    nf = c["n_features"]
    for key in ((3, 8), (8, 3)):
        d[key] = np.column_stack([rng.integers(0, nf[key[0]], n), rng.integers(0, nf[key[1]], n)]).astype(np.int32)
    keys = sorted(d)
    out = dict(c)
    out["pairs"] = np.array(keys, np.int32)
    out["match_off"] = np.concatenate([[0], np.cumsum([len(d[k]) for k in keys])]).astype(np.int32)
    out["matches"] = np.concatenate([d[k] for k in keys]).astype(np.int32)
    return out


# ---- claims: one feature of the new camera matched in three visible cameras; one feature of camera 2 in two matches of a pair ----
def claims_case(seed):
    w = World(seed, [((0, 0, 0), 0.0, 0.0), ((10, 0, 0), 0.0, 0.0), ((-9, 0, 0), 0.02, 0.0), ((0, 9, 0), 0.0, 0.0)], [2, 0, 3, 1], 4)
    for c2 in (1, 2, 3):
        w.points(0, c2, 20, 8.0)
    X = w.place(0, 1, 8.0, 0.1)
    shared = w.observe(0, X, (0.0, 0.0))
    # offsets of d px across the epipolar lines (horizontal for cameras 1 and 2, vertical for camera 3): mse ~ d^2 / 4, so
    # entry 0 gets key 2 and entries 1, 2 key 0 (a tie)
    for c2, d in ((1, (0.0, 3.0)), (2, (0.0, 1.0)), (3, (1.0, 0.0))):
        w.match(0, c2, shared, w.observe(c2, X, d))
    X2 = w.place(0, 2, 8.0, -0.2)
    g2 = w.observe(2, X2, (0.0, 0.0))
    a, b = w.observe(0, X2, (0.0, 3.0)), w.observe(0, X2, (0.0, 1.0))
    w.match(0, 2, a, g2)              # walk-first, key 2
    w.match(0, 2, b, g2)              # sorted-first, key 0
    for c2 in (1, 2, 3):
        w.points(0, c2, 7, 8.0)
    w.new(0, [1, 2, 3])
    c = w.case()
    c["shared_f1"], c["shared_f2"], c["shared_f2_cam"] = shared, g2, 2
    return c


# ---- degenerate: a visible camera at the new camera's centre; points behind both cameras ----
DEGENERATE_N_MATCHES = [15, 12, 9]
DEGENERATE_N_ACCEPTED = [0, 0, 9]            # default options
DEGENERATE_N_ACCEPTED_400 = [0, 12, 9]       # th_mse_reprojection = 400: sqrt(100000) = 316.2 passes, with the key 100000


def degenerate_case(seed):
    w = World(seed, [((0, 0, 0), 0.0, 0.0), ((0, 0, 0), 0.05, 0.0), ((10, 0, 0), 0.0, 0.0), ((0, -9, 0), 0.0, 0.0)], [0, 1, 2, 3], 4)
    for _ in range(DEGENERATE_N_MATCHES[0]):
        X = np.array([w.rng.uniform(-20, 20), w.rng.uniform(-20, 20), 70.0])
        w.match(0, 1, w.observe(0, X), w.observe(1, X))
    w.points(0, 2, DEGENERATE_N_MATCHES[1], 8.0, behind=True)
    w.points(0, 3, DEGENERATE_N_MATCHES[2], 8.0)
    w.new(0, [1, 2, 3])
    return w.case()


# ---- the golden case: th_matches_large = 40, so a pair of 41 matches gets the large angle ----
GOLDEN_OPTS = dict(th_matches_large=40)


def golden_case():
    w = World(20261018, WALK_CAMS[:5], [3, 0, 4, 1, 2], 6)
    w.filler(0, 2)
    w.points(0, 2, 25, 4.0)
    w.points(0, 2, 15, 8.0)
    w.points(0, 3, 20, 4.0)
    m = w.points(0, 3, 21, 8.0)
    w.mark(0, m[2][0])
    w.mark(3, m[5][1])
    w.match(0, 3, *m[7])
    w.points(0, 4, 9, 1.5)
    w.points(0, 4, 6, 9.0)
    w.points(2, 0, 17, 8.0)
    w.image_pair(5, 3, 30)
    w.new(0, [1, 0, 2, 3, 4])
    w.new(2, [0, 2])
    return w.case()


# ---- the host mirror's driver, tests/newpoints_host_check.cc ----
def newest_last(c):
    """The one-new-camera case c with its cameras reordered so that the new camera is the newest, cams_.size() - 1, as
    IncrementalSfM::GenerateNew3DPoints takes it."""
    assert len(c["new_cam"]) == 1
    n, c1 = len(c["cam_img"]), int(c["new_cam"][0])
    order = [k for k in range(n) if k != c1] + [c1]
    new_index = np.empty(n, np.int32)
    new_index[order] = np.arange(n, dtype=np.int32)
    cam_fo = np.concatenate([[0], np.cumsum(c["n_features"][c["cam_img"]])])
    d = dict(c)
    d["cam_img"] = c["cam_img"][order]
    d["feat_point"] = np.concatenate([c["feat_point"][cam_fo[k]:cam_fo[k + 1]] for k in order]).astype(np.int32)
    for key in ("cam_R", "cam_t", "cam_c", "cam_fk"):
        d[key] = np.ascontiguousarray(c[key][order])
    d["new_cam"] = np.array([n - 1], np.int32)
    d["vis_cam"] = new_index[c["vis_cam"]]
    return d


def host_check_command(exe):
    """The compiler call for tests/newpoints_host_check.cc against this tree's library."""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "metricsfm_amd")
    return ["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(root, "host"), "-I", os.path.join(root, "include"),
            os.path.join(root, "tests", "newpoints_host_check.cc"), os.path.join(root, "host", "objectsfm.cc"), "-o", str(exe),
            "-L" + lib, "-lmsfm", "-Wl,-rpath," + lib, "-Wl,-rpath-link,/opt/rocm/lib"]


def write_model(path, c):
    """A model in the byte layout tests/newpoints_host_check.cc reads (the new camera is the last one)."""
    assert len(c["new_cam"]) == 1 and c["new_cam"][0] == len(c["cam_img"]) - 1
    i32 = lambda x: np.ascontiguousarray(np.asarray(x, dtype=np.int32).reshape(-1))
    f64 = lambda x: np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1))
    with open(path, "wb") as fh:
        for a in ([len(c["n_features"])], c["n_features"], [len(c["pairs"])], c["pairs"], c["match_off"], c["matches"], [len(c["cam_img"])],
                  c["cam_img"], c["feat_point"], [int(c["n_points"])], [len(c["vis_cam"])], c["vis_cam"]):
            fh.write(i32(a).tobytes())
        for a in (c["cam_R"], c["cam_t"], c["cam_c"], c["cam_fk"]):
            fh.write(f64(a).tobytes())
        fh.write(np.ascontiguousarray(c["keypoints"], dtype=np.float32).tobytes())


def read_host_result(path, c):
    raw = open(path, "rb").read()
    n = int(np.frombuffer(raw, np.int32, 1)[0])
    rec = np.frombuffer(raw, np.int32, 5 * n, 4).reshape(n, 5)
    nfp = int(c["n_features"][c["cam_img"]].sum())
    at = 4 + 20 * n
    fp = np.frombuffer(raw, np.int32, nfp, at)
    at += 4 * nfp
    X = np.frombuffer(raw, np.float64, 3 * n, at).reshape(n, 3)
    mse = np.frombuffer(raw, np.float64, n, at + 24 * n)
    return dict(global1=rec[:, 0], global2=rec[:, 1], cam2=rec[:, 2], takes1=rec[:, 3], takes2=rec[:, 4], feat_point=fp, X=X, mse=mse)
