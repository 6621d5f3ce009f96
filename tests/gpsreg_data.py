"""Seeded cases of the SLAM + GPS registration tests (tests/test_gpsreg_ref.py, tests/test_gpu_gpsreg.py): camera paths with
a planted similarity onto their GPS track, and two CSR track sets that reach every path of the accuracy / GPS-shift kernels."""
import numpy as np

from metricsfm_amd import _abi as A

PLANTED_SCALE = 3.7
PLANTED_AA = np.array([0.31, -0.22, 0.83])          # a general rotation
PLANTED_T = np.array([4.0e5, -3.1e5, 2.6e2])        # large: the offset of slam_gps.cc:1651-1673 matters
GPS_NOISE = 0.3
SLICE_ROWS = 256                                    # rows of a workgroup's slice in gpsreg.hip's row form


def rodrigues(aa):
    aa = np.asarray(aa, dtype=np.float64)
    th = np.linalg.norm(aa)
    if th < 1e-12:
        return np.eye(3)
    k = aa / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def path_centres(kind):
    """Camera centres in the model's own frame."""
    if kind == "lawn60":     # two straight legs and a turn: the weights run from tan(0) on a leg to the 80 degree clip
        leg1 = np.column_stack([np.arange(25) * 2.0, np.zeros(25), np.full(25, 30.0)])
        ang = np.linspace(0, np.pi, 12)[1:-1]
        turn = np.column_stack([48.0 + 6.0 * np.sin(ang), 6.0 - 6.0 * np.cos(ang), np.full(10, 30.0)])
        leg2 = np.column_stack([48.0 - np.arange(25) * 2.0, np.full(25, 12.0), np.full(25, 30.0)])
        c = np.concatenate([leg1, turn, leg2])
    elif kind == "line5":    # both clamps of :1607-1614 act on every camera
        c = np.column_stack([np.arange(5) * 3.0, 0.4 * np.arange(5) ** 2, np.full(5, 25.0)])
    elif kind == "tri3":
        c = np.array([[0.0, 0.0, 20.0], [4.0, 1.0, 21.0], [7.0, 5.0, 19.5]])
    else:
        raise KeyError(kind)
    return c


def camera_path(kind, noisy):
    """cam_R [n][9], cam_c [n][3], gps [n][3] = the planted similarity of the centres (+ GPS_NOISE when noisy)."""
    seed = {"lawn60": 11, "line5": 12, "tri3": 13}[kind]
    rng = np.random.default_rng(seed)
    c = path_centres(kind) + rng.normal(0, 0.05, path_centres(kind).shape)
    n = len(c)
    down = rodrigues([np.pi, 0.0, 0.0])              # looking down
    R = np.array([(rodrigues(rng.normal(0, 0.15, 3)) @ down).reshape(9) for _ in range(n)])
    Rp = rodrigues(PLANTED_AA)
    gps = PLANTED_SCALE * c @ Rp.T + PLANTED_T
    if noisy:
        gps = gps + np.random.default_rng(seed + 100).normal(0, GPS_NOISE, gps.shape)
    return dict(cam_R=R, cam_c=c, gps=gps, Rp=Rp)


PATHS = [(k, noisy) for k in ("lawn60", "line5", "tri3") for noisy in (False, True)]


def _project(R, t, fk, dc, X):
    pc = R.reshape(3, 3) @ X + t
    x, y = pc[0] / pc[2], pc[1] / pc[2]
    r2 = x * x + y * y
    d = 1.0 + r2 * (fk[1] + fk[2] * r2)
    return np.array([fk[0] * d * x + dc[0], fk[0] * d * y + dc[1]])


def _cameras(rng, n, away=()):
    """n cameras on a line looking along +z (those in `away` along -z: every point has non-positive depth in them)."""
    c = np.column_stack([np.arange(n) * 2.0, rng.normal(0, 0.3, n), rng.normal(0, 0.3, n)])
    R = np.array([rodrigues(rng.normal(0, 0.03, 3)) for _ in range(n)])
    for a in away:
        R[a] = R[a] @ rodrigues([np.pi, 0.0, 0.0])
    t = np.array([-R[i] @ c[i] for i in range(n)])
    fk = np.column_stack([rng.uniform(900, 1100, n), rng.uniform(-0.05, 0.05, n), rng.uniform(-0.01, 0.01, n)])
    gps = c + np.array([1.5, -0.8, 0.4]) + 0.5 * np.sin(np.arange(n) / 3.0)[:, None] + rng.normal(0, 0.2, (n, 3))
    return R.reshape(n, 9), t, c, fk, gps


def _radius(rng, j):
    """Displacement radius of track j's observations: e_avg is about its square - both sides of th_outlier = 3.0, some close."""
    return [0.6, 2.6, 1.1, 3.5, 1.70, 1.76][j % 6] * rng.uniform(0.97, 1.03)


def _fill(rng, lengths, cams_of, n_cams, R, t, fk, dc, behind, ok0):
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    cam = np.zeros(off[-1], np.int32)
    xy = np.zeros((off[-1], 2))
    X = np.zeros((len(lengths), 3))
    for j, L in enumerate(lengths):
        X[j] = [rng.uniform(0, 2.0 * (n_cams - 1)), rng.uniform(-15, 15), rng.uniform(40, 80)]
        if j in behind:
            X[j, 2] = -X[j, 2]
        cs = cams_of(j, L)
        r = _radius(rng, j)
        for k, c in enumerate(cs):
            cam[off[j] + k] = c
            a = rng.uniform(0, 2 * np.pi)
            xy[off[j] + k] = _project(R[c], t[c], fk[c], dc[c], X[j]) + r * rng.uniform(0.8, 1.2) * np.array([np.cos(a), np.sin(a)])
    ok = np.ones(len(lengths), np.uint8)
    ok[list(ok0)] = 0
    return off, cam, xy, X, ok


def track_set(kind):
    """dict(tracks=A.TrackArrays, X, ok_in, cam_dc or None, gps, min_views)."""
    if kind == "A":
        # 6 cameras (camera 5 looks the other way), 48 tracks of 1 .. 6 rows; with dcx / dcy
        rng = np.random.default_rng(21)
        n = 6
        R, t, c, fk, gps = _cameras(rng, n, away=(5,))
        dc = rng.uniform(-4, 4, (n, 2))
        lengths = [1 + (j % 6) for j in range(48)]

        def cams_of(j, L):
            if j == 8:      # 3 rows, exactly two of positive depth
                return [0, 1, 5]
            if L == 6:
                return list(range(6))
            return sorted(rng.choice(5, L, replace=False))   # (camera 5 only where asked for)
        off, cam, xy, X, ok = _fill(rng, lengths, cams_of, n, R, t, fk, dc, behind={21}, ok0={9, 22, 35})
        assert lengths[8] == 3 and lengths[21] == 4
        return dict(tracks=A.TrackArrays(off, cam, xy, R, t, c, fk), X=X, ok_in=ok, cam_dc=dc, gps=gps, min_views=3)
    if kind == "B":
        # 70 cameras, 300 tracks; lengths 1, 2, 3, 4, 5, 63, 64, 65, 70 among them, an empty track, and the 70-row track on the
        # last row of a 256-row slice, so that it runs past the LDS window of its workgroup; no dcx / dcy
        rng = np.random.default_rng(22)
        n = 70
        R, t, c, fk, gps = _cameras(rng, n)
        lengths = [1, 2, 3, 4, 5, 63, 64, 65] + [int(v) for v in rng.integers(3, 13, 40)]
        pad = (SLICE_ROWS - 1 - sum(lengths)) % SLICE_ROWS
        lengths += [3] * (pad // 3 - 1) + [3 + pad % 3] + [70, 0]
        assert sum(lengths[:-2]) % SLICE_ROWS == SLICE_ROWS - 1
        lengths += [int(v) for v in rng.integers(3, 13, 300 - len(lengths))]
        i70, i0 = lengths.index(70), lengths.index(0)
        if sum(lengths) % 64 == 0:
            lengths[-1] += 1

        def cams_of(j, L):
            return sorted(rng.choice(n, L, replace=False))
        behind = set(range(61, 300, 41)) - {i70, i0}
        off, cam, xy, X, ok = _fill(rng, lengths, cams_of, n, R, t, fk, np.zeros((n, 2)), behind=behind, ok0={i0, 77, 150, 223})
        assert len(lengths) == 300 and off[-1] % 64 != 0 and off[-1] % 256 != 0
        return dict(tracks=A.TrackArrays(off, cam, xy, R, t, c, fk), X=X, ok_in=ok, cam_dc=None, gps=gps, min_views=3)
    raise KeyError(kind)
