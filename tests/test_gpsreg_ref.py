"""tests/gpsreg_ref.cpp pinned independently of the library: its 3x3 Jacobi SVD against the matrices it decomposes, its
similarity transform against a planted one, its weights, accuracies and shifts against numpy, and the conditions the seeded
cases of tests/gpsreg_data.py must meet for the GPU comparison to mean something."""
import numpy as np
import pytest

from tests import gpsreg_data as D
from tests import gpsreg_ref as G


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return G.build_ref(tmp_path_factory.mktemp("gpsreg_ref"))


def _matrices():
    rng = np.random.default_rng(5)
    out = []
    for k in range(1000):
        M = rng.normal(0, 1, (3, 3)) * 10.0 ** rng.integers(-6, 7)
        kind = k % 10
        if kind == 1:      # rank 2
            M[:, 2] = 0.5 * M[:, 0] - 2.0 * M[:, 1]
        elif kind == 2:    # rank 1
            M = np.outer(rng.normal(0, 1, 3), rng.normal(0, 1, 3))
        elif kind == 3:    # a reflection
            M = D.rodrigues(rng.normal(0, 1, 3)) @ np.diag([1.0, 1.0, -1.0])
        elif kind == 4:    # diagonal already, one negative entry
            M = np.diag(rng.normal(0, 1, 3))
        elif kind == 5:    # symmetric
            M = M + M.T
        out.append(M)
    out.append(np.zeros((3, 3)))
    return out


def test_svd_reproduces_its_input(L):
    for M in _matrices():
        U, S, V = G.svd3(L, M)
        scale = max(np.abs(M).max(), np.finfo(float).tiny)
        assert np.abs(U @ np.diag(S) @ V.T - M).max() <= 1e-13 * scale
        assert np.abs(U.T @ U - np.eye(3)).max() <= 1e-14 and np.abs(V.T @ V - np.eye(3)).max() <= 1e-14
        assert S[0] >= S[1] >= S[2] >= 0.0
        if np.abs(M).max() > 0:
            np.testing.assert_allclose(S, np.linalg.svd(M, compute_uv=False), rtol=1e-12, atol=1e-13 * scale)


@pytest.mark.parametrize("kind", ["lawn60", "line5"])
def test_noise_free_planted_similarity_is_recovered(L, kind):
    """With exact data ds_i -> scale Rp ds_i for every i, so cov = scale * sum w_i ds_i ds_i^T Rp^T whatever the weights: the
    planted transform solves the reference's mixed centroid / covariance weighting too."""
    p = D.camera_path(kind, noisy=False)
    r = G.orient_global(L, p["cam_R"], p["cam_c"], p["gps"])
    assert abs(r["scale"] - D.PLANTED_SCALE) <= 1e-9 * D.PLANTED_SCALE
    assert np.abs(r["Rg"] - p["Rp"]).max() <= 1e-9
    assert np.abs(r["tg"] - D.PLANTED_T).max() <= 1e-9 * np.abs(D.PLANTED_T).max()
    assert r["err"] <= 1e-9 * np.abs(D.PLANTED_T).max()
    # the cameras land on their GPS positions, both re-centred on the offset
    np.testing.assert_allclose(r["cam_c"], r["gps"], atol=1e-9 * np.abs(D.PLANTED_T).max())
    np.testing.assert_allclose(r["offset"], p["gps"].mean(axis=0), rtol=1e-9)
    np.testing.assert_allclose(r["gps"], p["gps"] - r["offset"], rtol=0, atol=0)
    # Camera::Transformation: R' = R Rg^-1, t' = -R' c', the angle-axis vector of R'
    for i in range(len(p["cam_c"])):
        Rn = r["cam_R"][i].reshape(3, 3)
        np.testing.assert_allclose(Rn, p["cam_R"][i].reshape(3, 3) @ p["Rp"].T, atol=1e-9)
        np.testing.assert_allclose(r["cam_t"][i], -Rn @ r["cam_c"][i], rtol=0, atol=1e-9 * np.abs(r["cam_c"]).max())
        np.testing.assert_allclose(D.rodrigues(r["cam_aa"][i]), Rn, atol=1e-9)


@pytest.mark.parametrize("kind,noisy", D.PATHS)
def test_weights_against_numpy(L, kind, noisy):
    p = D.camera_path(kind, noisy)
    r = G.orient_global(L, p["cam_R"], p["cam_c"], p["gps"])
    g, n = p["gps"], len(p["gps"])
    i = np.arange(n)
    s, e = np.maximum(i - 20, 0), np.minimum(i + 20, n - 1)
    ds, de = g[s, :2] - g[:, :2], g[e, :2] - g[:, :2]
    cosv = (ds * de).sum(1) / np.sqrt((ds * ds).sum(1) + 0.1) / np.sqrt((de * de).sum(1) + 0.1)
    ang = np.minimum(np.abs(np.arccos(cosv) - np.pi), np.deg2rad(80.0))
    np.testing.assert_allclose(r["weight"], np.tan(ang), rtol=1e-9)
    if kind == "lawn60":   # from a straight leg (tan of about 0) to the clip
        assert r["weight"].min() < 0.05 and r["weight"].max() == np.tan(np.pi * 80.0 / 180.0)
    if noisy:              # the similarity still fits to the noise level
        assert r["err"] < 3.0 * D.GPS_NOISE * np.sqrt(3.0) and abs(r["scale"] - D.PLANTED_SCALE) < 0.1


def _numpy_accuracy(ts):
    T, X = ts["tracks"], ts["X"]
    n = T.struct.n_tracks
    dc = np.zeros((len(T.cam_t), 2)) if ts["cam_dc"] is None else ts["cam_dc"]
    e_avg, e_mse, used = np.full(n, 1000.0), np.zeros(n), np.zeros(n, np.int32)
    for j in range(n):
        b, e = T.track_off[j], T.track_off[j + 1]
        if not ts["ok_in"][j] or e - b < ts["min_views"]:
            continue
        cam = T.track_cam[b:e]
        pc = np.einsum("nij,j->ni", T.cam_R[cam].reshape(-1, 3, 3), X[j]) + T.cam_t[cam]
        pos = pc[:, 2] > 0
        if pos.sum() < 2:
            continue
        xy = pc[pos, :2] / pc[pos, 2:3]
        r2 = (xy * xy).sum(1)
        fk = T.cam_fk[cam[pos]]
        uv = (fk[:, 0] * (1.0 + r2 * (fk[:, 1] + fk[:, 2] * r2)))[:, None] * xy + dc[cam[pos]]
        err = ((uv - T.track_xy[b:e][pos]) ** 2).sum(1)
        e_avg[j], e_mse[j], used[j] = np.mean(err), np.std(err, ddof=1), pos.sum()
    return e_avg, e_mse, used


@pytest.mark.parametrize("kind", ["A", "B"])
def test_accuracy_and_shift_against_numpy_and_the_data_condition(L, kind):
    ts = D.track_set(kind)
    T = ts["tracks"]
    e_avg, e_mse, used, ok, n_out, n_in = G.point_accuracy(L, T, ts["X"], ts["ok_in"], ts["cam_dc"], ts["min_views"], 3.0)
    a, m, u = _numpy_accuracy(ts)
    np.testing.assert_array_equal(used, u)
    np.testing.assert_allclose(e_avg, a, rtol=1e-9)
    np.testing.assert_allclose(e_mse, m, rtol=1e-9, atol=1e-9 * a.max())
    live = (ts["ok_in"] != 0) & (np.diff(T.track_off) >= ts["min_views"])
    np.testing.assert_array_equal(ok, (live & ~(e_avg > 3.0)).astype(np.uint8))
    assert n_out == int((e_avg > 3.0).sum()) and n_in == len(e_avg) - n_out
    # the data condition: every outcome occurs
    kept, removed, none = int(ok.sum()), int(((e_avg > 3.0) & (e_avg != 1000.0)).sum()), int((e_avg == 1000.0).sum())
    assert kept >= 5 and removed >= 5 and none >= 5, (kept, removed, none)
    assert ((e_avg > 2.7) & (e_avg < 3.0)).any() and ((e_avg > 3.0) & (e_avg < 3.4)).any()     # on both sides of the threshold, close to it
    lens = np.diff(T.track_off)
    assert (live & (used == 0)).any()                                    # rows, but fewer than two of positive depth
    if kind == "A":
        assert used[8] == 2 and lens[8] == 3 and ts["ok_in"][8]          # exactly two rows of positive depth
        assert lens[21] == 4 and used[21] == 0 and ts["ok_in"][21]       # every row of non-positive depth
    assert ((lens == ts["min_views"] - 1) & (ts["ok_in"] != 0)).any() and (~(ts["ok_in"] != 0) & (lens >= 3)).any()
    if kind == "B":
        assert set([1, 2, 3, 4, 5, 63, 64, 65, 70]) <= set(lens.tolist())
        j = int(np.nonzero(lens == 70)[0][0])
        assert T.track_off[j] % D.SLICE_ROWS == D.SLICE_ROWS - 1
    # the shift of GPSRegistration2 against a vectorised weighted mean
    Xs = G.register_points(L, T.track_off, T.track_cam, ok, T.cam_c, ts["gps"], ts["X"])
    want = ts["X"].copy()
    offs = ts["gps"] - T.cam_c
    for j in np.nonzero(ok)[0]:
        cam = T.track_cam[T.track_off[j]:T.track_off[j + 1]]
        w = 1.0 / (np.sqrt(np.linalg.norm(ts["X"][j] - T.cam_c[cam], axis=1)) + 5.0)
        want[j] += (w[:, None] * offs[cam]).sum(0) / w.sum()
    np.testing.assert_allclose(Xs, want, rtol=1e-9)
    np.testing.assert_array_equal(Xs[ok == 0], ts["X"][ok == 0])
    assert np.abs(Xs[ok != 0] - ts["X"][ok != 0]).max() > 0.5
