"""Loader of tests/gpsreg_ref.cpp, the sequential restatement of AbsoluteOrientationWithGPSGlobal, GetAccuracy and
GPSRegistration2 (slam_gps.cc:1596-1674, :1573-1594, :917-983): each function returns what its `capi` counterpart returns."""
import ctypes as C
import os
import subprocess

import numpy as np

from metricsfm_amd import _abi as A

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULTS = dict(window=20, min_views=3, clip_deg=80.0, th_outlier=3.0)


def build_ref(tmpdir):
    so = os.path.join(str(tmpdir), "gpsreg_ref.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "gpsreg_ref.cpp")])
    L = C.CDLL(so)
    dp, ip, up, i, d = A.c_double_p, A.c_int_p, A.c_u8_p, C.c_int, C.c_double
    L.gr_svd3.argtypes = [dp, dp, dp, dp]
    L.gr_svd3.restype = None
    L.gr_similarity.argtypes = [i, dp, dp, dp, dp, dp, dp, dp]
    L.gr_orient_global.argtypes = [i, i, d, dp, dp, dp, dp, dp, dp, dp, dp, dp, dp, dp]
    L.gr_accuracy.argtypes = [i, ip, ip, dp, dp, dp, dp, dp, dp, up, i, d, dp, dp, ip, up, ip, ip]
    L.gr_accuracy.restype = None
    L.gr_register_points.argtypes = [i, ip, ip, up, i, dp, dp, dp]
    L.gr_register_points.restype = None
    return L


def _f64(x, shape):
    return np.array(np.asarray(x, dtype=np.float64).reshape(shape), order="C")


def svd3(L, M):
    M = _f64(M, 9)
    U, S, V = np.zeros(9), np.zeros(3), np.zeros(9)
    L.gr_svd3(A.ptr(M, A.c_double_p), A.ptr(U, A.c_double_p), A.ptr(S, A.c_double_p), A.ptr(V, A.c_double_p))
    return U.reshape(3, 3), S, V.reshape(3, 3)


def orient_global(L, cam_R, cam_c, gps, window=DEFAULTS["window"], clip_deg=DEFAULTS["clip_deg"]):
    R, c, g = _f64(cam_R, (-1, 9)), _f64(cam_c, (-1, 3)), _f64(gps, (-1, 3))
    n = len(c)
    out = dict(cam_R=R, cam_t=np.zeros((n, 3)), cam_c=c, cam_aa=np.zeros((n, 3)), gps=g, weight=np.zeros(n))
    Rg, tg, off, scale, err = np.zeros(9), np.zeros(3), np.zeros(3), C.c_double(), C.c_double()
    dp = A.c_double_p
    ok = L.gr_orient_global(n, window, clip_deg, A.ptr(R, dp), A.ptr(out["cam_t"], dp), A.ptr(c, dp), A.ptr(out["cam_aa"], dp), A.ptr(g, dp),
                            A.ptr(out["weight"], dp), A.ptr(Rg, dp), A.ptr(tg, dp), C.cast(C.byref(scale), dp), C.cast(C.byref(err), dp), A.ptr(off, dp))
    assert ok == 1
    out.update(Rg=Rg.reshape(3, 3), tg=tg, scale=scale.value, err=err.value, offset=off)
    return out


def point_accuracy(L, tracks, X, ok_in, cam_dc=None, min_views=DEFAULTS["min_views"], th_outlier=DEFAULTS["th_outlier"]):
    """`tracks` is an A.TrackArrays; returns e_avg, e_mse, n_used, ok_out, n_outliers, n_inliers."""
    n = tracks.struct.n_tracks
    X, ok_in = _f64(X, (-1, 3)), np.ascontiguousarray(ok_in, dtype=np.uint8)
    dc = None if cam_dc is None else _f64(cam_dc, (-1, 2))
    e_avg, e_mse, n_used, ok = np.zeros(n), np.zeros(n), np.zeros(n, np.int32), np.zeros(n, np.uint8)
    n_out, n_in = np.zeros(1, np.int32), np.zeros(1, np.int32)
    dp, ip, up = A.c_double_p, A.c_int_p, A.c_u8_p
    L.gr_accuracy(n, A.ptr(tracks.track_off, ip), A.ptr(tracks.track_cam, ip), A.ptr(tracks.track_xy, dp), A.ptr(tracks.cam_R, dp),
                  A.ptr(tracks.cam_t, dp), A.ptr(tracks.cam_fk, dp), A.ptr(dc, dp), A.ptr(X, dp), A.ptr(ok_in, up), min_views, th_outlier,
                  A.ptr(e_avg, dp), A.ptr(e_mse, dp), A.ptr(n_used, ip), A.ptr(ok, up), A.ptr(n_out, ip), A.ptr(n_in, ip))
    return e_avg, e_mse, n_used, ok, int(n_out[0]), int(n_in[0])


def register_points(L, track_off, track_cam, ok, cam_c, gps, X):
    off, cam = np.ascontiguousarray(track_off, dtype=np.int32), np.ascontiguousarray(track_cam, dtype=np.int32)
    ok, c, g, X = np.ascontiguousarray(ok, dtype=np.uint8), _f64(cam_c, (-1, 3)), _f64(gps, (-1, 3)), _f64(X, (-1, 3))
    L.gr_register_points(len(off) - 1, A.ptr(off, A.c_int_p), A.ptr(cam, A.c_int_p), A.ptr(ok, A.c_u8_p), len(c), A.ptr(c, A.c_double_p),
                         A.ptr(g, A.c_double_p), A.ptr(X, A.c_double_p))
    return X
