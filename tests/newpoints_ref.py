"""Loader of tests/newpoints_ref.cpp, the sequential restatement of IncrementalSfM::GenerateNew3DPoints
(sfm_incremental.cc:755-915): the dict `Context.new_points` returns (without h2d_bytes), plus the per-candidate values the
margins of tests/test_newpoints_ref.py are asserted on."""
import ctypes as C
import os
import subprocess

import numpy as np

from metricsfm_amd import _abi as A

HERE = os.path.dirname(os.path.abspath(__file__))
POINT_KEYS = ("cam2", "feat1", "feat2", "vis_entry", "pt_match", "X", "mse", "takes1", "takes2")
ENTRY_KEYS = ("n_matches", "large", "n_candidates", "n_accepted")
FETCHED = ("pt_off",) + POINT_KEYS + ENTRY_KEYS
DEFAULTS = dict(th_mse_reprojection=3.0, th_angle_small=3.0 / 180.0 * 3.1415, th_angle_large=5.0 / 180.0 * 3.1415, th_matches_large=500)


def build_ref(tmpdir):
    so = os.path.join(str(tmpdir), "newpoints_ref.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "newpoints_ref.cpp")])
    L = C.CDLL(so)
    dp, ip, up, fp = A.c_double_p, A.c_int_p, A.c_u8_p, A.c_float_p
    L.nr_new_points.argtypes = [C.c_int, ip, ip, ip, ip, fp, C.c_int, ip, ip, dp, dp, dp, dp, C.c_int, ip, ip, ip, C.c_double, C.c_double, C.c_double,
                                C.c_int, ip, ip, ip, ip, ip, ip, dp, dp, up, up, ip, up, ip, ip, ip, ip, dp, dp, dp]
    return L


def new_points(L, n_features, pairs, match_off, matches, keypoints, cam_img, feat_point, cam_R, cam_t, cam_c, cam_fk, new_cam, vis_off, vis_cam,
               diagnostics=False, **opts):
    o = dict(DEFAULTS)
    for k in opts:
        if k not in o:
            raise AttributeError(k)
    o.update(opts)
    i32 = lambda x, shape=(-1,): np.ascontiguousarray(np.asarray(x, dtype=np.int32).reshape(shape))
    f64 = lambda x, shape: np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(shape))
    nf = i32(n_features)
    fo = np.ascontiguousarray(np.concatenate([[0], np.cumsum(nf)]), dtype=np.int32)
    pr, mo, m = i32(pairs, (-1, 2)), i32(match_off), i32(matches, (-1, 2))
    kp = np.ascontiguousarray(np.asarray(keypoints, dtype=np.float32).reshape(-1, 2))
    assert len(kp) == fo[-1]
    ci, fpt, nc_, vo, vc = i32(cam_img), i32(feat_point), i32(new_cam), i32(vis_off), i32(vis_cam)
    assert len(fpt) == int(nf[ci].sum()) and len(vo) == len(nc_) + 1
    R, t, c, fk = f64(cam_R, (-1, 9)), f64(cam_t, (-1, 3)), f64(cam_c, (-1, 3)), f64(cam_fk, (-1, 3))
    nn, ne = len(nc_), int(vo[-1])
    # capacity of the walk
    img_new = ci[nc_] if nn else np.zeros(0, np.int32)
    count = {(int(a), int(b)): int(mo[p + 1] - mo[p]) for p, (a, b) in enumerate(pr)}
    cap = 0
    for k in range(nn):
        for q in range(vo[k], vo[k + 1]):
            if vc[q] != nc_[k]:
                cap += count.get((int(img_new[k]), int(ci[vc[q]])), 0)
    cp, ce = max(1, cap), max(1, ne)
    out = dict(pt_off=np.zeros(nn + 1, np.int32), cam2=np.zeros(cp, np.int32), feat1=np.zeros(cp, np.int32), feat2=np.zeros(cp, np.int32),
               vis_entry=np.zeros(cp, np.int32), pt_match=np.zeros(cp, np.int32), X=np.zeros((cp, 3)), mse=np.zeros(cp),
               takes1=np.zeros(cp, np.uint8), takes2=np.zeros(cp, np.uint8), n_matches=np.zeros(ce, np.int32), large=np.zeros(ce, np.uint8),
               n_candidates=np.zeros(ce, np.int32), n_accepted=np.zeros(ce, np.int32))
    nd = np.zeros(1, np.int32)
    dstate, drmse, dcos, dcmin = np.zeros(cp, np.int32), np.zeros(cp), np.zeros(cp), np.zeros(cp)
    dp, ip, up = A.c_double_p, A.c_int_p, A.c_u8_p
    rc = L.nr_new_points(len(pr), A.ptr(pr, ip), A.ptr(mo, ip), A.ptr(m, ip), A.ptr(fo, ip), A.ptr(kp, A.c_float_p), len(ci), A.ptr(ci, ip),
                         A.ptr(fpt, ip), A.ptr(R, dp), A.ptr(t, dp), A.ptr(c, dp), A.ptr(fk, dp), nn, A.ptr(nc_, ip), A.ptr(vo, ip), A.ptr(vc, ip),
                         o["th_mse_reprojection"], o["th_angle_small"], o["th_angle_large"], o["th_matches_large"],
                         A.ptr(out["pt_off"], ip), A.ptr(out["cam2"], ip), A.ptr(out["feat1"], ip), A.ptr(out["feat2"], ip),
                         A.ptr(out["vis_entry"], ip), A.ptr(out["pt_match"], ip), A.ptr(out["X"], dp), A.ptr(out["mse"], dp),
                         A.ptr(out["takes1"], up), A.ptr(out["takes2"], up), A.ptr(out["n_matches"], ip), A.ptr(out["large"], up),
                         A.ptr(out["n_candidates"], ip), A.ptr(out["n_accepted"], ip), A.ptr(nd, ip), A.ptr(dstate, ip), A.ptr(drmse, dp),
                         A.ptr(dcos, dp), A.ptr(dcmin, dp))
    assert rc == 0
    npt = int(out["pt_off"][nn])
    for k in POINT_KEYS:
        out[k] = out[k][:npt]
    for k in ENTRY_KEYS:
        out[k] = out[k][:ne]
    if diagnostics:
        n = int(nd[0])
        out["diag"] = dict(state=dstate[:n], rmse=drmse[:n], cos=dcos[:n], cos_min=dcmin[:n])
    return out
