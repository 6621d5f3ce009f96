"""The C++ host mirror's registration steps (SLAMGPS::AbsoluteOrientationWithGPSGlobal, GetAccuracy, GPSRegistration2 of
host/objectsfm.h): tests/gpsreg_host_check.cc compares each with the mirror's own literal walk and fails when they disagree;
what it writes is compared here with the Python host, array for array."""
import os
import subprocess

import numpy as np
import pytest

from metricsfm_amd import _abi as A
from metricsfm_amd import capi, gpsreg, scene
from tests import gpsreg_data as D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _command(exe):
    lib = os.path.join(ROOT, "metricsfm_amd")
    return ["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "host"), "-I", os.path.join(ROOT, "include"),
            os.path.join(ROOT, "tests", "gpsreg_host_check.cc"), os.path.join(ROOT, "host", "objectsfm.cc"), "-o", str(exe),
            "-L" + lib, "-lmsfm", "-Wl,-rpath," + lib, "-Wl,-rpath-link,/opt/rocm/lib"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    e = tmp_path_factory.mktemp("gpsreg_host") / "gpsreg_host_check"
    subprocess.check_call(_command(e))
    return e


@pytest.mark.parametrize("kind", ["A", "B"])
def test_mirror_equals_its_walks_and_the_python_host(ctx, exe, tmp_path, kind):
    ts = D.track_set(kind)
    T = ts["tracks"]
    n, nt, nr = len(T.cam_t), T.struct.n_tracks, int(T.track_off[-1])
    dc = np.zeros((n, 2)) if ts["cam_dc"] is None else ts["cam_dc"]
    # a GPS path for the orientation: the planted similarity of these cameras' centres, noisy
    path_gps = D.PLANTED_SCALE * T.cam_c @ D.rodrigues(D.PLANTED_AA).T + D.PLANTED_T + np.random.default_rng(4).normal(0, D.GPS_NOISE, (n, 3))
    # the mirror keeps the short tracks flagged before GetAccuracy sees them (slam_gps.cc:643)
    ok_in = (ts["ok_in"] != 0) & (np.diff(T.track_off) >= ts["min_views"])
    src, dst = tmp_path / "model.bin", tmp_path / "out.bin"
    with open(src, "wb") as fh:
        np.array([n, nt, nr], np.int32).tofile(fh)
        for a in (T.cam_R, T.cam_c, np.column_stack([T.cam_fk, dc]), ts["gps"], path_gps):
            np.ascontiguousarray(a, np.float64).tofile(fh)
        T.track_off.tofile(fh); T.track_cam.tofile(fh)
        T.track_xy.tofile(fh); np.ascontiguousarray(ts["X"], np.float64).tofile(fh)
        ok_in.astype(np.uint8).tofile(fh)
    run = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    raw = open(dst, "rb").read()
    pos = 0

    def take(dtype, *shape):
        nonlocal pos
        cnt = int(np.prod(shape)) if shape else 1
        a = np.frombuffer(raw, dtype=dtype, count=cnt, offset=pos).reshape(shape)
        pos += a.nbytes
        return a
    # the orientation against capi.gps_orient_global.  The mirror rebuilds t = -R c from R and c as it builds its cameras;
    # the orientation reads only R and c
    o = capi.gps_orient_global(T.cam_R, T.cam_c, path_gps)
    for k, shape in (("cam_R", (n, 9)), ("cam_t", (n, 3)), ("cam_c", (n, 3)), ("cam_aa", (n, 3)), ("gps", (n, 3)), ("weight", (n,)), ("Rg", (3, 3)),
                     ("tg", (3,)), ("scale", ()), ("err", ()), ("offset", (3,))):
        np.testing.assert_array_equal(take(np.float64, *shape), o[k], err_msg=k)
    # GetAccuracy / GPSRegistration2 against Context.point_accuracy / gps_register_points (min_views 0: the flags carry it)
    Rm, c = T.cam_R.reshape(-1, 3, 3), T.cam_c
    t = -(Rm[:, :, 0] * c[:, 0:1] + Rm[:, :, 1] * c[:, 1:2] + Rm[:, :, 2] * c[:, 2:3])      # in the mirror's order of operations
    tr = A.TrackArrays(T.track_off, T.track_cam, T.track_xy, T.cam_R, t, T.cam_c, T.cam_fk)
    e_avg, e_mse, used, ok, n_out, _ = ctx.point_accuracy(tr, ts["X"], ok_in.astype(np.uint8), dc, 0, 3.0)
    np.testing.assert_array_equal(take(np.float64, nt), e_avg)
    np.testing.assert_array_equal(take(np.float64, nt), e_mse)
    np.testing.assert_array_equal(take(np.int32, nt), used)
    np.testing.assert_array_equal(take(np.uint8, nt), 1 - ok)
    assert int(take(np.int32)) == n_out
    Xs = ctx.gps_register_points(T.track_off, T.track_cam, ok, T.cam_c, ts["gps"], ts["X"])
    np.testing.assert_array_equal(take(np.float64, nt, 3), Xs)
    assert np.abs(Xs - ts["X"]).max() > 0.5
    # every camera on its GPS position: the angle-axis vector stays, t = -R gps (to rounding: the mirror's R comes from its own
    # AngleAxisToRotationMatrix)
    data = take(np.float64, n, 6)
    assert pos == len(raw)
    aa = scene.R_to_angle_axis(T.cam_R.reshape(-1, 3, 3))
    _, _, pose = gpsreg.set_ac_pose(aa, ts["gps"])
    np.testing.assert_allclose(data, pose, rtol=0, atol=1e-9 * max(1.0, np.abs(pose).max()))
