"""The host mirror's RelativePoseEstimation::RelativePoseWithoutFocalLength and its batch form (host/objectsfm.cc; reference
relative_pose_estimation.cc:29-83) against the Python host: both drive msfm_relpose_8pt_batch with the reference's 200 samples and
the same seed, so every number must agree bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from tests import relposef_data as D

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_SEED = 0x4D53464D50     # kPoseSeed of host/objectsfm.cc


def test_host_mirror_matches_the_python_host(tmp_path, ctx):
    lib = os.path.join(ROOT, "metricsfm_amd")
    exe = tmp_path / "relposef_host_check"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "host"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "relposef_host_check.cc"), os.path.join(ROOT, "host", "objectsfm.cc"), "-o", str(exe),
                           "-L" + lib, "-lmsfm", "-Wl,-rpath," + lib, "-Wl,-rpath-link,/opt/rocm/lib"])
    sizes = [150, 7, 0, 12, 400, 80]
    off, a, b = D.make_mixed_batch(61, sizes)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as fh:
        np.array([len(sizes)] + sizes, np.int32).tofile(fh)
        for p in range(len(sizes)):
            np.ascontiguousarray(a[off[p]:off[p + 1]]).tofile(fh)
            np.ascontiguousarray(b[off[p]:off[p + 1]]).tofile(fh)
    run = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "relposef_host_check ok" in run.stdout, run.stdout + run.stderr
    raw = np.fromfile(dst, dtype=np.float64).reshape(2, len(sizes), 15)
    _, f1, f2, _, R, t, ok, _, _, _ = ctx.relpose_8pt(off, a, b, ransac_times=200, seed=HOST_SEED)
    assert ok.any() and not ok.all()
    for p in range(len(sizes)):
        rec = raw[0, p]
        assert rec[0] == ok[p]
        np.testing.assert_array_equal(rec[1], f1[p])
        np.testing.assert_array_equal(rec[2], f2[p])
        np.testing.assert_array_equal(rec[3:12].reshape(3, 3), R[p])
        np.testing.assert_array_equal(rec[12:15], t[p])
        # the single form is a batch of one: pair index 0
        s = slice(off[p], off[p + 1])
        _, g1, g2, _, Rs, ts, oks, _, _, _ = ctx.relpose_8pt([0, off[p + 1] - off[p]], a[s], b[s], ransac_times=200, seed=HOST_SEED)
        rec = raw[1, p]
        assert rec[0] == oks[0]
        if oks[0]:
            np.testing.assert_array_equal(rec[1], g1[0])
            np.testing.assert_array_equal(rec[2], g2[0])
            np.testing.assert_array_equal(rec[3:12].reshape(3, 3), Rs[0])
            np.testing.assert_array_equal(rec[12:15], ts[0])
        else:
            assert (rec[1:] == -1.0).all()
