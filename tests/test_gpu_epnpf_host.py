"""The host mirror's AbsolutePoseWithoutFocalLengthBatch (host/objectsfm.cc; reference absolute_pose_estimation.cc:28-40) against the
Python host: both drive msfm_epnpf_sweep_batch with the reference's options and the same seed, so every number must agree bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from tests.twoview import make_pnp_batch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_mirror_matches_the_python_host(tmp_path, ctx):
    lib = os.path.join(ROOT, "metricsfm_amd")
    exe = tmp_path / "epnpf_host_check"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "host"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "epnpf_host_check.cc"), os.path.join(ROOT, "host", "objectsfm.cc"), "-o", str(exe),
                           "-L" + lib, "-lmsfm", "-Wl,-rpath," + lib, "-Wl,-rpath-link,/opt/rocm/lib"])
    sizes = [150, 3, 0, 40]
    off, X, x, _, _ = make_pnp_batch(51, sizes, outlier_frac=0.1)
    f_est = np.array([5760.0, 4000.0, 4000.0, 3600.0])
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as fh:
        np.array([len(sizes)] + sizes, np.int32).tofile(fh)
        for p in range(len(sizes)):
            f_est[p:p + 1].tofile(fh)
            np.ascontiguousarray(X[off[p]:off[p + 1]]).tofile(fh)
            np.ascontiguousarray(x[off[p]:off[p + 1]]).tofile(fh)
    run = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "epnpf_host_check ok" in run.stdout, run.stdout + run.stderr
    f, R, t, err, avg, _, _ = ctx.epnpf_sweep(off, X, x, f_est)
    raw = np.fromfile(dst, dtype=np.float64)
    assert len(raw) == 14 * len(sizes) + off[-1]
    pos = 0
    for p, n in enumerate(sizes):
        rec = raw[pos:pos + 14 + n]
        pos += 14 + n
        np.testing.assert_array_equal(rec[0], f[p])
        np.testing.assert_array_equal(rec[1:10].reshape(3, 3), R[p])
        np.testing.assert_array_equal(rec[10:13], t[p])
        np.testing.assert_array_equal(rec[13], avg[p])
        np.testing.assert_array_equal(rec[14:], err[off[p]:off[p + 1]])
