"""The host mirror's IncrementalSfM::AdjustRound (host/objectsfm.cc; reference sfm_incremental.cc:172-186) against its own
PartialBundleAdjustment -> RemovePointOutliers on a copy of the model (inside tests/round_host_check.cc, which fails when the
accept / reject sequence, the iteration count, the costs to rtol 1e-11, the parameters to 1e-9 or the bad flags disagree - the
tolerances tests/test_window.py::test_compact_window_hand_over_gives_the_same_solution sets - and, since both paths hand the
solver the same compact problem and come out bitwise equal, when the costs and parameters are not identical) and against the Python host: both
make the same library call, so what AdjustRound writes back must be what Context.round_adjust returns."""
import subprocess

import numpy as np
import pytest

from tests import round_data as D

pytestmark = pytest.mark.gpu


def test_adjust_round_matches_the_object_graph_path_and_the_python_host(tmp_path, ctx):
    c = D.main_case()
    exe, src, dst = tmp_path / "round_host_check", tmp_path / "in.bin", tmp_path / "out.bin"
    subprocess.check_call(D.host_check_command(exe))
    D.write_model(src, c)
    run = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True, timeout=300)
    print(run.stdout)
    assert run.returncode == 0 and "round_host_check ok" in run.stdout, run.stdout + run.stderr
    assert "worst parameter difference 0," in run.stdout and "solve bitwise equal: yes" in run.stdout
    got = D.read_host_result(dst, c)
    store = ctx.match_store(*D.store_args(c))
    try:
        r = ctx.round_adjust(store, *D.call_args(c), pt_new_added=c["pt_new_added"], new_cam=c["new_cam"], visible=c["visible"],
                             keypoints=c["keypoints"], partial=True, full=False, outliers=True)
    finally:
        store.close()
    for k in ("cam_pose", "cam_model", "point_xyz", "pt_mse", "pt_bad", "pt_mutable", "pt_new_added"):
        np.testing.assert_array_equal(got[k], r[k], err_msg=k)
    assert got["counts"].tolist() == [r["count_outliers"], r["count_new_add"], r["count_outliers_new_add"]]
    assert got["adjust"][:, 0].tolist() == r["adjust_cams"].tolist() and got["adjust"][:, 1].tolist() == r["adjust_pts"].tolist()
    assert got["solved"].tolist() == [1, 0] and r["count_outliers"] > 0
