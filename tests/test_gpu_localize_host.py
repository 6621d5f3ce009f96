"""The host mirror's IncrementalSfM::FindImageToLocalize (host/objectsfm.cc; reference sfm_incremental.cc:417-563) against the Python
host (metricsfm_amd/localize.py) on the ring round: both gather the same flat state and make the same library call, so every
list must be equal.  The driver also runs the mirror's std::map walk and fails when it disagrees with the library."""
import subprocess

import numpy as np
import pytest

from metricsfm_amd import localize
from tests import localize_data as D

pytestmark = pytest.mark.gpu


def test_host_mirror_matches_the_python_host(tmp_path, ctx):
    exe = tmp_path / "localize_host_check"
    subprocess.check_call(D.host_check_command(exe))
    c = D.ring_round()
    n = len(c["n_features"])
    fail = np.zeros(n, np.int32)
    fail[c["cand_img"]] = c["fail_times"]
    fail[9] = 5                                        # th_max_failure_localization reached: image 9 is no candidate any more
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    D.write_round(src, c, fail)
    run = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "localize_host_check ok" in run.stdout, run.stdout + run.stderr
    ids_c, corres_c, visible_c = D.read_round_result(dst)
    st = ctx.match_store(*D.store_args(c))
    match_count = np.zeros((n, n), np.int32)
    match_count[c["pairs"][:, 0], c["pairs"][:, 1]] = np.diff(c["match_off"])
    ids, corres, visible = localize.find_images_to_localize(ctx, st, match_count, c["cam_img"], c["feat_point"], c["pt_bad"], c["pt_mse"],
                                                            c["pt_views"], fail)
    st.close()
    assert ids_c == ids and sorted(ids) == [6, 7, 8]
    for a, b in zip(corres_c, corres):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(visible_c, visible):
        np.testing.assert_array_equal(a, b)
