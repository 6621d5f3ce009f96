"""One round of IncrementalSfM::Run (sfm_incremental.cc:126-167) - FindImageToLocalize, the localisation of the next image,
GenerateNew3DPoints - in the host mirror (host/objectsfm.cc, through tests/localizepose_host_check.cc) and in the Python host
(metricsfm_amd/localize.py + newpoints.py).  The driver itself fails unless the mirror's batched LocalizeNextImage and its
one-image-at-a-time LocalizeImage walk agree bit for bit; both hosts make the same library calls, so the camera, its
observations, the flags of every point and the new points must be identical."""
import subprocess

import numpy as np
import pytest

from metricsfm_amd import localize, newpoints
from tests import localize_data as D
from tests import localizepose_data as PD

pytestmark = pytest.mark.gpu
IDX_MAX = 1000000   # IncrementalSfMOptions::idx_max_per_image


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("localizepose_host") / "localizepose_host_check"
    subprocess.check_call(PD.host_check_command(path))
    return path


def test_one_round_in_the_mirror_its_walk_and_the_python_host(tmp_path, ctx, exe):
    h = PD.host_round()
    c = h["case"]
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    PD.write_host_round(src, h)
    run = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "localizepose_host_check ok" in run.stdout, run.stdout + run.stderr
    got = PD.read_host_round_result(dst, h)

    state = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in h["state"].items()}
    st = ctx.match_store(*D.store_args(c))
    r = localize.localize_next_image(ctx, st, state, h["match_count"], h["fail_times"], h["image_f"], h["image_f_init"], keypoints=c["keypoints"])
    assert r["image_ids"] == PD.EXPECT["images"] and r["n_calls"] == 1
    assert r["image"] == got["image"] and r["image"] in (8, 9) and list(got["failed"]) == r["failed_images"]
    assert r["failed_images"] == r["image_ids"][:r["row"]] and r["failed_images"][0] == 7      # image 7 misses the gate on either arm
    visible = localize.apply_localized_image(state, r)
    new_cam = len(state["cam_img"]) - 1
    assert visible == list(got["visible"]) and visible[0] == new_cam == 6
    assert got["f"] == r["f"] == state["cam_fk"][-1][0]
    np.testing.assert_array_equal(got["R"], state["cam_R"][-1]); np.testing.assert_array_equal(got["t"], state["cam_t"][-1])
    np.testing.assert_array_equal(got["c"], state["cam_c"][-1])
    np.testing.assert_array_equal(got["feat_row"], state["feat_point"][-len(got["feat_row"]):])
    assert (got["feat_row"] >= 0).sum() == r["n_inliers"] > 50
    for k in ("pt_bad", "pt_views", "pt_new_added"):
        np.testing.assert_array_equal(got[k], state[k], err_msg=k)
    assert state["pt_bad"].sum() > h["state"]["pt_bad"].sum()
    p = newpoints.generate_new_points(ctx, st, state, new_cam, visible, keypoints=c["keypoints"])
    st.close()
    np.testing.assert_array_equal(got["new"][:, 0], p.feat1 + r["image"] * IDX_MAX)
    np.testing.assert_array_equal(got["new"][:, 1], p.feat2 + state["cam_img"][p.cam2] * IDX_MAX)
    np.testing.assert_array_equal(got["new"][:, 2], p.cam2)
    np.testing.assert_array_equal(got["X"], p.X); np.testing.assert_array_equal(got["mse"], p.mse)
