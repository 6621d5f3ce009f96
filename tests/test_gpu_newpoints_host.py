"""The host mirror's IncrementalSfM::GenerateNew3DPoints (host/objectsfm.cc; reference sfm_incremental.cc:755-915) against its
own per-candidate walk (inside tests/newpoints_host_check.cc, which fails when they disagree) and against the Python host
metricsfm_amd/newpoints.py: both make the same library call, so the points, their order and the feat_point table afterwards
must be identical."""
import subprocess

import numpy as np
import pytest

from metricsfm_amd import newpoints
from tests import newpoints_data as D
from tests.newpoints_data import SEED_CLAIMS, SEED_WALK

pytestmark = pytest.mark.gpu
IDX_MAX = 1000000   # IncrementalSfMOptions::idx_max_per_image


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("newpoints_host") / "newpoints_host_check"
    subprocess.check_call(D.host_check_command(path))
    return path


@pytest.mark.parametrize("which", ["walk", "claims"])
def test_host_mirror_matches_its_walk_and_the_python_host(tmp_path, ctx, exe, which):
    c = D.newest_last(D.sub(D.walk_case(SEED_WALK), [0]) if which == "walk" else D.claims_case(SEED_CLAIMS))
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    D.write_model(src, c)
    run = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "newpoints_host_check ok" in run.stdout, run.stdout + run.stderr
    got = D.read_host_result(dst, c)
    st = ctx.match_store(*D.store_args(c))
    state = dict(n_features=c["n_features"], cam_img=c["cam_img"], feat_point=c["feat_point"].copy(), cam_R=c["cam_R"], cam_t=c["cam_t"],
                 cam_c=c["cam_c"], cam_fk=c["cam_fk"], point_xyz=np.zeros((D.N_POINTS, 3)), pt_bad=np.zeros(D.N_POINTS, np.uint8),
                 pt_mse=np.zeros(D.N_POINTS), pt_views=np.full(D.N_POINTS, 3, np.int32))
    c1 = int(c["new_cam"][0])
    r = newpoints.generate_new_points(ctx, st, state, c1, c["vis_cam"], keypoints=c["keypoints"])
    st.close()
    newpoints.apply_new_points(state, r)
    assert len(r.mse) > 30
    np.testing.assert_array_equal(got["global1"], r.feat1 + int(c["cam_img"][c1]) * IDX_MAX)
    np.testing.assert_array_equal(got["global2"], r.feat2 + c["cam_img"][r.cam2] * IDX_MAX)
    np.testing.assert_array_equal(got["cam2"], r.cam2)
    np.testing.assert_array_equal(got["takes1"], r.takes1)
    np.testing.assert_array_equal(got["takes2"], r.takes2)
    np.testing.assert_array_equal(got["X"], r.X)
    np.testing.assert_array_equal(got["mse"], r.mse)
    np.testing.assert_array_equal(got["feat_point"], state["feat_point"])
