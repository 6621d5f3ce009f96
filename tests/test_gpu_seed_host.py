"""The host mirror's IncrementalSfM::FindSeedPairThenReconstruct (host/objectsfm.cc; reference sfm_incremental.cc:224-415)
against its own one-hypothesis-at-a-time walk (inside tests/seed_host_check.cc, which fails when they disagree) and against
the Python host metricsfm_amd/seed.py::find_seed_pair: both rank with the C library's log and make the same library calls, so
the pair, the cameras and the points must be equal."""
import subprocess

import numpy as np
import pytest

from metricsfm_amd import seed
from tests import seed_data as D

pytestmark = pytest.mark.gpu
IDX_MAX = 1000000   # IncrementalSfMOptions::idx_max_per_image


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("seed_host") / "seed_host_check"
    subprocess.check_call(D.host_check_command(path))
    return path


@pytest.mark.parametrize("chunk,known_f", [(64, True), (2, True), (64, False)])
def test_host_mirror_matches_its_walk_and_the_python_host(tmp_path, ctx, exe, chunk, known_f):
    # the gates store (five-point arm), or three eight-point pairs of which the second and third reconstruct
    c = D.build_case(D.GATES, 23) if known_f else D.build_case([D.MIXED[8], D.MIXED[11], D.MIXED[10]], 31)
    nf, pairs, moff, m = D.store_args(c)
    n = len(nf)
    focal = np.full(n, D.F if known_f else 0.0)
    model = np.arange(n) // 2 if not known_f else np.arange(n)      # (unknown f: the two images of a pair share one model)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    D.write_image_set(src, c, focal, model, chunk)
    run = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "seed_host_check ok" in run.stdout, run.stdout + run.stderr
    got = D.read_seed_result(dst)
    graph = np.zeros((n, n), np.int32)
    graph[pairs[:, 0], pairs[:, 1]] = np.diff(moff)
    by_pair = {tuple(p): m[moff[k]:moff[k + 1]] for k, p in enumerate(pairs.tolist())}
    st = ctx.match_store(nf, pairs, moff, m)
    r = seed.find_seed_pair(ctx, st, graph, np.zeros(n, bool), focal, model, k=chunk, keypoints=c["keypoints"],
                            pair_matches=lambda a, b: by_pair[(a, b)])
    st.close()
    assert got["found"] and r is not None
    assert got["images"] == r["images"] and got["n_visited"] == r["n_visited"]
    np.testing.assert_array_equal(got["f"], r["cam_model"][:, 0])
    np.testing.assert_array_equal(got["R"], r["cam_R"][1])
    np.testing.assert_array_equal(got["t"], r["cam_t"][1])
    np.testing.assert_array_equal(got["c"], r["cam_c"][1])
    np.testing.assert_array_equal(got["X"], r["point"])
    np.testing.assert_array_equal(got["mse"], r["mse"])
    i1, i2 = r["images"]
    np.testing.assert_array_equal(got["global_ids"], r["obs_feature"].reshape(-1, 2) + np.array([i1, i2]) * IDX_MAX)
