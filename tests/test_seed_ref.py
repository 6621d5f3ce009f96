"""The CPU side of the seed-pair hypotheses (no GPU): sort_image_pairs against the literal loop of SortImagePairs, and the
sequential restatement tests/seed_ref.cpp against the truth of a noise-free pair, against oracle.triangulate_midpoint on the same
two-view tracks, and on the gate edge cases the GPU test then repeats through the library."""
import numpy as np
import pytest

from metricsfm_amd import _abi as A
from metricsfm_amd import seed
from tests import relposef_data as RF
from tests import seed_data as D
from tests import seed_ref as SR


@pytest.fixture(scope="module")
def refs(tmp_path_factory, oracle):
    d = tmp_path_factory.mktemp("seed_ref")
    return oracle, RF.build_ref(d), SR.build_ref(d)


def test_sort_image_pairs_is_the_literal_loop():
    """Two ties that std::sort leaves open: the pairs (7, 8) and (9, 10) have the same match count and equal rows, so equal
    non-zero strengths; the pairs (1, 2) and (3, 4) have n_ij = 1, so strength log(1) = 0 whatever their rows.  Image 5 is
    processed, image 6 matches nothing."""
    g = np.zeros((11, 11), np.int32)
    for i, j in ((0, 1), (0, 2), (1, 3), (2, 3)):
        g[i, j] = g[j, i] = 50
    g[1, 2] = g[2, 1] = 1
    g[3, 4] = g[4, 3] = 1
    g[0, 4] = g[4, 0] = 1234567
    g[2, 5] = g[5, 2] = 900
    g[1, 4] = 7                                            # the upper triangle alone is read for n_ij; the row sums see both
    g[7, 8] = g[8, 7] = g[9, 10] = g[10, 9] = 40
    processed = [False] * 5 + [True] + [False] * 5
    got = seed.sort_image_pairs(g, processed)
    want = SR.sort_image_pairs_loop(g, processed)
    assert got.dtype == np.int32 and got.tolist() == [list(p) for p in want]
    assert len(want) == 10 and want[0] == (0, 4)
    assert want[-2:] == [(1, 2), (3, 4)]                   # strength 0 twice: the lower i * n + j first
    assert want.index((9, 10)) == want.index((7, 8)) + 1   # equal strengths: the lower i * n + j first
    assert all(5 not in p and 6 not in p for p in want)
    assert seed.sort_image_pairs(np.zeros((3, 3), np.int32), [False] * 3).shape == (0, 2)


def test_noise_free_pair_is_recovered(refs):
    """An unrotated second camera is recovered with its points (up to the free scale; the keypoints are binary32, 2e-8
    relative).  A rotated one (0.05 rad per axis, as tests/twoview.py makes them) shows the reference's convention: the t the
    estimator returns is R^T t of the true pose, and :334 uses it as the translation - the reprojection gate then fails."""
    O, L8, LS = refs
    c = D.build_case([dict(n=200, f=(D.F, D.F), kw=dict(rot=0.0, **D.EXACT)), dict(n=200, f=(D.F, D.F), kw=dict(rot=0.05, **D.EXACT))], 21)
    r = D.expected(O, L8, LS, c)
    R, t, X = c["truth"][0]
    assert r["arm"].tolist() == [5, 5] and r["pose_ok"].tolist() == [1, 1] and r["pass"][0] == 1 and r["winner"] == 0
    assert r["n_matches"][0] == 200 and r["pt_off"][:2].tolist() == [0, 200] and r["pt_match"][:200].tolist() == list(range(200))
    scale = np.linalg.norm(t) / np.linalg.norm(r["t"][0])
    np.testing.assert_allclose(r["R"][0], np.eye(3), atol=1e-6)
    np.testing.assert_allclose(r["t"][0] * scale, t, atol=1e-4)
    np.testing.assert_allclose(r["c"][0] * scale, -t, atol=1e-4)
    np.testing.assert_allclose(r["X"][:200] * scale, X, rtol=1e-4)
    assert r["mse"][:200].max() < 1e-6
    R, t, _ = c["truth"][1]
    np.testing.assert_allclose(r["R"][1], R, atol=1e-6)
    np.testing.assert_allclose(r["t"][1] * np.linalg.norm(t), R.T @ t, atol=1e-4)
    Re, te = r["R"][1].tolist(), r["t"][1].tolist()
    assert r["c"][1].tolist() == [-(Re[0][k] * te[0] + Re[1][k] * te[1] + Re[2][k] * te[2]) for k in range(3)]   # Camera::SetRTPose
    assert r["pass"][1] == 0 and r["pt_off"][2] - r["pt_off"][1] < 20


def test_points_agree_with_the_triangulation_oracle(refs):
    """X / mse of the restatement (built without fused multiply-adds) against oracle.triangulate_midpoint on the same two-view
    tracks, within tests/test_gpu_tri.py's tolerances; the accepted set is the oracle's ok."""
    O, L8, LS = refs
    c = D.build_case([D.MIXED[9], D.MIXED[11], D.MIXED[4]], 22)
    r = D.expected(O, L8, LS, c)
    assert r["pose_ok"].tolist() == [1, 1, 1] and np.diff(r["pt_off"]).min() > 5
    args, th, tm = D.two_view_tracks(c, r)
    Xo, mo, oko = O.triangulate_midpoint(A.TrackArrays(*args), D.OPTS["th_mse_reprojection"], D.OPTS["th_angle_small"])
    keep = oko == 1
    np.testing.assert_array_equal(np.bincount(th[keep], minlength=3), np.diff(r["pt_off"]))
    np.testing.assert_array_equal(tm[keep], r["pt_match"])
    np.testing.assert_allclose(r["X"], Xo[keep], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(r["mse"], mo[keep], rtol=1e-7, atol=1e-9)


def test_gate_edge_cases(refs):
    O, L8, LS = refs
    c = D.build_case(D.GATES, 23)
    r = D.expected(O, L8, LS, c)
    assert r["pose_ok"].tolist() == [1] * 5
    assert np.diff(r["pt_off"]).tolist() == D.GATES_POINTS
    assert r["pass"].tolist() == D.GATES_PASS and r["winner"] == 2
    assert r["n_matches"].tolist() == [100, 29, 30, 150, 129]
    # only failing hypotheses: no winner; the first failing, the second passing: the second
    none = D.expected(O, L8, LS, c, c["hyp_img"][[0, 1, 3]], c["cam_fk"][[0, 1, 3]], c["same_model"][[0, 1, 3]])
    assert none["winner"] == -1 and none["pass"].tolist() == [0, 0, 0]
    # a failed pose (4 matches) and an absent pair: no points, no pass
    m = D.build_case(D.MIXED[:3], 24)
    rm = D.expected(O, L8, LS, m)
    assert rm["n_matches"].tolist() == [0, 4, 5] and rm["pose_ok"][:2].tolist() == [0, 0] and rm["pt_off"][:3].tolist() == [0, 0, 0]
    assert not rm["R"][:2].any() and rm["f"][:2].tolist() == [[D.F, D.F]] * 2
