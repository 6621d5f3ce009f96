"""The cases of tests/test_gpu_seedstart.py held to their conditions on the CPU, and the numpy forms of
metricsfm_amd/incremental.py held to the literal loops of tests/seedstart_ref.py."""
import numpy as np
import pytest

from metricsfm_amd import incremental, seed
from tests import relposef_data as RF
from tests import seed_data as D
from tests import seed_ref as SR
from tests import seedstart_data as SD
from tests import seedstart_ref as REF


@pytest.fixture(scope="module")
def refs(tmp_path_factory, oracle):
    d = tmp_path_factory.mktemp("seedstart_ref")
    return oracle, RF.build_ref(d), SR.build_ref(d)


@pytest.mark.parametrize("name", list(SD.SEED_CASES))
def test_seed_cases_win_behind_a_failing_pair(refs, name):
    c = SD.seed_case(name)
    n = len(c["n_features"])
    assert seed.sort_image_pairs(c["graph"], np.zeros(n, bool)).tolist() == c["hyp_img"].tolist()
    want = D.expected(*refs, c)
    assert want["pass"].tolist() == [0, 1] and want["winner"] == 1
    ptm = want["pt_match"][want["pt_off"][1]:]
    print(name, "points", len(ptm), "of", want["n_matches"][1], "f", want["f"][1])
    if name == "gates":
        assert len(ptm) == 20 and want["n_matches"][1] == 30     # (the rejected matches are the last ten: pt_match is 0 .. 19)
    if name == "dup":            # feature 3 of image 1 is in matches 3 and 300: both must be accepted for the case to show the insert rule
        assert want["n_matches"][1] == 301 and {3, 300} <= set(ptm.tolist()) and len(ptm) > 256
    if name == "eight":
        assert want["arm"][1] == 8 and len(ptm) > 1000 and not c["same_model"][1] and c["cam_fk"][1, :, 1:].any()
        assert ptm.tolist() != list(range(len(ptm)))             # matches in between are rejected: pt_match is not the identity
    if name == "shared":
        assert want["arm"][1] == 8 and c["same_model"][1] and want["f"][1, 0] == want["f"][1, 1] and len(ptm) > 200


@pytest.mark.parametrize("P", [63, 257, 1500])
def test_a_pairwise_sum_gives_other_bits(P):
    """The planted clouds tell the orders apart: a tree-shaped sum of the same data has another mean."""
    x = SD.planted_points(P)
    mid, scale, out = REF.normalize(x)
    assert np.isfinite(scale) and (REF.pairwise_mid(x) != mid).any()


@pytest.mark.parametrize("P", [1, 63, 257, 1500])
def test_normalize_points_is_the_loop(P):
    x = SD.planted_points(P)
    noise = np.random.default_rng(P).standard_normal((P, 3))
    for nz in (None, noise):
        mid, scale, out = REF.normalize(x, nz)
        if P == 1:               # one point: mad = 0, scale = inf, nothing is written
            assert scale == float("inf")
            with pytest.raises(incremental.capi.MsfmError) as e:
                incremental.normalize_points(x, nz)
            assert e.value.code == incremental.A.MSFM_E_NUMERIC
            continue
        g_mid, g_scale, g_out = incremental.normalize_points(x, nz)
        np.testing.assert_array_equal(g_mid, mid)
        assert g_scale == scale
        np.testing.assert_array_equal(g_out, out)


def test_state_from_seed_keeps_the_first_point_of_a_feature():
    P = 6
    feat = np.array([[0, 4], [1, 3], [0, 2], [2, 3], [1, 1], [3, 0]], np.int32)      # features 0, 1 of camera 0 and 3 of camera 1 twice
    s = dict(images=(2, 0), point=np.arange(3.0 * P).reshape(P, 3), mse=np.arange(1.0 * P), obs_pt=np.repeat(np.arange(P), 2),
             obs_cam=np.tile([0, 1], P), obs_feature=feat.reshape(-1), cam_pose=np.zeros((2, 6)), cam_model=np.array([[100.0, 1e-3, 2e-3]]),
             cam_model_of_cam=np.zeros(2, np.int32), cam_R=np.tile(np.eye(3), (2, 1, 1)), cam_t=np.zeros((2, 3)), cam_c=np.zeros((2, 3)),
             hypotheses=dict(winner=1, f=np.array([[1.0, 2.0], [100.0, 100.0]])))
    nf = np.array([6, 9, 5], np.int32)
    want = REF.state_from_seed(s, nf)
    got = incremental.state_from_seed(s, nf)
    assert want["feat_point"].tolist() == [0, 1, 3, 5, -1] + [5, 4, 2, 1, 0, -1]
    for k in ("cam_img", "feat_point", "obs_point", "obs_cam", "obs_feat", "point_xyz", "pt_bad", "pt_mse", "pt_views", "pt_mutable", "pt_new_added",
              "cam_R", "cam_t", "cam_c", "cam_fk"):
        assert np.asarray(got[k]).dtype == np.asarray(want[k]).dtype, k
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert got["cam_fk"].tolist() == [[100.0, 1e-3, 2e-3]] * 2


def test_normalize_cameras_without_noise_keeps_the_rotation():
    rng = np.random.default_rng(3)
    pose = rng.normal(0, 0.3, (2, 6))
    c = rng.normal(0, 5, (2, 3))
    mid, scale = np.array([1.0, -2.0, 3.0]), 7.5
    p, R, t, cc = incremental.normalize_cameras(pose, c, mid, scale)
    np.testing.assert_array_equal(p[:, :3], pose[:, :3])
    np.testing.assert_array_equal(cc, scale * (c - mid))
    np.testing.assert_allclose(np.einsum("nij,nj->ni", R, cc), -t, rtol=0, atol=1e-12)
    np.testing.assert_array_equal(p[:, 3:], t)
    nz = rng.standard_normal((2, 2, 3))
    p2, R2, t2, c2 = incremental.normalize_cameras(pose, c, mid, scale, nz)
    np.testing.assert_allclose(p2[:, :3], pose[:, :3] + 0.1 * nz[:, 0], atol=1e-12)       # R -> angle-axis -> R round trip
    np.testing.assert_allclose(c2, -np.einsum("nji,nj->ni", R2, t2), atol=1e-10)
    assert np.abs(t2 - t).max() > 0.1


def test_each_strip_starts_with_a_pair_that_passes(refs):
    """tests/test_gpu_seedstart.py::test_whole_models needs a seed in either strip: the first ranked pair of all images, and the
    first ranked pair once the first strip is processed, pass the gates (oracle relpose_5pt + tests/seed_ref.cpp)."""
    c = SD.strips_case()
    nf, pairs, moff, m = c["store"]
    n = len(nf)
    case = dict(n_features=nf, pairs=pairs, match_off=moff, matches=m, keypoints=c["keypoints"])
    processed = np.zeros(n, bool)
    for strip in range(2):
        hyp = seed.sort_image_pairs(c["book"]["match_count"], processed)[:64]
        fk = np.zeros((len(hyp), 2, 3)); fk[:, :, 0] = SD.STRIP_F
        want = D.expected(*refs, case, hyp, fk, np.zeros(len(hyp), np.uint8))
        print("strip", strip, "first pair", hyp[0].tolist(), "points", np.diff(want["pt_off"])[0], "of", want["n_matches"][0])
        assert want["winner"] == 0
        processed[(hyp[0, 0] // SD.STRIP_IMAGES) * SD.STRIP_IMAGES:][:SD.STRIP_IMAGES] = True
    assert processed.all()
