"""The planted pairs of tests/slam_chain_ref.py contain every case tests/test_gpu_slam_chain.py compares on, by the sequential
restatement alone (CPU oracle, no GPU): the GPU test cannot pass vacuously."""
import numpy as np
import pytest

from tests import slam_chain_ref as R

SEED = 0x4D53464D46


@pytest.fixture(scope="module")
def planted():
    pl = R.planted_pairs()
    return pl, R.planted_reference(pl, seed=SEED)


def test_survivors_are_the_planted_ones(planted):
    pl, ref = planted
    for p, (i, j) in enumerate(pl["pairs"]):
        s = R.survivors(ref["codes"][p])
        assert len(s) == pl["want"][p], (p, len(s))
        assert len(ref["codes"][p]) == len(pl["descs"][j])
        # a survivor joins two features of one world point, in query order
        assert (pl["wid"][i][s[:, 0]] == pl["wid"][j][s[:, 1]]).all() and (pl["wid"][j][s[:, 1]] >= 0).all()
        assert (np.diff(s[:, 1]) > 0).all()


def test_every_case_occurs(planted):
    pl, ref = planted
    pairs, want, n_m, ok = pl["pairs"], np.array(pl["want"]), ref["n_matches"], ref["ok"]
    nq = np.array([len(pl["descs"][j]) for _, j in pairs])
    assert {0, 1, 255, 256, 257, 600} <= set(nq.tolist())
    assert {0, 29, 30, 31, 200} <= set(want.tolist())
    # fewer than 30 survivors keep nothing, with or without query features
    assert (n_m[want < 30] == 0).all() and (ok[want < 30] == 0).all()
    assert ((want == 0) & (nq > 0)).any() and ((want == 0) & (nq == 0)).any() and (want == 29).any() and (want == 1).any()
    # 30 or more survivors, 1..29 inliers: the verdict is 0 and the matches stay
    low = (want >= 30) & (ok == 0)
    assert low.any() and ((n_m[low] >= 1) & (n_m[low] <= 29)).all(), (want, n_m, ok)
    # that pair's survivors lie in the last 256-chunk of a 600-feature query image
    p7 = int(np.nonzero(low)[0][0])
    assert nq[p7] == 600 and R.survivors(ref["codes"][p7])[:, 1].min() >= 512
    # verdict 1, at exactly 30 survivors too
    assert (ok[want == 200] == 1).all() and (n_m[want == 200] >= 150).all()
    assert ((want == 30) & (ok == 1)).any()
    assert (ok == 1).sum() >= 4 and ((ok == 1) == (n_m >= 30)).all()
    # an empty pair between two full ones: the offsets of the neighbours
    assert any(n_m[p - 1] > 0 and n_m[p] == 0 and n_m[p + 1] > 0 for p in range(1, len(pairs) - 1))
    # the same image in several pairs, as train and as query
    tr, qu = pairs[n_m > 0, 0].tolist(), pairs[n_m > 0, 1].tolist()
    assert any(tr.count(i) >= 2 and qu.count(i) >= 1 for i in set(tr)) and any(qu.count(j) >= 2 for j in set(qu))
    # kept matches: a subset of the survivors in ascending query order, F where a model was found
    for p in range(len(pairs)):
        k = ref["kept"][p]
        assert len(k) == n_m[p] and (np.diff(k[:, 1]) > 0).all()
        assert (np.abs(ref["F"][p]).sum() > 0) == (want[p] >= 30)


def test_tracks_join_the_pairs(planted):
    """Tracks of more than two views exist (an image is train in one pair and query in another) and every track is one
    world point, except where a false survivor was kept."""
    pl, ref = planted
    off, img, feat = ref["tracks"]
    assert len(off) - 1 > 100 and np.diff(off).max() >= 3
    pure = [len({int(pl["wid"][i][f]) for i, f in zip(img[off[t]:off[t + 1]], feat[off[t]:off[t + 1]])}) == 1 for t in range(len(off) - 1)]
    assert np.mean(pure) == 1.0      # (a survivor always joins two features of one world point)
    g = R.match_graph(len(pl["descs"]), pl["pairs"], ref["kept"])
    assert g.sum() == ref["n_matches"].sum() and g[0, 1] == ref["n_matches"][0] and g[1, 0] == ref["n_matches"][7]
