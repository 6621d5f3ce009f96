"""The two restatements of msfm_descset_voctree_train - numpy (tests/voctrain_ref.py) and a literal scalar loop
(tests/voctrain_ref.cpp) - against each other, and what the stated arithmetic promises on the restatement itself."""
import numpy as np
import pytest

from tests import voctrain_data as D
from tests import voctrain_ref as V


@pytest.fixture(scope="module")
def ref_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("voctrain_ref") / "voctrain_ref"
    D.build_ref_cpp(exe)
    return exe


def test_the_scenes_hold_what_they_are_there_for():
    D.check_scenes()


@pytest.mark.parametrize("name", sorted(D.scenes()))
def test_the_two_restatements_agree_byte_for_byte(ref_exe, tmp_path, name):
    imgs, opt = D.scenes()[name]
    want, want_st, _ = D.expected(name)
    got, got_st, _ = D.run_ref_cpp(ref_exe, tmp_path, imgs, **opt)
    assert V.same_tree(want, got) is None, V.same_tree(want, got)
    assert V.same_stats(want_st, got_st) is None, V.same_stats(want_st, got_st)


def objective(X, mem, assign, centres):
    d = X[mem].astype(np.float64) - centres[assign].astype(np.float64)
    return float((d * d).sum())


@pytest.mark.parametrize("name", ["ragged", "k64", "floats", "runs_out"])
def test_the_objective_never_rises(name):
    """Per node, in binary64: J(assignment t, centres t) >= J(assignment t + 1, centres t) up to the rounding of the binary32
    distances that decide an assignment, and J(assignment, its means) <= J(assignment, any other centres) up to the rounding of
    the means to binary32.  Both slacks are relative 2^-20 of the objective: a distance of 128 terms carries at most 128 * 2^-24
    relative error and the sum over members no more; a mean's rounding moves each of m * 128 terms by at most 2^-24 of |x|."""
    X = np.concatenate([np.asarray(d, np.float32).reshape(-1, 128) for d in D.scenes()[name][0][::D.scenes()[name][1].get("image_step", 1)]])
    _, _, trace = D.expected(name)
    nodes = {}
    for t in trace:
        nodes.setdefault((t["level"], t["ordinal"]), []).append(t)
    assert len(nodes) >= 1
    checked = 0
    for steps in nodes.values():
        last = None
        for t in steps:
            now = objective(X, t["mem"], t["assign"], t["centres"])
            if last is not None:
                assert now <= last * (1 + 2.0 ** -20) + 1e-9, (t["level"], t["ordinal"], t["it"], last, now)
                checked += 1
            last = now
    assert checked >= 3


@pytest.mark.parametrize("name", ["ragged", "k64"])
def test_final_centres_are_the_binary64_means_to_one_ulp(name):
    """Integer-valued data: the int64 sums are exact, so a centre is the binary64 quotient rounded once to binary32; numpy's
    own binary64 mean (pairwise summation, exact here as well: the sums stay below 2^53) differs by the quotient's rounding."""
    imgs, opt = D.scenes()[name]
    X = np.concatenate(imgs)
    assert (X == np.round(X)).all()
    _, _, trace = D.expected(name)
    final = {}
    for t in trace:
        final[(t["level"], t["ordinal"])] = t
    n = 0
    for t in final.values():
        for c in np.unique(t["assign"]):
            mean = X[t["mem"][t["assign"] == c]].astype(np.float64).mean(axis=0)
            got = t["centres"][c].astype(np.float64)
            ulp = np.spacing(np.abs(mean).astype(np.float32)).astype(np.float64)
            assert (np.abs(got - mean) <= ulp).all()
            n += 1
    assert n > 20


def test_planted_clusters_come_back_at_the_root():
    """The seed of the scene was chosen on the CPU as the first for which the restatement finds the planted partition
    (k-means++ does not promise it for every seed); see tests/voctrain_data.py."""
    rows, pick = D.planted_rows()
    tree, st, trace = D.expected("converges")
    a = trace[-1]["assign"]
    assert len(set(zip(a.tolist(), pick.tolist()))) == D.PLANTED_K
    assert tree["block_n"][0] == D.PLANTED_K and st["level_capped"] == [0]
    for c in range(D.PLANTED_K):
        members = rows[a == c]
        assert np.abs(tree["node_desc"][0, c] - members.mean(axis=0)).max() < 1e-3


def test_refusals_of_the_restatement():
    imgs = [np.zeros((4, 128), np.float32)]
    for bad in (dict(k=1), dict(k=65), dict(levels=0), dict(levels=33), dict(max_iters=0), dict(image_step=0)):
        with pytest.raises(ValueError):
            V.train(imgs, **bad)
    for v in (np.nan, np.inf, 2896.0, -2896.0):
        x = imgs[0].copy()
        x[1, 7] = v
        with pytest.raises(ValueError):
            V.train([x])
    with pytest.raises(ValueError):
        V.train([np.zeros((0, 128), np.float32)])
    x = imgs[0].copy()
    x[1, 7] = np.float32(2895.9998)
    V.train([x])
    assert V.draw(0, 0, 0, 0) != V.draw(0, 0, 0, 1) != V.draw(0, 1, 0, 1) != V.draw(1, 1, 0, 1)
