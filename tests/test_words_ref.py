"""The visual words without a GPU: the two restatements of the descent against each other, the conditions planted into the
data, and the reference's files (voctree, <i>_words)."""
import numpy as np
import pytest

from metricsfm_amd import featurefiles as FF
from tests import words_data as D
from tests import words_ref as R


@pytest.fixture(scope="module")
def ref_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("words_ref") / "words_ref"
    D.build_ref_cpp(exe)
    return exe


@pytest.mark.parametrize("name", sorted(D.scenes()))
def test_numpy_and_cpp_restatements_agree(name, ref_exe, tmp_path):
    tree, imgs, mf = D.scenes()[name]
    got, _ = D.run_ref_cpp(ref_exe, tmp_path, tree, imgs, mf)
    assert R.same(D.expected(name), got) is None


def test_trees_have_the_shapes_they_promise():
    sizes, leaf_depths, deepest = D.tree_stats(D.ragged_tree())
    assert sizes == set(range(1, 11)) and leaf_depths == {1, 2, 3, 4} and deepest == 4
    assert int(D.ragged_tree()["node_link"][0, 7]) == 0
    assert D.tree_stats(D.k3_tree())[2] == 6 and D.tree_stats(D.k64_tree())[2] == 1
    assert tuple(len(i) for i in D.ragged_images()[0]) == D.SIZES


def test_planted_near_ties_tell_the_arithmetics_apart():
    p = D.planted()
    assert p["n_planted"] == 256 and all(v >= 16 for v in p["differs"].values()), p["differs"]
    e = D.expected("planted")
    assert e["n_unassigned"] == 0 and e["has_words"][0] == 1
    # every planted feature ends in one of the two leaves of its own pair
    assert np.array_equal(e["word_id"][:256] // 2, np.arange(256))


def test_bags_depend_on_the_order_of_the_sum():
    D.bag_images()   # asserts it
    e = D.expected("k64")
    assert e["bow_off"][1] == 12 and e["num_words"] == 11


def test_degenerate_rows_and_the_link_to_block_0_end_without_a_word():
    imgs, stop = D.ragged_images()
    e = D.expected("ragged")
    last = e["word_id"][e["feat_off"][-2]:]
    assert (last[stop] == -1).all() and last[10] == (int(D.ragged_tree()["node_link"][0, 0]) & 0x7FFFFFFF)
    assert e["n_unassigned"] >= len(stop)
    assert list(e["has_words"]) == [0] * 9 + [1, 1]           # 300 features: none; 301: words
    assert list(D.expected("ragged_all")["has_words"]) == [0] + [1] * 10


@pytest.mark.parametrize("layout", [None, dict(alignment=64, feature_off_start=128, desc_size_bytes_wp=576)])
def test_voctree_file_round_trips(layout, tmp_path):
    t = D.ragged_tree()
    rng = np.random.default_rng(5)
    nb = len(t["block_n"])
    leaf, parent = rng.integers(0, 2, nb).astype(np.uint16), rng.integers(0, nb, nb).astype(np.uint32)
    lay = None if layout is None else FF.voctree_layout(t["k"], **layout)
    path = tmp_path / "voctree"
    FF.write_voctree(path, t["k"], t["block_n"], t["node_desc"], t["node_link"], t["node_weight"], leaf, parent, layout=lay)
    got = FF.read_voctree(path)
    assert got["k"] == t["k"]
    for name in ("block_n", "node_desc", "node_link", "node_weight"):
        assert got[name].dtype == t[name].dtype and np.array_equal(got[name], t[name]), name
    assert np.array_equal(got["block_leaf"], leaf) and np.array_equal(got["block_parent"], parent)
    if layout is not None:
        assert got["layout"]["feature_off_start"] == 128 and got["layout"]["desc_size_bytes_wp"] == 576
        assert got["layout"]["child_off_start"] == 128 + 10 * 576 and got["layout"]["block_size_bytes_wp"] % 64 == 0
    # the header is the reference's: 60 bytes, then _total_size bytes
    raw = open(path, "rb").read()
    assert len(raw) == 60 + nb * got["layout"]["block_size_bytes_wp"]
    # the same descent from the file
    assert R.same(R.words_of_set(got, D.ragged_images()[0], 300), D.expected("ragged")) is None


def test_words_files_round_trip_with_the_running_maximum(tmp_path):
    e = D.expected("ragged_all")
    running = FF.write_all_words(str(tmp_path), e)
    want = np.maximum.accumulate(np.where(e["has_words"] > 0, e["image_max_id"], 0))
    assert np.array_equal(running, want) and running[-1] == e["num_words"] and len(set(running)) > 2
    fo, bo = e["feat_off"], e["bow_off"]
    for i in range(e["n_images"]):
        ids, w, max_id, wid = FF.read_words(str(tmp_path), i)
        if not e["has_words"][i]:
            assert ids is None
            continue
        assert np.array_equal(ids, e["bow_word"][bo[i]:bo[i + 1]]) and w.tobytes() == e["bow_weight"][bo[i]:bo[i + 1]].tobytes()
        assert max_id == running[i] and np.array_equal(wid, e["word_id"][fo[i]:fo[i + 1]])
        assert (np.diff(ids) > 0).all()
