"""msfm_voctree_create / msfm_descset_words / msfm_wordset_create_from_words against the restatement tests/words_ref.py: every
comparison is exact, the weights bit for bit."""
import os

import numpy as np
import pytest

from metricsfm_amd import _abi as A
from metricsfm_amd import capi, featurefiles, pairsel
from tests import pairselect_data as PD
from tests import words_data as D
from tests import words_ref as R

pytestmark = pytest.mark.gpu
LEAF = 0x80000000


def gpu_words(ctx, tree, imgs, min_features, keypoints=None):
    """-> (result dict as words_ref.words_of_set gives it, tree sizes)"""
    vt = ctx.voctree(tree["k"], tree["block_n"], tree["node_desc"], tree["node_link"], tree["node_weight"])
    ds = ctx.descset([np.zeros((0, 128), np.float32) if len(d) == 0 else d for d in imgs], keypoints)
    try:
        res = ds.words(vt, min_features)
        try:
            got = dict(res.fetch(), **res.size())
        finally:
            res.close()
        return got, vt.size()
    finally:
        ds.close()
        vt.close()


@pytest.mark.parametrize("name", ["ragged", "k3", "k64"])
def test_words_bags_and_maxima_equal_the_restatement(ctx, name):
    tree, imgs, mf = D.scenes()[name]
    got, size = gpu_words(ctx, tree, imgs, mf)
    want = D.expected(name)
    assert R.same(want, got) is None, R.same(want, got)
    assert size["k"] == tree["k"] and size["n_blocks"] == len(tree["block_n"]) and size["depth"] == D.tree_stats(tree)[2]
    assert size["n_leaves"] == int(sum(((tree["node_link"][b, :n] & LEAF) != 0).sum() for b, n in enumerate(tree["block_n"])))
    assert size["h2d_bytes"] >= tree["node_desc"].nbytes


def test_planted_near_ties_follow_the_eight_partial_sums(ctx):
    p = D.planted()
    got, _ = gpu_words(ctx, p["tree"], p["images"], 300)
    want = D.expected("planted")
    assert np.array_equal(got["word_id"], want["word_id"]), int((got["word_id"] != want["word_id"]).sum())
    assert R.same(want, got) is None
    assert min(p["differs"].values()) >= 16   # the data tells a fused, a sequential and a binary64 sum apart


def test_the_min_features_rule_and_short_images(ctx):
    tree, imgs, _ = D.scenes()["ragged"]
    got, _ = gpu_words(ctx, tree, imgs, 300)
    assert list(got["has_words"]) == [0] * 9 + [1, 1] and len(imgs[8]) == 300 and len(imgs[9]) == 301
    fo = got["feat_off"]
    assert (got["word_id"][:fo[9]] == -1).all() and got["bow_off"][9] == 0 and not got["image_max_id"][:9].any()
    got0, _ = gpu_words(ctx, tree, imgs, 0)
    want0 = D.expected("ragged_all")
    assert list(got0["has_words"]) == [0] + [1] * 10
    assert R.same(want0, got0) is None, R.same(want0, got0)


def test_rows_without_a_word(ctx):
    tree, imgs, _ = D.scenes()["ragged"]
    _, stop = D.ragged_images()
    got, _ = gpu_words(ctx, tree, imgs, 300)
    want = D.expected("ragged")
    base = got["feat_off"][10]
    last = got["word_id"][base:]
    assert (last[stop] == -1).all() and got["n_unassigned"] == want["n_unassigned"] >= len(stop)
    bag = got["bow_word"][got["bow_off"][10]:got["bow_off"][11]]
    assert sorted(set(last[last >= 0].tolist())) == list(bag) and -1 not in bag
    assert got["image_max_id"][10] == last.max() and got["num_words"] == max(got["image_max_id"])
    # the same rows alone: nothing gets a word, the maximum stays 0, the bag is empty
    only = [imgs[10][stop], imgs[10][stop]]
    alone, _ = gpu_words(ctx, tree, only, 0)
    assert (alone["word_id"] == -1).all() and alone["n_unassigned"] == 2 * len(stop) and alone["n_bow"] == 0
    assert not alone["image_max_id"].any() and alone["num_words"] == 0


def small_tree():
    """k = 3: the root's node 1 links block 1 (two leaves).  Constant descriptors: 0 and 100 in the root, 90 and 200 below."""
    desc = np.zeros((2, 3, 128), np.float32)
    desc[0, 1], desc[1, 0], desc[1, 1] = 100, 90, 200
    return dict(k=3, block_n=np.array([2, 2], np.uint16), node_desc=desc,
                node_link=np.array([[LEAF | 1, 1, 0], [LEAF | 2, LEAF | 3, 0]], np.uint32), node_weight=np.ones((2, 3), np.float32))


def test_tree_refusals_leave_the_context_usable(ctx):
    t = small_tree()

    def refused(**change):
        u = dict(t, **change)
        with pytest.raises(capi.MsfmError) as e:
            ctx.voctree(u["k"], u["block_n"], u["node_desc"], u["node_link"], u["node_weight"])
        assert e.value.code == A.MSFM_E_INVAL

    for k in (1, 65):
        refused(k=k, node_desc=np.zeros((2, k, 128), np.float32), node_link=np.zeros((2, k), np.uint32), node_weight=np.zeros((2, k), np.float32))
    refused(block_n=np.array([2, 4], np.uint16))                                              # above k
    refused(block_n=np.array([2, 0], np.uint16))                                              # reached and empty
    refused(node_link=np.array([[LEAF | 1, 2, 0], [LEAF | 2, LEAF | 3, 0]], np.uint32))       # child outside the tree
    refused(node_link=np.array([[1, 1, 0], [LEAF | 2, LEAF | 3, 0]], np.uint32))              # reached twice
    refused(node_link=np.array([[LEAF | 1, 1, 0], [1, LEAF | 3, 0]], np.uint32))              # a cycle
    deep = 33
    chain = np.zeros((deep, 3), np.uint32)
    chain[:, 0] = np.arange(1, deep + 1)
    chain[-1, 0] = LEAF | 1
    refused(block_n=np.ones(deep, np.uint16), node_desc=np.zeros((deep, 3, 128), np.float32), node_link=chain,
            node_weight=np.ones((deep, 3), np.float32))
    L, out = capi.lib(), capi.C.c_void_p()
    bn = np.array([2, 2], np.uint16)
    assert L.msfm_voctree_create(ctx._h, 3, 2, A.ptr(bn, capi.C.POINTER(capi.C.c_uint16)), None, None, None, capi.C.byref(out)) == A.MSFM_E_INVAL
    # a link to block 0 is legal, and the context still works
    ok = dict(t, node_link=np.array([[LEAF | 1, 1, 0], [0, LEAF | 3, 0]], np.uint32))
    imgs = [np.tile(ok["node_desc"][1, 0], (3, 1)), np.tile(ok["node_desc"][0, 0], (2, 1))]
    got, size = gpu_words(ctx, ok, imgs, 0)
    assert list(got["word_id"]) == [-1, -1, -1, 1, 1] and got["n_unassigned"] == 3 and size["depth"] == 2 and size["n_leaves"] == 2
    assert R.same(R.words_of_set(ok, imgs, 0), got) is None


@pytest.fixture(scope="module")
def pair_scene():
    """The planted pair-selection scene with descriptors that the tree of words_data.tree_for_words turns back into its words;
    the image without words there gets random words here (it has 400 features, so the 300 rule gives it words)."""
    d = PD.planted_scene()
    tree, desc_of_word = D.tree_for_words(d["num_words"])
    rng = np.random.default_rng(11)
    words = [rng.integers(0, d["num_words"], d["n_features"][i]).astype(np.int32) if w is None else w for i, w in enumerate(d["words"])]
    descs = [desc_of_word[w] for w in words]
    want = R.words_of_set(tree, descs, 300)
    assert np.array_equal(want["word_id"], np.concatenate(words)) and want["n_unassigned"] == 0
    kps = [d["keypoints"][d["feat_off"][i]:d["feat_off"][i + 1]] for i in range(len(words))]
    return dict(d, tree=tree, descs=descs, words=words, kps=kps, want=want)


def test_wordset_from_words_equals_the_host_route(ctx, pair_scene):
    s = pair_scene
    t = s["tree"]
    vt = ctx.voctree(t["k"], t["block_n"], t["node_desc"], t["node_link"], t["node_weight"])
    ds = ctx.descset(s["descs"], s["kps"])
    res = ds.words(vt)
    try:
        got = dict(res.fetch(), **res.size())
        assert R.same(s["want"], got) is None
        dev = res.wordset()
        host = ctx.wordset(s["n_features"], s["words"], got["num_words"], s["keypoints"])
        try:
            a, b = dev.fetch(), host.fetch()
            for name in b:
                assert np.array_equal(a[name], b[name]), name
            assert (dev.n_images, dev.n_hypotheses, dev.n_inverted, dev.n_mapped) == (host.n_images, host.n_hypotheses, host.n_inverted, host.n_mapped)
            sa, sb = dev.select(0, 6), host.select(0, 6)
            for name in sb:
                assert np.array_equal(sa[name], sb[name]), name
            assert len(sa["pairs"]) > 0
            assert dev.h2d_bytes < 4 * got["n_features"] < host.h2d_bytes
        finally:
            dev.close()
            host.close()
        # refusals: a stale generation, an image with words but no keypoints, features without a word, one image
        with pytest.raises(capi.MsfmError) as e:
            res.wordset(max_hypotheses=12)
        assert e.value.code == A.MSFM_E_INVAL
        ctx.check(capi.lib().msfm_descset_upload(ds._h, 3, A.ptr(s["descs"][3], A.c_float_p), len(s["descs"][3])))
        with pytest.raises(capi.MsfmError) as e:
            res.wordset()
        assert e.value.code == A.MSFM_E_INVAL
        fresh = ds.words(vt)
        try:
            with pytest.raises(capi.MsfmError) as e:     # the upload dropped image 3's keypoints
                fresh.wordset()
            assert e.value.code == A.MSFM_E_INVAL
            ds.upload_keypoints(3, s["kps"][3])
            ws = fresh.wordset()
            assert np.array_equal(ws.fetch()["hyp_img"], a["hyp_img"])
            ws.close()
        finally:
            fresh.close()
    finally:
        res.close()
        ds.close()
    rimgs, _ = D.ragged_images()
    rt = D.ragged_tree()
    vr = ctx.voctree(rt["k"], rt["block_n"], rt["node_desc"], rt["node_link"], rt["node_weight"])
    for imgs in (rimgs[9:], rimgs[9:10]):     # features without a word; a single image
        ds = ctx.descset(imgs, [np.zeros((len(i), 2), np.float32) for i in imgs])
        res = ds.words(vr if len(imgs) == 2 else vt)
        try:
            with pytest.raises(capi.MsfmError) as e:
                res.wordset()
            assert e.value.code == A.MSFM_E_INVAL
        finally:
            res.close()
            ds.close()
    vr.close()
    vt.close()
    assert ctx.knn2(s["descs"][0][:64], s["descs"][1][:64])[0].shape == (64, 2)   # the context goes on working


def test_golden_fixture(ctx):
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "words_golden.npz"))
    tree = {name: g["tree_" + name] for name in ("block_n", "node_link", "node_weight")}
    tree.update(k=int(g["tree_k"]), node_desc=g["tree_node_desc"].astype(np.float32))
    imgs = [g["desc_%d" % i].astype(np.float32) for i in range(3)]
    got, _ = gpu_words(ctx, tree, imgs, 300)
    want = {name: g["want_" + name] for name in R.ARRAYS + R.SCALARS}
    assert R.same(want, got) is None, R.same(want, got)
    assert list(got["has_words"]) == [1, 0, 1] and got["n_bow"] > 10


def test_select_pairs_from_descriptors(ctx, pair_scene, tmp_path):
    s = pair_scene
    t = s["tree"]
    vt = ctx.voctree(t["k"], t["block_n"], t["node_desc"], t["node_link"], t["node_weight"])
    ds = ctx.descset(s["descs"], s["kps"])
    try:
        pairs, rec = pairsel.select_pairs_from_descriptors(ctx, ds, vt, rows_per_call=5, fold=str(tmp_path))
    finally:
        ds.close()
        vt.close()
    want_pairs, want = pairsel.select_pairs(ctx, s["n_features"], s["words"], rec["num_words"], s["keypoints"], rows_per_call=5)
    assert np.array_equal(pairs, want_pairs) and len(pairs) > 0
    for name in ("hyp_img", "hyp_sim", "n_init", "n_inliers", "verdict"):
        assert np.array_equal(rec[name], want[name]), name
    assert rec["match_graph_init"] == want["match_graph_init"] and rec["n_unassigned"] == 0 and rec["num_words"] == s["want"]["num_words"]
    e = s["want"]
    running = np.maximum.accumulate(e["image_max_id"])
    for i in range(e["n_images"]):
        ids, w, max_id, wid = featurefiles.read_words(str(tmp_path), i)
        bo = e["bow_off"]
        assert np.array_equal(ids, e["bow_word"][bo[i]:bo[i + 1]]) and w.tobytes() == e["bow_weight"][bo[i]:bo[i + 1]].tobytes()
        assert max_id == running[i] and np.array_equal(wid, s["words"][i])
    assert os.path.exists(os.path.join(str(tmp_path), "similarity_graph.txt"))
