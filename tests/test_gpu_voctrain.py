"""msfm_descset_voctree_train / msfm_voctree_fetch against the restatement tests/voctrain_ref.py: every comparison is exact, the
centres bit for bit."""
import os

import numpy as np
import pytest

from metricsfm_amd import _abi as A
from metricsfm_amd import capi, featurefiles, pairsel
from tests import voctrain_data as D
from tests import voctrain_ref as V
from tests import words_ref as R

pytestmark = pytest.mark.gpu
EMPTY = np.zeros((0, 128), np.float32)
TREE_KEYS = ("k", "block_n", "node_desc", "node_link", "node_weight")


def descset(ctx, imgs, keypoints=None):
    return ctx.descset([EMPTY if len(d) == 0 else d for d in imgs], keypoints)


def gpu_train(ctx, imgs, **opt):
    """-> (fetched tree, stats, size)"""
    ds = descset(ctx, imgs)
    try:
        vt = ds.train_voctree(**opt)
        try:
            return vt.fetch(), vt.stats, vt.size()
        finally:
            vt.close()
    finally:
        ds.close()


def check_against_restatement(ctx, name):
    imgs, opt = D.scenes()[name]
    want, want_st, _ = D.expected(name)
    got, st, size = gpu_train(ctx, imgs, **opt)
    assert V.same_tree(want, got) is None, V.same_tree(want, got)
    assert V.same_stats(want_st, st) is None, (V.same_stats(want_st, st), want_st, st)
    assert 3 <= st["host_waits"] <= V.max_host_waits(want_st)
    assert (size["k"], size["n_blocks"], size["depth"], size["n_leaves"]) == (opt["k"], want_st["n_blocks"], want_st["depth"], want_st["n_leaves"])
    assert size["h2d_bytes"] == 0      # no tree byte crossed PCIe
    return got, st


@pytest.mark.parametrize("name", ["small", "ragged", "ragged_step2", "k64", "floats", "floats_small", "floats_large"])
def test_trained_tree_and_stats_equal_the_restatement(ctx, name):
    D.check_scenes()
    check_against_restatement(ctx, name)


@pytest.mark.parametrize("name", ["few_distinct", "identical", "tie", "empties"])
def test_planted_degeneracies(ctx, name):
    D.check_scenes()
    got, st = check_against_restatement(ctx, name)
    if name == "identical":
        assert got["block_n"].tolist() == [1] and got["node_link"][0, 0] == 0x80000000 and got["block_leaf"].tolist() == [1]


def test_stopping_rules_show_in_the_stats(ctx):
    D.check_scenes()
    _, one = check_against_restatement(ctx, "ragged_one_iteration")
    _, conv = check_against_restatement(ctx, "converges")
    _, out = check_against_restatement(ctx, "runs_out")
    assert one["level_max_iters"] == [1, 1, 1] and one["level_capped"] == one["level_split"]
    assert conv["level_capped"] == [0] and conv["level_max_iters"][0] < 11
    assert out["level_capped"] == [1] and out["level_max_iters"] == [11]


def test_same_call_same_bytes_other_seed_other_tree(ctx):
    imgs, opt = D.scenes()["ragged"]
    a, sa, _ = gpu_train(ctx, imgs, **opt)
    b, sb, _ = gpu_train(ctx, imgs, **opt)
    assert V.same_tree(a, b) is None and V.same_stats(sa, sb) is None
    c, _, _ = gpu_train(ctx, imgs, **dict(opt, seed=opt["seed"] + 1))
    assert V.same_tree(a, c) is not None


def test_the_trained_tree_feeds_the_pipeline(ctx, tmp_path):
    imgs, opt = D.scenes()["ragged"]
    imgs = [EMPTY if len(d) == 0 else d for d in imgs]
    kps = [np.zeros((len(d), 2), np.float32) for d in imgs]
    ds = descset(ctx, imgs, kps)
    trained = ds.train_voctree(**opt)
    try:
        fetched = trained.fetch()
        assert V.same_tree(D.expected("ragged")[0], fetched) is None
        want = R.words_of_set(fetched, imgs, 300)
        assert want["n_unassigned"] == 0 and want["num_words"] > 100
        res = ds.words(trained)
        try:
            got = dict(res.fetch(), **res.size())
            assert R.same(want, got) is None, R.same(want, got)
            ws = res.wordset()               # the word set accepts the result
            assert ws.n_images == len(imgs)
            ws.close()
        finally:
            res.close()
        uploaded = ctx.voctree(**{name: fetched[name] for name in TREE_KEYS})
        try:
            res = ds.words(uploaded)
            try:
                assert R.same(want, dict(res.fetch(), **res.size())) is None
            finally:
                res.close()
            again = uploaded.fetch()         # an uploaded tree gives back what went in, its block fields derived from the links
            assert V.same_tree(fetched, again) is None, V.same_tree(fetched, again)
            assert uploaded.stats is None and uploaded.size()["h2d_bytes"] >= fetched["node_desc"].nbytes
            assert capi.lib().msfm_voctree_train_stats(uploaded._h, *([None] * 12)) == A.MSFM_E_INVAL      # not trained
            assert capi.lib().msfm_voctree_train_stats(trained._h, *([None] * 12)) == A.MSFM_OK
        finally:
            uploaded.close()
        path = os.path.join(str(tmp_path), "voctree")
        featurefiles.write_voctree(path, **fetched)
        back = featurefiles.read_voctree(path)
        assert V.same_tree(fetched, back) is None, V.same_tree(fetched, back)
        size = trained.size()
        assert size["n_blocks"] == len(fetched["block_n"]) and size["k"] == fetched["k"]
        assert size["n_leaves"] == int(sum(((fetched["node_link"][b, :n] & 0x80000000) != 0).sum() for b, n in enumerate(fetched["block_n"])))
    finally:
        trained.close()
        ds.close()


def test_build_vocabulary_writes_the_reference_file(ctx, tmp_path):
    imgs, opt = D.scenes()["ragged"]
    ds = descset(ctx, imgs)
    try:
        tree = pairsel.build_vocabulary(ds, num_image_voc=3, k=10, levels=3, seed=3, fold=str(tmp_path))   # 7 // 3: every second image
        try:
            assert tree.stats["n_images"] == 4
            assert V.same_tree(D.expected("ragged_step2")[0], tree.fetch()) is None
            assert V.same_tree(tree.fetch(), featurefiles.read_voctree(os.path.join(str(tmp_path), "voctree"))) is None
        finally:
            tree.close()
    finally:
        ds.close()


def test_more_than_2_23_sampled_features_are_refused(ctx):
    """The limit can only be met at its size: nine images of 2^20 features (one host array, uploaded nine times).  Step 1 samples
    9 * 2^20 features and is refused before any device work; the set goes on working (image 0 alone is a legal sample)."""
    big = np.zeros((1 << 20, 128), np.float32)
    ds = ctx.descset([big] * 9)
    try:
        with pytest.raises(capi.MsfmError) as e:
            ds.train_voctree(k=2, levels=1)
        assert e.value.code == A.MSFM_E_INVAL and "2^23" in str(e.value)
        vt = ds.train_voctree(k=2, levels=1, image_step=8 + 1)      # image 0 only: 2^20 identical members, one leaf
        try:
            assert vt.stats["n_features"] == 1 << 20 and vt.size()["n_blocks"] == 1 and vt.size()["n_leaves"] == 1
        finally:
            vt.close()
    finally:
        ds.close()


def test_refusals_leave_context_and_set_usable(ctx):
    imgs, opt = D.scenes()["ragged"]
    imgs = [d.copy() for d in imgs]
    ds = descset(ctx, imgs)

    def refused(target=None, **change):
        with pytest.raises(capi.MsfmError) as e:
            (target or ds).train_voctree(**dict(opt, **change)).close()
        assert e.value.code == A.MSFM_E_INVAL

    def accepted(target=None, **change):
        (target or ds).train_voctree(**dict(opt, **change)).close()

    try:
        for change in (dict(k=1), dict(k=65), dict(levels=0), dict(levels=33), dict(max_iters=0), dict(image_step=0)):
            refused(**change)
            accepted()
        L, out = capi.lib(), capi.C.c_void_p()
        assert L.msfm_descset_voctree_train(ds._h, 10, 3, 11, 1, 0, None) == A.MSFM_E_INVAL
        assert L.msfm_descset_voctree_train(None, 10, 3, 11, 1, 0, capi.C.byref(out)) == A.MSFM_E_INVAL and not out.value
        accepted()
        # image 3 is sampled by step 1 and not by step 2 (images 0, 2, 4, 6)
        for bad in (np.nan, np.inf, 2896.0, -2896.0):
            spoiled = [d.copy() for d in imgs]
            spoiled[3][17, 5] = bad
            ds2 = descset(ctx, spoiled)
            try:
                refused(ds2)
                accepted(ds2, image_step=2)
            finally:
                ds2.close()
        fine = [d.copy() for d in imgs]
        fine[3][17, 5] = np.float32(2895.9998)
        ds2 = descset(ctx, fine)
        try:
            accepted(ds2)
        finally:
            ds2.close()
        none = descset(ctx, [EMPTY, imgs[2], EMPTY])
        try:
            refused(none, image_step=2)      # images 0 and 2: no feature
            accepted(none)
        finally:
            none.close()
        accepted()
    finally:
        ds.close()
    assert ctx.knn2(imgs[2][:64], imgs[3][:64])[0].shape == (64, 2)   # the context goes on working
