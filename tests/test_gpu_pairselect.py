"""msfm_wordset_create / msfm_pair_select (include/msfm.h, "Which image pairs to match") against the sequential restatement
tests/pairselect_ref.py on the planted scenes of tests/pairselect_data.py.  Every comparison is exact: the restatement's
joins go through Context.fundamental_ransac with the same options, and the library promises that call's results bit for bit."""
import subprocess

import numpy as np
import pytest

from metricsfm_amd import _abi as A
from metricsfm_amd import capi, matchfiles, pairsel
from tests import pairselect_data as D
from tests import pairselect_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def data():
    d = D.planted_scene()
    d["ref"] = ref.match_graph_feature(d["words"], d["num_words"], ref.th_num_match(len(d["words"])))
    return d


@pytest.fixture(scope="module")
def wordset(ctx, data):
    ws = ctx.wordset(data["n_features"], data["words"], data["num_words"], data["keypoints"])
    yield ws
    ws.close()


def composition(ctx, d, rows, **opts):
    """The restatement's joins of these rows as one fundamental-RANSAC batch, then the gates."""
    r = d["ref"]
    off, matches, p1, p2 = ref.problem_list(r["joins"], rows, d["keypoints"], d["feat_off"], r["hyp_img"])
    F, inl, nin, ok = ctx.fundamental_ransac(off, p1, p2, **opts)
    n_init = np.diff(off)
    verdict = ref.gates(n_init, ok, nin)
    K = r["hyp_img"].shape[1]
    pairs = [(i, int(r["hyp_img"][i][s])) for k, i in enumerate(rows) for s in range(K) if verdict[k * K + s] == 0]
    return dict(init_off=off, init_matches=matches, F=F, init_inlier=inl, n_inliers=nin, n_init=n_init, verdict=verdict,
                pairs=np.array(pairs, np.int32).reshape(-1, 2))


def assert_equal_sets(got, want, rows, K):
    assert (got["n_init"].reshape(-1) == want["n_init"]).all()
    assert (got["init_off"] == want["init_off"]).all()
    assert (got["init_matches"] == want["init_matches"]).all()
    assert (got["F"].reshape(-1, 3, 3) == want["F"]).all()
    assert (got["n_inliers"].reshape(-1) == want["n_inliers"]).all()
    assert (got["init_inlier"] == want["init_inlier"]).all()
    assert (got["verdict"].reshape(-1) == want["verdict"]).all()
    assert (got["pairs"] == want["pairs"]).all() and got["pairs"].shape == want["pairs"].shape
    assert got["n_init"].shape == (len(rows), K)


def test_planted_scene_has_what_it_plants(data):
    inv = ref.generate_inverted_file(data["words"], data["num_words"])
    assert inv[D.WORD_IN_5] == [1, 2, 3, 4, 5] and inv[D.WORD_IN_6] == []
    assert sum(ref.keep_unique_vector(list(data["words"][k])).count(D.WORD_IN_6) for k in range(1, 7)) == 6
    maps = data["ref"]["maps"]
    a, b = D.RANDOM_PAIR
    assert sorted(w for w in maps[a] if w in maps[b] and w >= 411) == list(range(420, 500, 2))
    assert maps[D.NO_WORDS_IMAGE] == {}
    assert any(len(w) != len(set(w.tolist())) for w in data["words"] if w is not None)


def test_wordset_fetch_equals_the_restatement(ctx, data, wordset):
    r = data["ref"]
    got = wordset.fetch()
    assert wordset.n_hypotheses == 11 and wordset.n_images == 12
    assert (got["similarity"] == r["similarity"]).all() and r["similarity"].any()
    assert (got["hyp_img"] == r["hyp_img"]).all() and (got["hyp_sim"] == r["hyp_sim"]).all()
    off, word, feat = ref.tables_flat(r["maps"])
    assert (got["map_off"] == off).all() and (got["map_word"] == word).all() and (got["map_feat"] == feat).all()
    assert wordset.n_mapped == len(word) and wordset.n_inverted > 0
    # the first four of every ranking, with the ties of the image without words (similarity 0 to everybody: ids ascending)
    ws4 = ctx.wordset(data["n_features"], data["words"], data["num_words"], data["keypoints"], max_hypotheses=4)
    try:
        g4 = ws4.fetch(similarity=False)
    finally:
        ws4.close()
    assert g4["similarity"] is None and g4["hyp_img"].shape == (12, 4)
    assert (g4["hyp_img"] == r["hyp_img"][:, :4]).all() and (g4["hyp_sim"] == r["hyp_sim"][:, :4]).all()
    assert list(g4["hyp_img"][D.NO_WORDS_IMAGE]) == [0, 1, 2, 3] and not g4["hyp_sim"][D.NO_WORDS_IMAGE].any()
    assert any(len(set(row.tolist())) < 4 for row in g4["hyp_sim"])   # ties inside the first four


def test_pair_select_equals_the_composition(ctx, data, wordset):
    rows = list(range(12))
    got = wordset.select()
    want = composition(ctx, data, rows)
    assert_equal_sets(got, want, rows, 11)
    ver = got["verdict"]
    assert {0, 1, 2} <= set(ver.reshape(-1).tolist())
    a, b = D.RANDOM_PAIR
    slot = list(data["ref"]["hyp_img"][a]).index(b)
    assert got["n_init"][a, slot] >= 40 and ver[a, slot] == 2   # joined on 40 planted words, but no geometry behind them
    assert not (ver[D.NO_WORDS_IMAGE] != 1).any()
    lean = wordset.select(details=False)
    assert sorted(lean) == ["n_init", "n_inliers", "pairs", "verdict"] and (lean["pairs"] == got["pairs"]).all()


def test_chunks_equal_the_composition_of_their_own_rows(ctx, data, wordset):
    for first, rows in ((0, 5), (5, 7)):
        got = wordset.select(first, rows)
        assert_equal_sets(got, composition(ctx, data, list(range(first, first + rows))), range(rows), 11)


def test_fewer_slots_and_other_thresholds(ctx, data, wordset):
    got = wordset.select(2, 3, max_hypotheses=4, th_init_matches=10, th_inliers=45, min_points=10, seed=77)
    r = data["ref"]
    off, matches, p1, p2 = ref.problem_list([j[:4] for j in r["joins"]], [2, 3, 4], data["keypoints"], data["feat_off"], r["hyp_img"])
    F, inl, nin, ok = ctx.fundamental_ransac(off, p1, p2, min_points=10, seed=77)
    assert got["n_init"].shape == (3, 4) and (got["init_matches"] == matches).all() and (got["F"].reshape(-1, 3, 3) == F).all()
    assert (got["verdict"].reshape(-1) == ref.gates(np.diff(off), ok, nin, 10, 45)).all()


def test_refusals_leave_the_set_usable(ctx, data, wordset):
    for first, rows in ((-1, 2), (0, 13), (12, 1), (3, 0)):
        with pytest.raises(capi.MsfmError) as e:
            wordset.select(first, rows)
        assert e.value.code == A.MSFM_E_INVAL
    with pytest.raises(capi.MsfmError) as e:
        wordset.select(max_hypotheses=12)
    assert e.value.code == A.MSFM_E_INVAL
    bad = [None if w is None else w.copy() for w in data["words"]]
    bad[3][7] = data["num_words"] + 1
    for words, n in ((bad, 12), (data["words"][:1], 1)):
        with pytest.raises(capi.MsfmError) as e:
            ctx.wordset(data["n_features"][:n], words, data["num_words"], data["keypoints"][:data["feat_off"][n]])
        assert e.value.code == A.MSFM_E_INVAL
    got = wordset.select(0, 2, details=False)
    assert [len(j) for j in data["ref"]["joins"][0]] == list(got["n_init"][0])


def test_long_tables_join_in_order(ctx):
    d = D.long_tables()
    r = ref.match_graph_feature(d["words"], d["num_words"], 2)
    ws = ctx.wordset(d["n_features"], d["words"], d["num_words"], d["keypoints"])
    try:
        t = ws.fetch()
        got = ws.select()
    finally:
        ws.close()
    off, word, feat = ref.tables_flat(r["maps"])
    assert (t["map_off"] == off).all() and (t["map_word"] == word).all() and (t["map_feat"] == feat).all()
    assert off[3] - off[2] > 65536 and (t["hyp_img"] == r["hyp_img"]).all() and (t["similarity"] == r["similarity"]).all()
    o, matches, _, _ = ref.problem_list(r["joins"], [0, 1, 2], d["keypoints"], d["feat_off"], r["hyp_img"])
    assert (got["init_off"] == o).all() and (got["init_matches"] == matches).all()
    n_init = got["n_init"]
    assert n_init.max() >= 4490 and (n_init[2] > 256).all()   # image 2 walks its 70 000 entries against both short tables


def ranking(S, K):
    """The order of ref.hypotheses for every row at once (similarity descending, then image id)."""
    n = len(S)
    key = np.where(np.eye(n, dtype=bool), -1, S).astype(np.int64) * n + (n - 1 - np.arange(n))   # the diagonal last
    order = np.argsort(-key, axis=1, kind="stable")[:, :K]
    return order.astype(np.int32), np.take_along_axis(S, order, axis=1)


def test_bins_past_a_lane_group(ctx):
    # num_words 4 000: stop size 40.  Bins of 2, 16 and 17 images (either side of the lane-group limit), of 40 (the stop size:
    # counts) and of 41 (emptied), in overlapping image ranges
    d = D.sparse_images(48, 4000, {10: [3, 30], 11: range(0, 16), 12: range(5, 22), 13: range(8, 48), 14: range(0, 41)}, 0x5e4)
    S = ref.similarity_graph_inv_file(d["words"], d["num_words"])
    assert S[8, 47] == 1 and S[0, 40] == 0 and S[10, 12] == 3
    ws = ctx.wordset(d["n_features"], d["words"], d["num_words"], d["keypoints"], max_hypotheses=7)
    try:
        got = ws.fetch()
    finally:
        ws.close()
    assert (got["similarity"] == S).all()
    assert (got["hyp_img"] == np.array([ref.hypotheses(S, i, 7)[0] for i in range(48)])).all()
    img, sim = ranking(S, 7)
    assert (got["hyp_img"] == img).all() and (got["hyp_sim"] == sim).all()


def test_rankings_past_the_lds_sort(ctx):
    # 2 100 images: more keys per ranking than the in-LDS sort takes; K by the rule is 210
    n = 2100
    d = D.sparse_images(n, 300000, {20 + k: range(15 * k, 15 * k + 200, 1 + k % 3) for k in range(120)}, 0x5e5)
    S = ref.similarity_graph_inv_file(d["words"], d["num_words"])
    ws = ctx.wordset(d["n_features"], d["words"], d["num_words"], d["keypoints"])
    try:
        assert ws.n_hypotheses == ref.th_num_match(n) == 210
        got = ws.fetch()
    finally:
        ws.close()
    assert (got["similarity"] == S).all() and S.max() > 3
    img, sim = ranking(S, 210)
    assert (img[5] == ref.hypotheses(S, 5, 210)[0]).all()
    assert (got["hyp_img"] == img).all() and (got["hyp_sim"] == sim).all()


def test_pairs_go_straight_into_match_pairs(ctx, data, wordset):
    pairs = wordset.select(details=False)["pairs"]
    assert len(pairs) and pairs.dtype == np.int32
    assert (np.diff(pairs[:, 0]) >= 0).all()   # idx1-major
    sc = data["scene"]
    ds = capi.DescSet(ctx, sc.desc)
    try:
        res = ds.match_pairs(pairs)
        try:
            n_all, n_good = res.counts()
        finally:
            res.close()
    finally:
        ds.close()
    assert len(n_all) == len(pairs) and n_good.sum() > 0


def test_select_pairs_writes_the_references_files(ctx, data, wordset, tmp_path):
    pairs, rec = pairsel.select_pairs(ctx, data["n_features"], data["words"], data["num_words"], data["keypoints"], rows_per_call=12,
                                      fold=str(tmp_path))
    assert (pairs == wordset.select(details=False)["pairs"]).all()
    graph, id_last = matchfiles.read_init_match_graph(str(tmp_path))
    assert id_last == 11 and graph == rec["match_graph_init"]
    assert [(i, j) for i, row in enumerate(graph) for j in row] == [tuple(p) for p in pairs.tolist()]
    assert (matchfiles.read_similarity_graph(str(tmp_path)) == data["ref"]["similarity"]).all()
    assert rec["verdict"].shape == (12, 11)
    # other chunks: the same joins, samples of their own
    _, rec5 = pairsel.select_pairs(ctx, data["n_features"], data["words"], data["num_words"], data["keypoints"], rows_per_call=5)
    assert (rec5["n_init"] == rec["n_init"]).all()


def test_host_mirror_agrees_with_its_literal_walk(data, wordset, tmp_path):
    exe = tmp_path / "pairselect_host_check"
    subprocess.check_call(D.host_check_command(exe))
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    D.write_image_set(src, data, rows_per_call=5)
    run = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "pairselect_host_check ok" in run.stdout, run.stdout + run.stderr
    got = D.read_host_result(dst, 12)
    assert (got["hyp_img"] == data["ref"]["hyp_img"]).all()
    parts = [wordset.select(r, min(5, 12 - r), details=False) for r in (0, 5, 10)]
    for k in ("n_init", "n_inliers", "verdict"):
        assert (got[k] == np.concatenate([p[k] for p in parts])).all()
