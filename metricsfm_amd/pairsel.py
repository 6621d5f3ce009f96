"""Which image pairs to match (matching_type = "feature"): InitialMatchingGraph::match_graph_feature
(SfM/src/graph/initial_matching_graph.cc:164-294) through msfm_wordset_create + chunks of msfm_pair_select (include/msfm.h).

The sampler index of a hypothesis is its position in the msfm_pair_select call, so `rows_per_call` decides which samples a
pair sees: two runs agree bit for bit only with the same chunking."""
import os

import numpy as np

from . import capi, featurefiles, matchfiles


def rule_k(n_images):
    """th_num_match (:168-169)."""
    return min(min(max(200, n_images // 10), n_images - 1), 500)


def select_pairs(ctx: capi.Context, n_features, words, num_words, keypoints, rows_per_call=64, fold=None, max_hypotheses=0, **opts):
    """-> (pairs [n_kept][2] int32, idx1-major: the `pairs` of DescSet.match_pairs; record).  words: per image the word id of
    every feature (None: the image has no words); keypoints: flat [sum of n_features][2].  opts: fields of
    msfm_pair_select_options / msfm_fransac_options.  record: dict of hyp_img, hyp_sim, n_init, n_inliers, verdict [n][K] and
    match_graph_init (per image the kept images).  With fold, similarity_graph.txt and init_match_graph.txt are written there."""
    return _select_chunks(ctx.wordset(n_features, words, num_words, keypoints, max_hypotheses), rows_per_call, fold, opts)


def select_pairs_from_descriptors(ctx: capi.Context, descset, tree, rows_per_call=64, fold=None, min_features=300, max_hypotheses=0, **opts):
    """select_pairs for a descriptor set whose keypoints are resident (DescSet.upload_keypoints) and a `VocTree`: the words are
    computed on the device (DescSet.words, Database::BuildWords), the word set is built from them device to device
    (WordResult.wordset), then the same chunk loop.  -> (pairs, record) as select_pairs; record also holds num_words and
    n_unassigned.  With fold, every image's `<i>_words` file is written as well (featurefiles.write_all_words)."""
    res = descset.words(tree, min_features)
    try:
        size = res.size()
        if fold is not None:
            featurefiles.write_all_words(fold, res.fetch())
        ws = res.wordset(max_hypotheses)
    finally:
        res.close()
    pairs, record = _select_chunks(ws, rows_per_call, fold, opts)
    record.update(num_words=size["num_words"], n_unassigned=size["n_unassigned"])
    return pairs, record


def build_vocabulary(descset, num_image_voc=500, k=10, levels=6, seed=0, fold=None, **options):
    """Database::BuildVocabularyTree (SfM/src/database.cc:655-677) on a resident descriptor set: the tree is trained on every
    image_step-th image, image_step = max(n_images // num_image_voc, 1), by DescSet.train_voctree.  -> the resident `VocTree`
    (what select_pairs_from_descriptors takes).  With fold, `<fold>/voctree` is written in the reference's format; only then
    does the tree leave the device.  options: further arguments of DescSet.train_voctree (max_iters)."""
    step = max(len(descset.counts) // int(num_image_voc), 1)
    tree = descset.train_voctree(k=k, levels=levels, seed=seed, image_step=step, **options)
    if fold is not None:
        featurefiles.write_voctree(os.path.join(fold, "voctree"), **tree.fetch())
    return tree


def _select_chunks(ws, rows_per_call, fold, opts):
    """The chunk loop over a `Wordset`, which it closes."""
    try:
        n = ws.n_images
        got = ws.fetch(similarity=fold is not None)
        parts = [ws.select(r, min(rows_per_call, n - r), details=False, **opts) for r in range(0, n, rows_per_call)]
    finally:
        ws.close()
    pairs = np.concatenate([p["pairs"] for p in parts]).astype(np.int32).reshape(-1, 2)
    graph = [[] for _ in range(n)]
    for i, j in pairs:
        graph[i].append(int(j))
    record = dict(hyp_img=got["hyp_img"], hyp_sim=got["hyp_sim"], match_graph_init=graph,
                  **{k: np.concatenate([p[k] for p in parts]) for k in ("n_init", "n_inliers", "verdict")})
    if fold is not None:
        matchfiles.write_similarity_graph(fold, got["similarity"])
        matchfiles.write_init_match_graph(fold, graph)
    return pairs, record
