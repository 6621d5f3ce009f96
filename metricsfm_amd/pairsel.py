"""Which image pairs to match (matching_type = "feature"): InitialMatchingGraph::match_graph_feature
(SfM/src/graph/initial_matching_graph.cc:164-294) through msfm_wordset_create + chunks of msfm_pair_select (include/msfm.h).

The sampler index of a hypothesis is its position in the msfm_pair_select call, so `rows_per_call` decides which samples a
pair sees: two runs agree bit for bit only with the same chunking."""
import numpy as np

from . import capi, matchfiles


def rule_k(n_images):
    """th_num_match (:168-169)."""
    return min(min(max(200, n_images // 10), n_images - 1), 500)


def select_pairs(ctx: capi.Context, n_features, words, num_words, keypoints, rows_per_call=64, fold=None, max_hypotheses=0, **opts):
    """-> (pairs [n_kept][2] int32, idx1-major: the `pairs` of DescSet.match_pairs; record).  words: per image the word id of
    every feature (None: the image has no words); keypoints: flat [sum of n_features][2].  opts: fields of
    msfm_pair_select_options / msfm_fransac_options.  record: dict of hyp_img, hyp_sim, n_init, n_inliers, verdict [n][K] and
    match_graph_init (per image the kept images).  With fold, similarity_graph.txt and init_match_graph.txt are written there."""
    ws = ctx.wordset(n_features, words, num_words, keypoints, max_hypotheses)
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
