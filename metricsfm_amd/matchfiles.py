"""The reference's on-disk match formats, so that matches produced by libmsfm can
be consumed by the unmodified incremental pipeline and vice versa.

  <output_fold>/<idx1>_match   binary, appended per accepted pair: int32 idx2, int32 n, int32[2n] (ptid1, ptid2)
                               (FineMatchingGraph::WriteOutMatches, SfM/src/graph/fine_matching_graph.cc:247-272;
                                read back by Graph::QueryMatch, SfM/src/graph.cc:92-137)
  <output_fold>/graph_matching.txt   text, N rows of N counts separated by ' ', each row ends with ' \\n'
                               (WriteOutMatchGraph, fine_matching_graph.cc:275-292; Graph::ReadinMatchingGraph, graph.cc:72-85)
  <fold>/feature/prior.txt     text, the prior F / H of SLAMGPS::FeatureMatching step 1: the camera count, then per camera
                               i a line with n and n lines `j F00 H00 F01 H01 ... F22 H22 ` (std::fixed, 12 decimals)
                               (SLAMGPS::WriteOutPriorInfo / ReadinPriorInfo, SfM/src/slam_gps.cc:1821-1885)
  <output_fold>/init_match_graph.txt   text: the image count, id_last (the last image whose row is final), then per image
                               `n j0 j1 ... ` - every number followed by one blank, the line too
                               (InitialMatchingGraph::WriteOutInitMatchGraph / ReadinInitMatchGraph, initial_matching_graph.cc:296-344)
  <output_fold>/similarity_graph.txt   text: N, then N rows of N floats as operator<< prints them (%g), each followed by one blank
                               (WriteOutSimilarityGraph / ReadinSimilarityGraph, initial_matching_graph.cc:357-392)
Native little-endian ints, as the reference writes them with ofstream::write.
"""
import os

import numpy as np

from . import _abi as A


def match_file(fold, idx1):
    return os.path.join(fold, "%d_match" % idx1)


def write_out_matches(fold, idx1, idx2, matches):
    """Append one record; like the reference, an empty match list writes nothing."""
    m = np.asarray(matches, dtype=np.int32).reshape(-1, 2)
    if len(m) == 0:
        return
    with open(match_file(fold, idx1), "ab") as f:
        np.array([idx2, len(m)], dtype=np.int32).tofile(f)
        np.ascontiguousarray(m).tofile(f)


def query_match(fold, idx):
    """-> (image_ids, [matches [n,2]]) in file order (Graph::QueryMatch, graph.cc:92-121)."""
    ids, out = [], []
    path = match_file(fold, idx)
    if not os.path.exists(path):
        return ids, out
    raw = np.fromfile(path, dtype=np.int32)
    p = 0
    while p + 2 <= len(raw):
        idx2, n = int(raw[p]), int(raw[p + 1])
        p += 2
        ids.append(idx2)
        out.append(raw[p:p + 2 * n].reshape(n, 2).copy())
        p += 2 * n
    return ids, out


def write_out_match_graph(fold, match_graph):
    g = np.asarray(match_graph, dtype=np.int64)
    with open(os.path.join(fold, "graph_matching.txt"), "wb") as f:
        for row in g:
            f.write(("".join("%d " % v for v in row) + "\n").encode())


def read_in_matching_graph(fold, n):
    vals = np.array(open(os.path.join(fold, "graph_matching.txt")).read().split(), dtype=np.int64)
    return vals.reshape(n, n)


def write_init_match_graph(fold, match_graph_init, id_last=None):
    """match_graph_init: per image the list of images to match it against; id_last defaults to the last image (:80)."""
    n = len(match_graph_init)
    with open(os.path.join(fold, "init_match_graph.txt"), "wb") as f:
        f.write(("%d\n%d\n" % (n, n - 1 if id_last is None else id_last)).encode())
        for row in match_graph_init:
            f.write(("%d " % len(row) + "".join("%d " % int(v) for v in row) + "\n").encode())


def read_init_match_graph(fold):
    """-> (match_graph_init as a list of int lists, id_last)."""
    tok = open(os.path.join(fold, "init_match_graph.txt")).read().split()
    n, id_last = int(tok[0]), int(tok[1])
    rows, p = [], 2
    for _ in range(n):
        k = int(tok[p])
        rows.append([int(v) for v in tok[p + 1:p + 1 + k]])
        p += 1 + k
    return rows, id_last


def write_similarity_graph(fold, similarity):
    """similarity [n][n]; the reference keeps the counts in float and prints them with the stream's default format."""
    s = np.asarray(similarity, dtype=np.float32)
    with open(os.path.join(fold, "similarity_graph.txt"), "wb") as f:
        f.write(("%d\n" % len(s)).encode())
        for row in s:
            f.write(("".join("%g " % float(v) for v in row) + "\n").encode())


def read_similarity_graph(fold):
    tok = open(os.path.join(fold, "similarity_graph.txt")).read().split()
    n = int(tok[0])
    return np.array(tok[1:1 + n * n], dtype=np.float32).reshape(n, n)


def codes_to_matches(code):
    """(ptid1, ptid2) lists of the reference loop (fine_matching_graph.cc:116-133) from msfm_match_pairs codes."""
    code = np.asarray(code)
    m2 = np.nonzero(code >= 0)[0].astype(np.int32)
    m1 = (code[m2] & A.MSFM_MATCH_ID_MASK).astype(np.int32)
    good = (code[m2] & A.MSFM_MATCH_GOOD) != 0
    in_all = (code[m2] & A.MSFM_MATCH_NOT_ALL) == 0      # the two ratio tests are independent (:118-130)
    allm = np.column_stack([m1, m2])
    return allm[good], allm[in_all]


def write_prior_info(path, n_cams, pairs, F, H):
    """SLAMGPS::WriteOutPriorInfo (slam_gps.cc:1821-1847) of the kept pairs of step 1: pairs [k][2] = (i, j) grouped by i
    (the order msfm_slam_priors returns), F / H [k][3][3]."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    F = np.asarray(F, dtype=np.float64).reshape(-1, 9)
    H = np.asarray(H, dtype=np.float64).reshape(-1, 9)
    rows = [[] for _ in range(int(n_cams))]
    for (i, j), f, h in zip(pairs, F, H):
        rows[int(i)].append((int(j), f, h))
    out = ["%d\n" % int(n_cams)]
    for r in rows:
        out.append("%d\n" % len(r))
        for j, f, h in r:
            out.append("%d " % j + "".join("%.12f %.12f " % (f[k], h[k]) for k in range(9)) + "\n")
    with open(path, "w") as fh:
        fh.write("".join(out))


def read_prior_info(path):
    """SLAMGPS::ReadinPriorInfo (slam_gps.cc:1849-1885) -> (n_cams, pairs [k][2], F [k][3][3], H [k][3][3]) in file order."""
    tok = open(path).read().split()
    p = 0
    n_cams = int(tok[p]); p += 1
    pairs, F, H = [], [], []
    for i in range(n_cams):
        n = int(tok[p]); p += 1
        for _ in range(n):
            j = int(tok[p]); p += 1
            v = np.array(tok[p:p + 18], dtype=np.float64); p += 18
            pairs.append((i, j)); F.append(v[0::2].reshape(3, 3)); H.append(v[1::2].reshape(3, 3))
    return (n_cams, np.array(pairs, dtype=np.int32).reshape(-1, 2), np.array(F).reshape(-1, 3, 3), np.array(H).reshape(-1, 3, 3))
