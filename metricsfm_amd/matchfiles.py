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
