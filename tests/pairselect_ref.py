"""Sequential restatement of the pair selection of the reference, steps 1-5 of the msfm.h section "Which image pairs to
match": plain Python, dicts and sorted lists, one function per reference function, loops as the reference writes them.

  keep_unique_vector        SfM/src/utils/basic_funcs.h:127-152
  keep_unique_idx_vector    SfM/src/utils/basic_funcs.cc:380-408
  generate_inverted_file    SfM/src/graph/similarity_graph.cc:88-117
  similarity_graph_inv_file SfM/src/graph/similarity_graph.cc:47-86
  th_num_match, hypotheses, pt_word_map, join   SfM/src/graph/initial_matching_graph.cc:168-169, :216-231, :188-203, :242-253

Two places where the reference leaves the result to an unstable std::sort are fixed as the library fixes them: the feature of a
repeated word is the lowest index, and equal similarity goes to the lower image id."""
import numpy as np


def keep_unique_vector(data):
    """basic_funcs.h:127-152.  The first element is compared with itself, so the first group is never unique; the group that
    is open when the loop ends is never pushed."""
    data = sorted(data)
    out = []
    v = data[0]
    is_unique = True
    for x in data:
        if x != v:
            if is_unique:
                out.append(v)
            v = x
            is_unique = True
        else:
            is_unique = False
    return out


def keep_unique_idx_vector(data):
    """basic_funcs.cc:380-408.  Pushes the index of the element that OPENS a group when the group before it was unique."""
    data_new = sorted(((i, w) for i, w in enumerate(data)), key=lambda p: (p[1], p[0]))   # (:388; ties: the lowest index first)
    unique_idx = []
    is_unique = True
    v = data_new[0][1]
    for first, second in data_new:
        if second != v:
            if is_unique:
                unique_idx.append(first)
            v = second
            is_unique = True
        else:
            is_unique = False
    return unique_idx


def generate_inverted_file(words, num_words):
    """similarity_graph.cc:88-117.  words[i]: the word ids of image i, or None / empty."""
    inverted_file = [[] for _ in range(num_words)]
    for i, w in enumerate(words):
        if w is not None and len(w):
            for wid in keep_unique_vector([int(x) for x in w]):
                inverted_file[wid].append(i)
    th_bin_size = num_words // 100
    for b in inverted_file:
        if b and len(b) > th_bin_size:
            b.clear()
    return inverted_file


def similarity_graph_inv_file(words, num_words):
    """similarity_graph.cc:47-86 -> int32 [n][n]."""
    n = len(words)
    S = np.zeros((n, n), dtype=np.int32)
    for b in generate_inverted_file(words, num_words):
        for m in range(len(b) - 1):
            for k in range(m + 1, len(b)):
                S[b[m], b[k]] += 1
                S[b[k], b[m]] += 1
    return S


def th_num_match(num_imgs):
    """initial_matching_graph.cc:168-169."""
    k = min(max(200, num_imgs // 10), num_imgs - 1)
    return 500 if k > 500 else k


def hypotheses(S, i, K):
    """:216-231 -> (images, similarities) of the first K."""
    sim_sort = [(j, int(S[i][j])) for j in range(len(S)) if j != i]
    sim_sort.sort(key=lambda p: (-p[1], p[0]))
    return [p[0] for p in sim_sort[:K]], [p[1] for p in sim_sort[:K]]


def pt_word_map(w):
    """:188-203 -> dict word -> feature."""
    m = {}
    if w is None or not len(w):
        return m
    w = [int(x) for x in w]
    for idx in keep_unique_idx_vector(w):
        m.setdefault(w[idx], idx)   # (std::map::insert keeps the first; the words of two groups differ anyway)
    return m


def join(map1, map2):
    """:242-253 -> [(feature of image 1, feature of image 2)] in ascending word order (std::map iteration)."""
    return [(map1[w], map2[w]) for w in sorted(map1) if w in map2]


def match_graph_feature(words, num_words, K):
    """Everything before the verification: S, hyp_img / hyp_sim [n][K], the word tables, and per (row, slot) the join."""
    n = len(words)
    S = similarity_graph_inv_file(words, num_words)
    maps = [pt_word_map(w) for w in words]
    hyp_img, hyp_sim = np.zeros((n, K), np.int32), np.zeros((n, K), np.int32)
    joins = []
    for i in range(n):
        hyp_img[i], hyp_sim[i] = hypotheses(S, i, K)
        joins.append([join(maps[i], maps[int(j)]) for j in hyp_img[i]])
    return dict(similarity=S, hyp_img=hyp_img, hyp_sim=hyp_sim, maps=maps, joins=joins)


def tables_flat(maps):
    """The layout of msfm_wordset_fetch: map_off [n + 1], map_word, map_feat."""
    off, word, feat = [0], [], []
    for m in maps:
        for w in sorted(m):
            word.append(w)
            feat.append(m[w])
        off.append(len(word))
    return np.array(off, np.int32), np.array(word, np.int32), np.array(feat, np.int32)


def problem_list(joins, rows, keypoints, feat_off, hyp_img):
    """The arguments of one fundamental-RANSAC batch for the given rows: offsets, matches [..][2], pt1, pt2."""
    off, matches, p1, p2 = [0], [], [], []
    for i in rows:
        for s, jn in enumerate(joins[i]):
            j = int(hyp_img[i][s])
            for f1, f2 in jn:
                matches.append((f1, f2))
                p1.append(keypoints[feat_off[i] + f1])
                p2.append(keypoints[feat_off[j] + f2])
            off.append(len(matches))
    return (np.array(off, np.int32), np.array(matches, np.int32).reshape(-1, 2), np.array(p1, np.float32).reshape(-1, 2),
            np.array(p2, np.float32).reshape(-1, 2))


def gates(n_init, ok, n_inliers, th_init_matches=30, th_inliers=20):
    """:254, :270, :274 -> verdict per hypothesis."""
    v = np.zeros(len(n_init), np.uint8)
    for h in range(len(n_init)):
        v[h] = 1 if n_init[h] < th_init_matches else 2 if not ok[h] else 3 if not n_inliers[h] > th_inliers else 0
    return v
