"""The seeded scenes of the visual-word tests (tests/test_words_ref.py, tests/test_gpu_words.py): trees, images, planted
near-ties, bags whose sums depend on the order, degenerate rows.  The conditions that make a scene a test - enough planted
features on which another arithmetic picks another node, enough bags whose sum depends on the order - are asserted HERE, on
the CPU, on the data: they say nothing about the code under test."""
import functools
import os
import subprocess

import numpy as np

from metricsfm_amd import scene

from . import words_ref as R

F32 = np.float32
LEAF = 0x80000000
SIZES = (0, 1, 7, 8, 9, 63, 64, 65, 300, 301, 1000)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rng(salt):
    return np.random.Generator(np.random.PCG64(scene.SEED_BASE + 0x30d5 + salt))


def _tree(k, blocks):
    """blocks: list of lists of (desc [128], link, weight) -> tree dict (rows past N: zeros)."""
    nb = len(blocks)
    t = dict(k=k, block_n=np.array([len(b) for b in blocks], np.uint16), node_desc=np.zeros((nb, k, 128), F32),
             node_link=np.zeros((nb, k), np.uint32), node_weight=np.zeros((nb, k), F32))
    for b, nodes in enumerate(blocks):
        for i, (d, link, w) in enumerate(nodes):
            t["node_desc"][b, i], t["node_link"][b, i], t["node_weight"][b, i] = d, link, w
    return t


def tree_stats(t):
    """-> (sizes of the reached blocks, depths at which leaves sit, blocks on the longest path)."""
    sizes, leaf_depths, todo, deepest = set(), set(), [(0, 1)], 1
    while todo:
        b, depth = todo.pop()
        deepest = max(deepest, depth)
        sizes.add(int(t["block_n"][b]))
        for i in range(int(t["block_n"][b])):
            link = int(t["node_link"][b, i])
            if link & LEAF:
                leaf_depths.add(depth)
            elif link:
                todo.append((link, depth + 1))
    return sizes, leaf_depths, deepest


@functools.lru_cache(maxsize=None)
def ragged_tree():
    """k = 10: blocks of 1 .. 10 nodes, leaves at depths 1 .. 4, node 7 of the root links block 0 (the descent stops there without
    a word), nodes 2 and 5 of the block under root node 1 carry that node's descriptor (the lower wins), word ids with gaps and
    weights of mixed size."""
    rng = _rng(1)
    blocks = [None]
    next_word = [3]

    def leaf():
        next_word[0] += int(rng.integers(1, 4))
        return LEAF | next_word[0], F32(rng.uniform(0.01, 9.0))

    def make(b, depth, n_nodes):
        nodes = []
        for i in range(n_nodes):
            d = rng.integers(0, 256, 128).astype(F32)
            if b == 0 and i == 7:
                nodes.append((d, 0, F32(0.5)))                      # the `id != 0` quirk
            elif depth == 4 or (i % 3 == 0 and not (b == 0 and i > 1)):
                nodes.append((d,) + leaf())
            else:
                blocks.append(None)
                child = len(blocks) - 1
                nodes.append((d, child, F32(0.0)))
                make(child, depth + 1, 11 - i if depth == 1 else 1 + (child - 1) % 10 if depth < 3 else int(rng.integers(1, 11)))
        blocks[b] = nodes

    make(0, 1, 10)
    d2, dup = blocks[0][1][0], blocks[0][1][1]          # root node 1 and its block of 10 nodes
    for i in (2, 5):
        blocks[dup][i] = (d2.copy(),) + blocks[dup][i][1:]
    t = _tree(10, blocks)
    sizes, leaf_depths, deepest = tree_stats(t)
    assert sizes == set(range(1, 11)) and leaf_depths == {1, 2, 3, 4} and deepest == 4, (sizes, leaf_depths, deepest)
    return t


@functools.lru_cache(maxsize=None)
def k3_tree():
    """k = 3, six blocks deep, full: 364 blocks, 729 words."""
    rng = _rng(2)
    blocks, word = [None], [0]

    def make(b, depth):
        nodes = []
        for _ in range(3):
            d = rng.integers(0, 256, 128).astype(F32)
            if depth == 6:
                nodes.append((d, LEAF | word[0], F32(rng.uniform(0.1, 2.0))))
                word[0] += 1
            else:
                blocks.append(None)
                child = len(blocks) - 1
                nodes.append((d, child, F32(0.0)))
                make(child, depth + 1)
        blocks[b] = nodes

    make(0, 1)
    t = _tree(3, blocks)
    assert tree_stats(t)[1:] == ({6}, 6) and len(blocks) == 364
    return t


@functools.lru_cache(maxsize=None)
def k64_tree():
    """k = 64, one block: 64 leaves that share 12 word ids, with weights from 1e-3 to 1e3 - a word's bag entry sums weights of
    different sizes, so the order of the additions shows."""
    rng = _rng(3)
    nodes = [(rng.integers(0, 256, 128).astype(F32), LEAF | (i % 12), F32(10.0 ** rng.uniform(-3, 3))) for i in range(64)]
    return _tree(64, [nodes])


def random_images(sizes, salt):
    rng = _rng(salt)
    return [rng.integers(0, 256, (s, 128)).astype(F32) for s in sizes]


@functools.lru_cache(maxsize=None)
def ragged_images():
    """Images of SIZES features on the ragged tree.  The last image also holds: a copy of a leaf node (distance 0), 10 rows that meet
    the two equal nodes (asserted: the lower one decides their word), 20 rows next to
    root node 7 (the link to block 0), a row with a NaN, one with an infinity, one of 1e6 throughout (every distance >= 2^32).
    -> (images, rows of the last image that must end without a word)"""
    t = ragged_tree()
    imgs = random_images(SIZES, 4)
    rng = _rng(5)
    last = imgs[-1]
    last[10] = t["node_desc"][0, 0]                  # node 0 of the root is a leaf
    stop = np.arange(100, 120)
    last[stop] = t["node_desc"][0, 7] + rng.integers(-2, 3, (20, 128)).astype(F32)
    last[300:310] = t["node_desc"][0, 1] + rng.integers(-1, 2, (10, 128)).astype(F32)   # the tie of nodes 2 and 5 under root node 1
    dup = int(t["node_link"][0, 1])
    far = {i: dict(t, node_desc=t["node_desc"].copy()) for i in (2, 5)}
    for i in (2, 5):
        far[i]["node_desc"][dup, i] += 1000
    w = R.transform(t, last[300:310])[0]
    assert np.array_equal(w, R.transform(far[5], last[300:310])[0]) and not np.array_equal(w, R.transform(far[2], last[300:310])[0])
    last[200, 5] = np.nan
    last[201, 77] = np.inf
    last[202] = 1e6
    return imgs, np.concatenate([stop, [200, 201, 202]])


# ---- planted near-ties ----
def _winner(dA, dB, a_first):
    """Node order decides a tie: the winner is B only if it is strictly nearer, or equal and first.  -> True where B wins."""
    return np.where(a_first, dB < dA, dB <= dA)


def dist_f64(F, D):
    d = F.astype(np.float64) - D.astype(np.float64)
    return (d * d).sum(axis=1)


def dist_seq32(F, D):
    d = F - D
    q = d * d
    s = np.zeros(len(F), F32)
    for i in range(128):
        s = s + q[:, i]
    return s


def dist_fused(F, D):
    """The AVX order with a fused multiply-add per step: float32(float64(x) * float64(x) + float64(s)).  Exact in binary64 for the
    planted values (48-bit products, sums within 53 bits), so one rounding per step."""
    d = (F - D).astype(np.float64)
    s = np.zeros((len(F), 8), F32)
    for t in range(16):
        x = d[:, 8 * t:8 * t + 8]
        s = (x * x + s.astype(np.float64)).astype(F32)
    return ((s[:, 0] + s[:, 1]) + (s[:, 2] + s[:, 3])) + ((s[:, 4] + s[:, 5]) + (s[:, 6] + s[:, 7]))


def dist_avx_rows(F, D):
    return np.array([R.dist_avx(F[i:i + 1], D[i:i + 1])[0, 0] for i in range(len(F))], F32)


@functools.lru_cache(maxsize=None)
def planted():
    """k = 64, two blocks deep: 8 root nodes (random centres), under each a block of 32 pairs of leaves (A, B).  Pair p of a block
    belongs to one feature f: A = f + d, B = f + P(d), with d in multiples of 1/4096 below 8 in size, f integer and P a random
    permutation of the 128 elements (it mixes the residues mod 8).  f - A and f - B are exact and hold the same 128 values, so
    the real distances are equal; their squares need 30 bits, so the binary32 sums depend on the order.  Which of A and B comes
    first in the block is random.  Asserted: on at least 16 features the AVX order picks another node than binary64, than one
    sequential binary32 accumulator, and than the fused form.
    -> dict(tree, images (one image: the 256 planted features and 64 fillers), n_planted, differs = counts for the three)"""
    for attempt in range(8):
        rng = _rng(100 + attempt)
        centres = rng.integers(40, 216, (8, 128)).astype(F32)
        blocks = [[(centres[c], 1 + c, F32(0.0)) for c in range(8)]]
        feats, FA, FB, a_first = [], [], [], []
        word = 0
        for c in range(8):
            nodes = []
            for p in range(32):
                f = centres[c] + rng.integers(-20, 21, 128).astype(F32)
                d = (rng.integers(-32767, 32768, 128) / 4096.0).astype(F32)
                A, B = f + d, f + d[rng.permutation(128)]
                first = bool(rng.integers(0, 2))
                for node in ((A, B) if first else (B, A)):
                    nodes.append((node, LEAF | word, F32(rng.uniform(0.5, 1.5))))
                    word += 1
                feats.append(f), FA.append(A), FB.append(B), a_first.append(first)
            blocks.append(nodes)
        F, A, B, a_first = np.array(feats, F32), np.array(FA, F32), np.array(FB, F32), np.array(a_first)
        assert np.array_equal(np.sort((F - A).astype(np.float64), axis=1), np.sort((F - B).astype(np.float64), axis=1))   # exact, same values
        avx = _winner(dist_avx_rows(F, A), dist_avx_rows(F, B), a_first)
        differs = {name: int((avx != _winner(fn(F, A), fn(F, B), a_first)).sum())
                   for name, fn in (("binary64", dist_f64), ("sequential", dist_seq32), ("fused", dist_fused))}
        if min(differs.values()) >= 16:
            break
    assert min(differs.values()) >= 16, differs
    assert np.array_equal(dist_f64(F, A), dist_f64(F, B))   # binary64 sees the tie
    fillers = centres[rng.integers(0, 8, 64)] + rng.integers(-20, 21, (64, 128)).astype(F32)
    return dict(tree=_tree(64, blocks), images=[np.concatenate([F, fillers]).astype(F32)], n_planted=len(F), differs=differs)


@functools.lru_cache(maxsize=None)
def bag_images():
    """Two images on k64_tree: features next to random leaves, about 80 per word.  Asserted: at least 8 bag entries collect 50 or
    more features and sum to another binary32 value in feature order than with the weights sorted."""
    t = k64_tree()
    rng = _rng(6)
    imgs = []
    for s in (1000, 350):
        leaf = rng.integers(0, 64, s)
        imgs.append((t["node_desc"][0, leaf] + rng.integers(-3, 4, (s, 128))).astype(F32))
    w, wt = R.transform(t, imgs[0])
    order_matters = 0
    for wid in np.unique(w):
        ws = wt[w == wid]
        if len(ws) >= 50:
            a = F32(0.0)
            for x in ws:
                a = F32(a + x)
            b = F32(0.0)
            for x in np.sort(ws):
                b = F32(b + x)
            order_matters += int(a != b)
    assert order_matters >= 8, order_matters
    return imgs


def scenes():
    """name -> (tree, images, min_features)"""
    rimgs, _ = ragged_images()
    p = planted()
    return {
        "ragged": (ragged_tree(), rimgs, 300),
        "ragged_all": (ragged_tree(), rimgs, 0),
        "k3": (k3_tree(), random_images((65, 301, 400), 7), 300),
        "k64": (k64_tree(), bag_images(), 300),
        "planted": (p["tree"], p["images"], 300),
    }


@functools.lru_cache(maxsize=None)
def expected(name):
    tree, imgs, mf = scenes()[name]
    return R.words_of_set(tree, imgs, mf)


# ---- the C++ restatement ----
def build_ref_cpp(exe):
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "words_ref.cpp"), "-o", str(exe)])


def run_ref_cpp(exe, tmp, tree, imgs, min_features):
    """-> (the result dict of words_ref.words_of_set, seconds of the descent)"""
    fin, fout = os.path.join(str(tmp), "words_in.bin"), os.path.join(str(tmp), "words_out.bin")
    n = len(imgs)
    with open(fin, "wb") as fh:
        np.array([tree["k"], len(tree["block_n"]), n, min_features], np.int32).tofile(fh)
        tree["block_n"].astype(np.int32).tofile(fh)
        np.ascontiguousarray(tree["node_desc"], F32).tofile(fh)
        np.ascontiguousarray(tree["node_link"], np.uint32).tofile(fh)
        np.ascontiguousarray(tree["node_weight"], F32).tofile(fh)
        np.array([len(d) for d in imgs], np.int32).tofile(fh)
        for d in imgs:
            np.ascontiguousarray(d, F32).tofile(fh)
    out = subprocess.check_output([str(exe), fin, fout], text=True)
    seconds = float(out.split(",")[1].split()[0])
    total = sum(len(d) for d in imgs)
    with open(fout, "rb") as fh:
        n_un, num_words, n_bow = np.fromfile(fh, np.int32, 3)
        has = np.fromfile(fh, np.int32, n).astype(np.uint8)
        word = np.fromfile(fh, np.int32, total)
        imax = np.fromfile(fh, np.int32, n)
        boff = np.fromfile(fh, np.int32, n + 1)
        bword = np.fromfile(fh, np.int32, n_bow)
        bwt = np.fromfile(fh, F32, n_bow)
    feat_off = np.concatenate([[0], np.cumsum([len(d) for d in imgs])]).astype(np.int32)
    return dict(feat_off=feat_off, has_words=has, word_id=word, image_max_id=imax, bow_off=boff, bow_word=bword, bow_weight=bwt,
                num_words=int(num_words), n_unassigned=int(n_un), n_images=n, n_features=total, n_bow=int(n_bow)), seconds


# ---- a tree and descriptors that reproduce given words (the pair-selection scene) ----
def tree_for_words(n_words, salt=8):
    """k = 32, two blocks deep, leaf w = word w.  -> (tree, desc_of_word [n_words][128]): a feature that is a copy of its word's
    leaf descends to it (asserted by the caller through the restatement)."""
    rng = _rng(salt)
    n_groups = (n_words + 31) // 32
    assert n_groups <= 32
    centres = rng.integers(40, 216, (n_groups, 128)).astype(F32)
    blocks = [[(centres[c], 1 + c, F32(0.0)) for c in range(n_groups)]]
    desc = np.zeros((n_words, 128), F32)
    for c in range(n_groups):
        nodes = []
        for w in range(32 * c, min(n_words, 32 * c + 32)):
            desc[w] = centres[c] + rng.integers(-30, 31, 128).astype(F32)
            nodes.append((desc[w], LEAF | w, F32(rng.uniform(0.5, 1.5))))
        blocks.append(nodes)
    return _tree(32, blocks), desc
