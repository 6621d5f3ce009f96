"""msfm_descset_voctree_train restated in numpy (include/msfm.h states the definitions): node by node, every distance in the
binary32 form of words_ref.dist_avx, every sum a 64-bit integer.  tests/voctrain_ref.cpp is the same thing as a literal scalar
loop; tests/test_voctrain_ref.py holds the two against each other.

train() -> (tree, stats): tree is the dict VocTree.fetch() returns (k, block_n, node_desc, node_link, node_weight, block_leaf,
block_parent), stats the dict of VocTree.stats without host_waits."""
import numpy as np

from . import words_ref as R

F32 = np.float32
LEAF = 0x80000000
MASK = (1 << 64) - 1
SALT = 0x766F637472616E31
MAX_FEATURES = 1 << 23
BOUND_BITS = int(np.array([2896.0], F32).view(np.uint32)[0])


def _next(x):
    """splitmix64: -> (advanced state, output)"""
    x = (x + 0x9E3779B97F4A7C15) & MASK
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return x, z ^ (z >> 31)


def draw(seed, level, ordinal, j):
    _, h = _next((seed ^ SALT) & MASK)
    _, h = _next(h ^ ((level << 40) | ordinal))
    return _next(h ^ j)[1]


def shifts(X):
    """-> (weight_shift, sum_shift) of a sample, ValueError for values the call refuses."""
    maxbits = int((np.ascontiguousarray(X, F32).view(np.uint32) & np.uint32(0x7FFFFFFF)).max())
    if maxbits >= 0x7F800000:
        raise ValueError("a sampled value is not finite")
    if maxbits >= BOUND_BITS:
        raise ValueError("a sampled value has |value| >= 2896")
    e = (maxbits >> 23) - 126
    return 40 - (9 + 2 * e), 39 - e


def dist(F, D):
    """[nf][128], [nn][128] -> [nf][nn] float32, the descent's form, in slices that keep the temporaries small."""
    F, D = np.asarray(F, F32).reshape(-1, 128), np.asarray(D, F32).reshape(-1, 128)
    step = max(1, 4096 // max(1, len(D)))
    return np.concatenate([R.dist_avx(F[a:a + step], D) for a in range(0, len(F), step)]) if len(F) else np.zeros((0, len(D)), F32)


def nearest(F, C):
    """strict < in centre order: the first of equal minima"""
    return np.argmin(dist(F, C), axis=1)


def seed_centres(X, mem, k, wshift, seed, level, ordinal):
    """-> the members (feature numbers) chosen as centres, 1 .. k of them"""
    m = len(mem)
    chosen = [int(mem[draw(seed, level, ordinal, 0) % m])]
    mind = dist(X[mem], X[chosen[-1]])[:, 0]
    for j in range(1, k):
        w = np.trunc(mind.astype(np.float64) * 2.0 ** wshift).astype(np.uint64)
        W = int(w.sum(dtype=np.uint64))
        if W == 0:
            break
        r = draw(seed, level, ordinal, j) % W
        first = int(np.searchsorted(np.cumsum(w, dtype=np.uint64), np.uint64(r), side="right"))   # the first prefix above r
        chosen.append(int(mem[first]))
        mind = np.minimum(mind, dist(X[mem], X[chosen[-1]])[:, 0])
    return chosen


def recompute(X, mem, a, C, S):
    """The centres of assignment a: the mean of q(x) = trunc(x 2^S) as int64, divided in binary64; an empty cluster keeps its
    centre.  -> (centres, counts)"""
    C = C.copy()
    q = np.trunc(X[mem].astype(np.float64) * 2.0 ** S).astype(np.int64)
    counts = np.bincount(a, minlength=len(C))
    for c in np.flatnonzero(counts):
        total = q[a == c].sum(axis=0, dtype=np.int64)
        C[c] = ((total.astype(np.float64) / np.float64(counts[c])) * 2.0 ** -S).astype(F32)
    return C, counts


def iterate(X, mem, chosen, max_iters, S, trace=None):
    """-> (centres, final assignment, counts, iterations, capped)"""
    C = X[chosen].copy()
    prev, counts = None, None
    for it in range(1, max_iters + 1):
        a = nearest(X[mem], C)
        same = prev is not None and np.array_equal(a, prev)
        if not same:            # (an unchanged assignment: the centres already are its means)
            C, counts = recompute(X, mem, a, C, S)
        if trace is not None:
            trace.append(dict(it=it, mem=mem, assign=a.copy(), centres=C.copy()))
        prev = a
        if same:
            return C, a, counts, it, False
    return C, prev, counts, max_iters, True


def sample(descs, image_step):
    imgs = [np.asarray(d, F32).reshape(-1, 128) for d in descs[::image_step]]
    return np.concatenate(imgs) if imgs else np.zeros((0, 128), F32), len(imgs)


def train(descs, k=10, levels=6, max_iters=11, image_step=1, seed=0, trace=None):
    """trace: a list that receives, per iterated node and iteration, dict(level, ordinal, it, mem, assign, centres)."""
    if not (2 <= k <= 64 and 1 <= levels <= 32 and max_iters >= 1 and image_step >= 1):
        raise ValueError("options out of range")
    X, n_img = sample(descs, image_step)
    M = len(X)
    if M == 0 or M > MAX_FEATURES:
        raise ValueError("no sampled feature, or more than 2^23")
    wshift, S = shifts(X)
    st = dict(n_features=M, n_images=n_img, weight_shift=wshift, sum_shift=S, level_nodes=[], level_split=[], level_max_iters=[], level_capped=[])
    blocks, parents = [], []        # per block: list of (descriptor, link, weight); parent block
    nodes, node_parent = [np.arange(M)], [0]
    word, base = 0, 0
    for level in range(levels):
        if not nodes:
            break
        nn = len(nodes)
        nxt, nxt_parent = [], []
        split, most, capped = 0, 0, 0
        for o, mem in enumerate(nodes):
            rows = []           # (descriptor, members or None for a leaf)
            if len(mem) <= k:
                rows = [(X[i], None) for i in mem]
            else:
                chosen = seed_centres(X, mem, k, wshift, seed, level, o)
                if len(chosen) == 1:
                    rows = [(X[chosen[0]], None)]
                else:
                    tr = [] if trace is not None else None
                    C, a, counts, its, cap = iterate(X, mem, chosen, max_iters, S, tr)
                    if trace is not None:
                        trace.extend(dict(t, level=level, ordinal=o) for t in tr)
                    split, most, capped = split + 1, max(most, its), capped + int(cap)
                    for c in range(len(C)):
                        if counts[c] > 0:
                            leaf = level == levels - 1 or counts[c] == 1
                            rows.append((C[c], None if leaf else mem[a == c]))
            blk = []
            for d, members in rows:
                if members is None:
                    blk.append((d, LEAF | word, F32(1.0)))
                    word += 1
                else:
                    blk.append((d, base + nn + len(nxt), F32(0.0)))
                    nxt.append(members)
                    nxt_parent.append(base + o)
            blocks.append(blk)
            parents.append(node_parent[o])
        for name, v in (("level_nodes", nn), ("level_split", split), ("level_max_iters", most), ("level_capped", capped)):
            st[name].append(v)
        base += nn
        nodes, node_parent = nxt, nxt_parent
    nb = len(blocks)
    tree = dict(k=k, block_n=np.array([len(b) for b in blocks], np.uint16), node_desc=np.zeros((nb, k, 128), F32),
                node_link=np.zeros((nb, k), np.uint32), node_weight=np.zeros((nb, k), F32),
                block_leaf=np.array([all(l & LEAF for _, l, _ in b) for b in blocks], np.uint16), block_parent=np.array(parents, np.uint32))
    for b, blk in enumerate(blocks):
        for i, (d, link, w) in enumerate(blk):
            tree["node_desc"][b, i], tree["node_link"][b, i], tree["node_weight"][b, i] = d, link, w
    st.update(n_blocks=nb, n_leaves=word, depth=len(st["level_nodes"]))
    return tree, st


TREE_ARRAYS = ("block_n", "node_desc", "node_link", "node_weight", "block_leaf", "block_parent")
STATS = ("n_features", "n_leaves", "n_images", "n_blocks", "depth", "weight_shift", "sum_shift", "level_nodes", "level_split",
         "level_max_iters", "level_capped")


def same_tree(a, b):
    """Every array of two trees equal, the descriptors bit for bit.  -> the first name that differs, or None."""
    if int(a["k"]) != int(b["k"]):
        return "k"
    for name in TREE_ARRAYS:
        x, y = np.asarray(a[name]), np.asarray(b[name])
        if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
            return name
    return None


def same_stats(want, got):
    for name in STATS:
        if (list(want[name]) != list(got[name])) if name.startswith("level_") else (int(want[name]) != int(got[name])):
            return name
    return None


def max_host_waits(st):
    """The bound include/msfm.h states: the value scan, two per level, one per iteration of a level (asked at least once: a level
    whose larger nodes all end their seeding with one centre iterates nothing), the end."""
    return 2 + sum(2 + max(1, m) for m in st["level_max_iters"])
