"""The vocabulary-tree descent of msfm_descset_words restated in numpy (include/msfm.h states the semantics): every rounding is a
binary32 rounding, the eight partial sums are vectorised over features and nodes.  tests/words_ref.cpp is the same thing as a
literal scalar loop; tests/test_words_ref.py holds the two against each other.

A tree is a dict(k, block_n [nb], node_desc [nb][k][128] float32, node_link [nb][k] uint32, node_weight [nb][k] float32)."""
import numpy as np

LEAF = np.uint32(0x80000000)
BEST0 = np.float32(4294967296.0)
F32 = np.float32


def dist_avx(F, D):
    """[nf][128], [nn][128] -> [nf][nn]: eight partial sums, element i into partial i % 8 in ascending i as subtract, multiply,
    add; then ((s0+s1)+(s2+s3))+((s4+s5)+(s6+s7))."""
    F, D = np.asarray(F, F32), np.asarray(D, F32)
    with np.errstate(all="ignore"):
        d = F[:, None, :] - D[None, :, :]
        q = d * d
        s = np.zeros(q.shape[:2] + (8,), F32)
        for t in range(16):
            s = s + q[:, :, 8 * t:8 * t + 8]
        return ((s[..., 0] + s[..., 1]) + (s[..., 2] + s[..., 3])) + ((s[..., 4] + s[..., 5]) + (s[..., 6] + s[..., 7]))


def transform(tree, feats):
    """-> word_id [nf] int32 (-1: none), leaf_w [nf] float32 (0 without a word)."""
    feats = np.asarray(feats, F32).reshape(-1, 128)
    nf, k = len(feats), int(tree["k"])
    word, wt = np.full(nf, -1, np.int32), np.zeros(nf, F32)
    blk, go = np.zeros(nf, np.int64), np.ones(nf, bool)
    for _ in range(64):
        if not go.any():
            break
        for b in np.unique(blk[go]):
            idx = np.flatnonzero(go & (blk == b))
            N = int(tree["block_n"][b])
            d = dist_avx(feats[idx], tree["node_desc"][b, :N])
            ok = d < BEST0                      # NaN: False
            won = ok.any(axis=1)
            best = np.argmin(np.where(ok, d, np.inf), axis=1)   # the first of equal minima: strict < in node order
            link = tree["node_link"][b, best]
            leaf = (link & LEAF) != 0
            got = won & leaf
            word[idx[got]] = (link[got] & np.uint32(0x7FFFFFFF)).astype(np.int32)
            wt[idx[got]] = tree["node_weight"][b, best[got]]
            on = won & ~leaf & (link != 0)
            blk[idx[on]] = link[on]
            go[idx[~on]] = False
    assert not go.any(), "the tree has a cycle"
    return word, wt


def words_of_set(tree, descs, min_features=300):
    """What WordResult.fetch() and .size() return, as one dict."""
    n = len(descs)
    counts = np.array([len(d) for d in descs], np.int64)
    feat_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    has = (counts > min_features).astype(np.uint8)
    word_id = np.full(int(feat_off[-1]), -1, np.int32)
    image_max, bow_off = np.zeros(n, np.int32), np.zeros(n + 1, np.int32)
    bow_word, bow_weight, n_un = [], [], 0
    for i in range(n):
        if has[i]:
            w, wt = transform(tree, descs[i])
            word_id[feat_off[i]:feat_off[i + 1]] = w
            n_un += int((w < 0).sum())
            image_max[i] = max(0, int(w.max()))
            bag = {}
            for f in range(len(w)):            # feature order, from 0.0f
                if w[f] >= 0:
                    bag[int(w[f])] = F32(bag.get(int(w[f]), F32(0.0)) + wt[f])
            for wid in sorted(bag):
                bow_word.append(wid)
                bow_weight.append(bag[wid])
        bow_off[i + 1] = len(bow_word)
    return dict(feat_off=feat_off, has_words=has, word_id=word_id, image_max_id=image_max, bow_off=bow_off,
                bow_word=np.array(bow_word, np.int32), bow_weight=np.array(bow_weight, F32), num_words=int(image_max.max()) if n else 0,
                n_unassigned=n_un, n_images=n, n_features=int(feat_off[-1]), n_bow=len(bow_word))


ARRAYS = ("feat_off", "has_words", "word_id", "image_max_id", "bow_off", "bow_word", "bow_weight")
SCALARS = ("n_images", "n_features", "n_bow", "num_words", "n_unassigned")


def same(a, b):
    """Every array and count of two results equal, the weights bit for bit.  -> the first name that differs, or None."""
    for name in ARRAYS:
        x, y = np.asarray(a[name]), np.asarray(b[name])
        if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
            return name
    for name in SCALARS:
        if int(a[name]) != int(b[name]):
            return name
    return None
