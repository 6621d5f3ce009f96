"""Writes tests/golden/words_golden.npz: a small vocabulary tree (k = 4, three blocks deep, blocks of 2 .. 4 nodes), the
descriptors of three images (310, 40 and 305 features, integer-valued, stored as uint8), and the words, bags and maxima that
the numpy restatement tests/words_ref.py gives for them with min_features = 300.
    python -m tests.golden.make_words_golden"""
import os

import numpy as np

from tests import words_ref as R

LEAF = 0x80000000


def make():
    rng = np.random.Generator(np.random.PCG64(0x30d5601d))
    k, blocks, word = 4, [None], [0]

    def build(b, depth):
        nodes = []
        for i in range(int(rng.integers(2, 5))):
            d = rng.integers(0, 256, 128).astype(np.uint8)
            if depth == 3 or (depth == 2 and i == 0):
                word[0] += int(rng.integers(1, 3))
                nodes.append((d, LEAF | word[0], np.float32(rng.uniform(0.05, 5.0))))
            else:
                blocks.append(None)
                child = len(blocks) - 1
                nodes.append((d, child, np.float32(0.0)))
                build(child, depth + 1)
        blocks[b] = nodes

    build(0, 1)
    nb = len(blocks)
    tree = dict(k=k, block_n=np.array([len(b) for b in blocks], np.uint16), node_desc=np.zeros((nb, k, 128), np.uint8),
                node_link=np.zeros((nb, k), np.uint32), node_weight=np.zeros((nb, k), np.float32))
    for b, nodes in enumerate(blocks):
        for i, (d, link, w) in enumerate(nodes):
            tree["node_desc"][b, i], tree["node_link"][b, i], tree["node_weight"][b, i] = d, link, w
    descs = [rng.integers(0, 256, (s, 128)).astype(np.uint8) for s in (310, 40, 305)]
    want = R.words_of_set(dict(tree, node_desc=tree["node_desc"].astype(np.float32)), [d.astype(np.float32) for d in descs], 300)
    out = {"tree_" + name: v for name, v in tree.items()}
    out.update({"desc_%d" % i: d for i, d in enumerate(descs)})
    out.update({"want_" + name: want[name] for name in R.ARRAYS + R.SCALARS})
    return out


if __name__ == "__main__":
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "words_golden.npz")
    np.savez_compressed(path, **make())
    print(path, os.path.getsize(path), "bytes")
