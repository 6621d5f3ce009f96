"""Generator of tests/golden/hransac_small.npz: a small mixed batch and the CPU restatement's homography RANSAC output
(tests/hransac_ref.cpp), polish off and on.  tests/test_gpu_homography.py::test_golden_fixture checks the GPU against it
without a compiler.  Run from the repository root: python tests/golden/make_hransac_golden.py"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import hransac_data as D  # noqa: E402


def main():
    rng = np.random.default_rng(20261016)
    parts = []
    for n, frac, planar in ((0, 0, True), (4, 0, True), (9, 0.2, True), (150, 0.3, True), (300, 0.5, False), (1100, 0.4, True)):
        parts.append(D.make_pair(rng, n, frac, planar=planar, noise=0.5)[:2])
    off, p1, p2 = D.batch(parts)
    with tempfile.TemporaryDirectory() as tmp:
        L = D.build_ref(tmp)
        out = dict(off=off, pt1=p1, pt2=p2, threshold=np.float64(4.0), seed=np.uint64(0x600D))
        for polish in (0, 1):
            H, inl, nin, ok = D.ref_hransac(L, off, p1, p2, threshold=4.0, polish=polish, seed=0x600D)
            out.update({"H%d" % polish: H, "inlier%d" % polish: inl, "n_inliers%d" % polish: nin, "ok%d" % polish: ok})
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "hransac_small.npz"), **out)


if __name__ == "__main__":
    main()
