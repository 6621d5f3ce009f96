"""Generator of tests/golden/relposef_golden.npz: one small mixed batch and every output of the CPU restatement of the
unknown-focal seed-pair arm (tests/relposef_ref.cpp) on it.  tests/test_relposef_ref.py checks that the restatement still
reproduces it, tests/test_gpu_relposef.py checks the GPU against it without a compiler.
Run from the repository root: python tests/golden/make_relposef_golden.py"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import relposef_data as D  # noqa: E402

NAMES = ("F", "f_ref", "f_cur", "E", "R", "t", "ok", "best_iter", "best_error", "n_candidates")
SIZES = [120, 0, 7, 8, 11, 16, 400, 40]
SEED, TIMES = 0x600D8, 150


def main():
    off, a, b = D.make_mixed_batch(20261016, SIZES)
    with tempfile.TemporaryDirectory() as tmp:
        L = D.build_ref(tmp)
        out = D.ref_relpose_8pt(L, off, a, b, ransac_times=TIMES, seed=SEED)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "relposef_golden.npz"), off=off, pts_ref=a, pts_cur=b,
                        seed=np.uint64(SEED), ransac_times=np.int32(TIMES), **dict(zip(NAMES, out)))


if __name__ == "__main__":
    main()
