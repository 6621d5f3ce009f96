"""Generator of tests/golden/epnpf_golden.npz: three images of 40-120 correspondences, the reference's sweep options
(350 candidate focal lengths x 200 samples) and every output of the CPU reference (tests/epnpf_ref.py).
tests/test_gpu_epnpf.py::test_golden_fixture checks the GPU against it, tests/test_epnpf_ref.py that it still reproduces.
Run from the repository root: python tests/golden/make_epnpf_golden.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import epnpf_ref  # noqa: E402
from tests.twoview import make_pnp_batch  # noqa: E402

KEYS = ("f", "R", "t", "errors", "avg_error", "best_step", "best_iter", "step_error")
SEED = 0x600DF


def inputs():
    off, X, x, _, _ = make_pnp_batch(20261016, [40, 75, 120], outlier_frac=0.15, noise=0.5, f=4800.0)
    return off, X, x, np.array([4000.0, 5760.0, 3000.0])   # 1.2 * max(w, h) of three sensors; true ratios 1.2, 0.83, 1.6


def main():
    from oracle import oracle as O
    O.build()
    off, X, x, f_init = inputs()
    out = dict(off=off, X=X, x=x, f_init=f_init, seed=np.uint64(SEED))
    out.update(zip(KEYS, epnpf_ref.epnpf_sweep(O, off, X, x, f_init, seed=SEED)))
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "epnpf_golden.npz"), **out)


if __name__ == "__main__":
    main()
