"""Generator of tests/golden/localizepose_golden.npz: every output of the sequential restatement tests/localizepose_ref.py over
the oracle on tests/localizepose_data.py::ring_case, once with every row on the known-focal arm and once mixed with the sweep.
tests/test_gpu_localizepose.py::test_committed_answer checks the GPU against it, tests/test_localizepose_ref.py that it still
reproduces.  Run from the repository root: python tests/golden/make_localizepose_golden.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import localizepose_data as PD  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "localizepose_golden.npz")


def answers():
    out = {}
    for name in ("known", "mixed"):
        r = PD.reference(name)
        for k in PD.ROW_ARRAYS + PD.CORR_ARRAYS:
            out[name + "_" + k] = np.asarray(r[k])
        out[name + "_scalars"] = np.array([r[k] for k in PD.SCALARS], np.int32)
    return out


def load():
    with np.load(PATH) as z:
        return {k: z[k] for k in z.files}


def main():
    np.savez_compressed(PATH, **answers())


if __name__ == "__main__":
    main()
