"""Generator of tests/golden/newpoints_golden.npz: the inputs of tests/newpoints_data.py::golden_case (two new cameras, seven
visible entries, th_matches_large = 40) and every output of the sequential restatement tests/newpoints_ref.cpp.
tests/test_gpu_newpoints.py::test_golden_fixture checks the GPU against it, tests/test_newpoints_ref.py that it still reproduces.
Run from the repository root: python tests/golden/make_newpoints_golden.py"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import newpoints_data as D  # noqa: E402
from tests import newpoints_ref as NR  # noqa: E402


def main():
    c = D.golden_case()
    with tempfile.TemporaryDirectory() as d:
        want = NR.new_points(NR.build_ref(d), *D.ref_args(c), **D.GOLDEN_OPTS)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "newpoints_golden.npz"), **{k: c[k] for k in D.INPUTS},
                        **{"want_" + k: np.asarray(v) for k, v in want.items()})


if __name__ == "__main__":
    main()
