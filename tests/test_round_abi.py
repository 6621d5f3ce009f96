"""The structs of msfm_round_adjust (include/msfm.h) as the ctypes host mirrors them (metricsfm_amd/_abi.py) against a C compiler's
layout, in the manner of tests/test_abi.py, and the defaults msfm_round_default_options documents."""
import ctypes as C
import os
import subprocess

from metricsfm_amd import _abi as A
from metricsfm_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTION_FIELDS = ("partial", "full", "weight_partial", "weight_full", "th_mse_outliers", "keep_problem")
PROBLEM_FIELDS = [f for f, _ in A.RoundProblem._fields_]


def test_round_struct_layouts_match_the_c_compiler(tmp_path):
    fields = [("msfm_round_options", f) for f in OPTION_FIELDS] + [("msfm_round_problem", f) for f in PROBLEM_FIELDS]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "msfm.h"\nint main(){printf("%zu %zu", sizeof(msfm_round_options), '
                   'sizeof(msfm_round_problem));\n' + "".join('printf(" %%zu", offsetof(%s, %s));\n' % sf for sf in fields) + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    want = [C.sizeof(A.RoundOptions), C.sizeof(A.RoundProblem)] + [getattr(A.RoundOptions, f).offset for f in OPTION_FIELDS] + \
           [getattr(A.RoundProblem, f).offset for f in PROBLEM_FIELDS]
    assert got == want
    assert len(PROBLEM_FIELDS) == 25 and PROBLEM_FIELDS[-3:] == ["do_partial", "do_full", "do_outliers"]


def test_round_defaults_are_the_references():
    o = capi.round_options()
    for b in (o.partial, o.full):
        assert (b.max_num_iterations, b.huber_delta, b.function_tolerance, b.gradient_tolerance, b.parameter_tolerance) == (100, 1.0, 1e-6, 1e-10, 1e-8)
    assert (o.weight_partial, o.weight_full, o.th_mse_outliers, o.keep_problem) == (2.0, 1.0, 1.0, 0)
    o = capi.round_options(keep_problem=1, partial=dict(max_num_iterations=7))
    assert (o.partial.max_num_iterations, o.full.max_num_iterations, o.keep_problem) == (7, 100, 1)
