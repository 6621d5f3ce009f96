"""The structs of msfm_recon_create and msfm_recon_localize (include/msfm.h) as the ctypes host mirrors them (metricsfm_amd/_abi.py) against a C compiler's
layout, in the manner of tests/test_round_abi.py."""
import ctypes as C
import os
import subprocess

from metricsfm_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INIT_FIELDS = [f for f, _ in A.ReconInit._fields_]
WINNER_FIELDS = [f for f, _ in A.ReconWinner._fields_]


def test_recon_struct_layout_matches_the_c_compiler(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "msfm.h"\nint main(){printf("%zu %zu", sizeof(msfm_recon_init), sizeof(msfm_recon_winner));\n' +
                   "".join('printf(" %%zu", offsetof(msfm_recon_init, %s));\n' % f for f in INIT_FIELDS) +
                   "".join('printf(" %%zu", offsetof(msfm_recon_winner, %s));\n' % f for f in WINNER_FIELDS) + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [C.sizeof(A.ReconInit), C.sizeof(A.ReconWinner)] + [getattr(A.ReconInit, f).offset for f in INIT_FIELDS] + \
           [getattr(A.ReconWinner, f).offset for f in WINNER_FIELDS]
    assert WINNER_FIELDS[:2] == ["image", "row"] and WINNER_FIELDS[-1] == "avg_error"
    assert len(INIT_FIELDS) == 26 and INIT_FIELDS[-2:] == ["reserve_points", "reserve_obs"]
