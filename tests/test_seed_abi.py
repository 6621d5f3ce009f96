"""The two structs of msfm_seed_hypotheses against the C compiler, in the manner of tests/test_abi.py, and the defaults
msfm_seed_default_options fills (basic_structs.h:174, :187, :190; the sample counts and seeds of the two relpose calls)."""
import ctypes as C
import os
import subprocess

from metricsfm_amd import _abi as A
from metricsfm_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_seed_struct_layouts_match_the_c_compiler(tmp_path):
    fields = [("msfm_seed_options", A.SeedOptions, [f for f, _ in A.SeedOptions._fields_]),
              ("msfm_seed_problem", A.SeedProblem, [f for f, _ in A.SeedProblem._fields_])]
    exprs = []
    for cname, _, names in fields:
        exprs.append("sizeof(%s)" % cname)
        exprs += ["offsetof(%s,%s)" % (cname, f) for f in names]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "msfm.h"\nint main(){size_t v[]={%s};'
                   'for(size_t i=0;i<sizeof v/sizeof v[0];i++)printf("%%zu ",v[i]);return 0;}\n' % ",".join(exprs))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    want = []
    for _, cls, names in fields:
        want.append(C.sizeof(cls))
        want += [getattr(cls, f).offset for f in names]
    assert got == want


def test_seed_defaults_are_the_reference_values():
    o = capi.seed_options()
    assert (o.th_mse_reprojection, o.th_angle_small, o.th_seedpair_structures) == (3.0, 3.0 / 180.0 * 3.1415, 20)
    assert (o.ransac_times_5pt, o.ransac_times_8pt, o.seed_5pt, o.seed_8pt) == (100, 200, 0x4D53464D45, 0x4D53464D38)
    assert capi.seed_options(th_seedpair_structures=7).th_seedpair_structures == 7
