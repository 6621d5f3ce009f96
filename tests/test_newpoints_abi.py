"""The two structs of msfm_new_points against the C compiler, in the manner of tests/test_seed_abi.py, and the defaults
msfm_new_points_default_options fills (basic_structs.h:187, :190, :191; the 500 of sfm_incremental.cc:781)."""
import ctypes as C
import os
import subprocess

from metricsfm_amd import _abi as A
from metricsfm_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_points_struct_layouts_match_the_c_compiler(tmp_path):
    fields = [("msfm_new_points_options", A.NewPointsOptions, [f for f, _ in A.NewPointsOptions._fields_]),
              ("msfm_new_points_problem", A.NewPointsProblem, [f for f, _ in A.NewPointsProblem._fields_])]
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


def test_new_points_defaults_are_the_reference_values():
    o = capi.new_points_options()
    assert (o.th_mse_reprojection, o.th_angle_small, o.th_angle_large, o.th_matches_large) == (3.0, 3.0 / 180.0 * 3.1415, 5.0 / 180.0 * 3.1415, 500)
    assert capi.new_points_options(th_matches_large=7).th_matches_large == 7
