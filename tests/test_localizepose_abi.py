"""msfm_localize_pose_options against the C compiler, in the manner of tests/test_newpoints_abi.py, and the defaults
msfm_localize_pose_default_options fills (basic_structs.h:186, :177; the 200 samples of absolute_pose_via_epnp.cc; the sweep of
msfm_epnpf_default_options)."""
import ctypes as C
import os
import subprocess

from metricsfm_amd import _abi as A
from metricsfm_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_localize_pose_options_layout_matches_the_c_compiler(tmp_path):
    cname, cls = "msfm_localize_pose_options", A.LocalizePoseOptions
    names = [f for f, _ in cls._fields_]
    exprs = ["sizeof(%s)" % cname] + ["offsetof(%s,%s)" % (cname, f) for f in names] + ["sizeof(msfm_epnpf_options)"]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "msfm.h"\nint main(){size_t v[]={%s};'
                   'for(size_t i=0;i<sizeof v/sizeof v[0];i++)printf("%%zu ",v[i]);return 0;}\n' % ",".join(exprs))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [C.sizeof(cls)] + [getattr(cls, f).offset for f in names] + [C.sizeof(A.EpnpfOptions)]


def test_localize_pose_defaults_are_the_reference_values():
    o = capi.localize_pose_options()
    assert (o.th_mse_localization, o.th_min_2d3d_corres, o.max_iter, o.seed, o.first_row, o.max_tries) == (5.0, 20, 200, 0x4D53464D50, 0, 16)
    d = capi.epnpf_options()
    assert all(getattr(o.sweep, f) == getattr(d, f) for f, _ in A.EpnpfOptions._fields_)
    o = capi.localize_pose_options(max_tries=1, sweep=dict(f_ratio_step=0.05))
    assert o.max_tries == 1 and o.sweep.f_ratio_step == 0.05 and o.sweep.f_ratio_min == 0.5
