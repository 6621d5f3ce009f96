"""The structs of the "SLAM + GPS registration" section of include/msfm.h against a C compiler, and the default values."""
import ctypes as C
import os
import subprocess

from metricsfm_amd import _abi as A
from metricsfm_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_layouts_match_the_c_compiler(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "msfm.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n",'
                   'sizeof(msfm_gpsreg_options),offsetof(msfm_gpsreg_options,clip_deg),offsetof(msfm_gpsreg_options,th_outlier),'
                   'sizeof(msfm_gps_orient_result),offsetof(msfm_gps_orient_result,weight),offsetof(msfm_gps_orient_result,Rg),'
                   'offsetof(msfm_gps_orient_result,scale),offsetof(msfm_gps_orient_result,offset));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    want = [C.sizeof(A.GpsregOptions), A.GpsregOptions.clip_deg.offset, A.GpsregOptions.th_outlier.offset, C.sizeof(A.GpsOrientResult),
            A.GpsOrientResult.weight.offset, A.GpsOrientResult.Rg.offset, A.GpsOrientResult.scale.offset, A.GpsOrientResult.offset.offset]
    assert got == want


def test_defaults_are_the_references():
    o = capi.gpsreg_options()
    assert (o.th_outlier, o.min_views, o.window, o.clip_deg) == (3.0, 3, 20, 80.0)
    assert capi.gpsreg_options(window=5).window == 5
