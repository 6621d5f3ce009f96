"""The geometry of the point workgroups (PtMap in metricsfm_amd/csrc/ba_device.h: which points a workgroup of k_point and
k_backsub holds, and with how many lanes each) walked on the CPU by tests/ptmap_host_check.cc, a stand-alone program compiled
for the host only.  Needs no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ptmap_round_trips_on_the_host(tmp_path):
    exe = tmp_path / "ptmap_host_check"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    # (ba_device.h is HIP source - the lane operations beside PtMap are device builtins - so the HIP compiler reads it, host side only)
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-std=c++17", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "metricsfm_amd", "csrc"), os.path.join(ROOT, "tests", "ptmap_host_check.cc"), "-o", str(exe)])
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "ptmap_host_check ok" in run.stdout, run.stdout + run.stderr
