"""The row function of the back substitution (msfm_backsub_row in metricsfm_amd/csrc/ba_device.h: residual, scaled point block
and the derivative of the residual along the step, one forward-mode tangent) against the full scaled Jacobian contracted with
the step (linearize_core, what k_backsub evaluated before) and against the same in long double, by
tests/backsub_row_host_check.cc: a stand-alone program compiled for the host only, with the address and undefined-behaviour
sanitizers.  Needs no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_backsub_row_against_full_jacobian_on_the_host(tmp_path):
    exe = tmp_path / "backsub_row_host_check"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    # (ba_device.h is HIP source - the lane operations beside the row functions are device builtins - so the HIP compiler reads
    #  it, host side only; -ffp-contract=off: the bit comparison of the residuals is between two statements of the same operations)
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "metricsfm_amd", "csrc"), os.path.join(ROOT, "tests", "backsub_row_host_check.cc"), "-o", str(exe)])
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(run.stdout)
    assert run.returncode == 0 and "backsub_row_host_check ok" in run.stdout, run.stdout + run.stderr
