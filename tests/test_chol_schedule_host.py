"""The launch schedule of an elimination plan (CholSchedule in metricsfm_amd/csrc/chol_schedule.h: what msfm_chol_factor_solve
launches for a plan, on both factorisation forms and both back-substitution forms) built for hand-written plans on the CPU and
checked against brute force by tests/chol_schedule_host_check.cc, a stand-alone host program built with the address and
undefined-behaviour sanitizers.  Needs no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_schedule_holds_on_the_host(tmp_path):
    exe = tmp_path / "chol_schedule_host_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "metricsfm_amd", "csrc"), os.path.join(ROOT, "tests", "chol_schedule_host_check.cc"), "-o", str(exe)])
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "chol_schedule_host_check ok" in run.stdout, run.stdout + run.stderr
