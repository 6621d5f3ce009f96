"""The layout of the BA partial-sum buffers (BaPartials in metricsfm_amd/csrc/ba_partials.h: where each kernel of an LM
iteration puts its per-workgroup sums, how many entries each buffer needs and how many each reduction takes) walked on the CPU
by tests/ba_partials_host_check.cc, a stand-alone host program built with the address and undefined-behaviour sanitizers.
Needs no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_partial_layout_holds_on_the_host(tmp_path):
    exe = tmp_path / "ba_partials_host_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "metricsfm_amd", "csrc"), os.path.join(ROOT, "tests", "ba_partials_host_check.cc"), "-o", str(exe)])
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "ba_partials_host_check ok" in run.stdout, run.stdout + run.stderr
