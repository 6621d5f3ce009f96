"""DevScope (metricsfm_amd/csrc/common.h), the type that keeps a call's device scratch out of the block cache until the stream
has drained: tests/devscope_check.cc, a stand-alone program with its own context and a "pool" that records the stream's state
at every free, leaves a function that owns three blocks and has a 512 MiB memset in flight through HIP_TRY, finish() and
dismiss(), and checks the counting of up().  Built for gfx950 and run once, as a child process."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_devscope_frees_behind_the_stream(tmp_path):
    exe = tmp_path / "devscope_check"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function",
                           "-I", os.path.join(ROOT, "metricsfm_amd", "csrc"), os.path.join(ROOT, "tests", "devscope_check.cc"), "-o", str(exe)])
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    # (exit status 2: the memset was too short for the frees to have raced it - the run proves nothing)
    assert run.returncode == 0 and "devscope_check ok" in run.stdout, run.stdout + run.stderr
