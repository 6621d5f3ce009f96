"""The children of a context (metricsfm_amd/csrc/common.h): child_new counts an object from the moment it exists, and
msfm_child_destroy - every public destroy of a child, and the path of a create that fails - waits for the stream if the object
holds blocks, deletes it and releases it last.  tests/child_check.cc, a stand-alone program with its own context, a "pool" that
records the stream's state at every free and a recording release, runs a failed create, a destroy with work in flight, a destroy
of a child without blocks and a destroy of null.  Built for gfx950 and run once, as a child process.  Then every child type that
has a one-line constructor at the Python boundary, used and closed after its context."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_child_destroy_waits_deletes_releases(tmp_path):
    exe = tmp_path / "child_check"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function",
                           "-I", os.path.join(ROOT, "metricsfm_amd", "csrc"), os.path.join(ROOT, "tests", "child_check.cc"), "-o", str(exe)])
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    # (exit status 2: a memset was too short for the frees, or the query of case 3, to have raced it - the run proves nothing)
    assert run.returncode == 0 and "child_check ok" in run.stdout, run.stdout + run.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["creation", "reverse"])
def test_every_child_type_outlives_its_context(order):
    """One child of each kind that has a one-line constructor, each at the smallest shape its create accepts, on a context of
    its own.  The context is closed first; every child still answers, and the last close - whichever child that is - releases
    the context."""
    from metricsfm_amd import _abi as A
    from metricsfm_amd import capi, scene
    c = capi.Context(0)
    rng = np.random.default_rng(1)
    rows = [np.rint(rng.uniform(0, 255, (64, 128))).astype(np.float32) for _ in range(2)]
    ds = c.descset(rows)
    res = ds.match_pairs(np.array([[0, 1]], np.int32))
    ba = c.ba(A.BaArrays.from_scene(scene.make_ring_scene(4, 200, seed=3)))
    ss = c.scalespace(np.array([[0, 255], [255, 0]], np.uint8), 1, 3)
    sgm = c.stereo_sgm(64, 1, 64)
    store = c.match_store([8, 8], [[0, 1]], [0, 4], [[0, 1], [2, 3], [4, 5], [6, 7]])
    na0, ng0 = res.counts()
    c.close()                       # six children alive: the library keeps the context
    got, xy = ds.fetch(1)
    assert (got == rows[1]).all() and xy is None
    na1, ng1 = res.counts()
    assert (na0 == na1).all() and (ng0 == ng1).all()
    assert ba.run(capi.default_options(max_num_iterations=3))["num_iterations"] == 3
    assert (ss.size(0)["w"], ss.size(0)["h"]) == (2, 2)
    assert sgm.size()["disp_size"] == 64
    children = [ds, res, ba, ss, sgm, store]
    for child in (children if order == "creation" else children[::-1]):
        child.close()
