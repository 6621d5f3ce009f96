"""Dense stereo on the device against the sequential restatement tests/sgm_ref.cpp: every plane msfm_sgm_fetch returns, byte for
byte, on shapes chosen so that each kernel's edges are met (tests/sgm_data.py names them), then the parameters' extremes, strides,
reuse, depth, the stats, every refusal, and dense.sgm_dense."""
import ctypes as C

import numpy as np
import pytest

from metricsfm_amd import _abi as A
from metricsfm_amd import capi, dense
from tests import sgm_data as X

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def fetch_all(sgm):
    got = {}
    for kind, name, _ in A.SGM_FETCH:
        got[name] = np.stack([sgm.fetch(kind, r) for r in range(8)]) if kind == 2 else sgm.fetch(kind)
    return got


def assert_planes(got, want, what=""):
    for _, name, _ in A.SGM_FETCH:
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, (what, name)
        if name == "path_cost":
            for r in range(8):
                assert np.array_equal(got[name][r], want[name][r]), (what, name, r)
        else:
            assert np.array_equal(got[name], want[name]), (what, name)


def run_case(ctx, name, variant=0, **par):
    D, w, h, _ = X.CASES[name]
    left, right = X.case_pair(name, variant)
    p = dict(X.DEFAULTS, **par)
    with ctx.stereo_sgm(w, h, D, p["P1"], p["P2"], p["uniqueness"]) as sgm:
        st = sgm.execute(left, right)
        return fetch_all(sgm), st


def test_groups_case_derivation():
    """The two further cases are one pixel larger, in both dimensions, than a multiple of the path kernels' groups per workgroup,
    SGM_PATH_THREADS / (D / SGM_LANE_DISP)."""
    for name, D in (("groups64", 64), ("groups128", 128)):
        g = A.SGM_PATH_THREADS // (D // A.SGM_LANE_DISP)
        _, w, h, _ = X.CASES[name]
        assert g == X.path_groups(D) and w % g == 1 and h % g == 1 and w >= D


@pytest.mark.parametrize("name", list(X.CASES))
def test_every_plane_equals_the_restatement(ctx, name):
    got, st = run_case(ctx, name)
    want = X.expected(name)
    assert_planes(got, want, name)
    D, w, h, _ = X.CASES[name]
    assert st == dict(host_waits=0, h2d_bytes=2 * w * h, kernel_launches=7)
    if name in ("flat64",):
        assert not got["census_left"].any() and not got["census_right"].any()
    if name == "onerow64":
        assert got["census_left"][3].any() and not got["census_left"][:3].any() and not got["census_left"][4:].any()


def test_largest_penalties(ctx):
    got, _ = run_case(ctx, "odd64", P1=224, P2=224)
    want = X.expected("odd64", P1=224, P2=224)
    assert_planes(got, want)
    # the numpy restatement keeps its costs in 64 bits: its largest one fits a byte, and is the largest byte of the device
    from tests import sgm_ref as R
    wide = R.run(*X.case_pair("odd64"), 64, 224, 224, 0.96)
    top = int(got["path_cost"].max())
    print("largest cost at P1 = P2 = 224: %d untruncated, %d on the device" % (wide["cost_max"], top))
    assert wide["cost_max"] <= 255 and top == wide["cost_max"]


@pytest.mark.parametrize("uniqueness", [0.0, 1.0])
def test_uniqueness_extremes(ctx, uniqueness):
    got, _ = run_case(ctx, "odd128", uniqueness=uniqueness)
    assert_planes(got, X.expected("odd128", uniqueness=uniqueness))


def test_strided_input_equals_packed(ctx):
    D, w, h, _ = X.CASES["odd64"]
    left, right = X.case_pair("odd64")
    wide_l, wide_r = np.full((h, w + 13), 255, np.uint8), np.full((h, w + 5), 0, np.uint8)
    wide_l[:, :w], wide_r[:, :w] = left, right
    with ctx.stereo_sgm(w, h, D) as sgm:
        sgm.execute(wide_l[:, :w], wide_r[:, :w])
        assert_planes(fetch_all(sgm), X.expected("odd64"))


def test_reuse(ctx):
    """execute twice gives the same bytes; another pair on the same object equals a fresh object (= the restatement of that pair)."""
    D, w, h, _ = X.CASES["groups128"]
    with ctx.stereo_sgm(w, h, D) as sgm:
        sgm.execute(*X.case_pair("groups128"))
        first = fetch_all(sgm)
        sgm.execute(*X.case_pair("groups128"))
        assert_planes(fetch_all(sgm), first)
        sgm.execute(*X.case_pair("groups128", 1))
        second = fetch_all(sgm)
    assert_planes(first, X.expected("groups128"))
    assert_planes(second, X.expected("groups128", variant=1))
    with ctx.stereo_sgm(w, h, D) as fresh:
        fresh.execute(*X.case_pair("groups128", 1))
        assert_planes(fetch_all(fresh), second)
    assert not np.array_equal(first["disparity"], second["disparity"])


def test_depth(ctx):
    D, w, h, _ = X.CASES["odd64"]
    want = X.expected("odd64")
    with ctx.stereo_sgm(w, h, D) as sgm:
        sgm.execute(*X.case_pair("odd64"))
        got = sgm.depth(X.BASELINE, X.FOCAL)
        assert np.array_equal(sgm.disparity(), want["disparity"]) and sgm.right_disparity().dtype == np.uint16
        assert sgm.size() == dict(width=w, height=h, disp_size=D, device_bytes=w * h * (2 + 8 + 8 * D + 8 + 1))
    assert np.array_equal(got, want["depth"])
    disp = want["disparity"]
    beyond = (disp > 0) & (((200.0 * X.BASELINE) * X.FOCAL) / np.maximum(disp, 1) > 255)
    assert beyond.any() and not got[beyond].any()            # the > 255 branch
    assert ((disp > 0) & ~beyond).any() and got[(disp > 0) & ~beyond].all()   # the in-range branch


def test_refusals_leave_the_object_usable(ctx):
    L = capi.lib()
    INV = A.MSFM_E_INVAL
    h_ = C.c_void_p()

    def create(*a):
        return L.msfm_sgm_create(ctx._h, *a, C.byref(h_))
    for args in ((64, 5, 96, 10, 120, 0.96), (63, 5, 64, 10, 120, 0.96), (127, 5, 128, 10, 120, 0.96), (16385, 5, 64, 10, 120, 0.96),
                 (64, 0, 64, 10, 120, 0.96), (64, 16385, 64, 10, 120, 0.96), (64, 5, 64, 10, 225, 0.96), (64, 5, 64, 121, 120, 0.96),
                 (64, 5, 64, -1, 120, 0.96), (64, 5, 64, 10, 120, float("nan")), (64, 5, 64, 10, 120, float("inf")), (64, 5, 64, 10, 120, 1.01),
                 (64, 5, 64, 10, 120, -0.01)):
        assert create(*args) == INV and not h_.value, args
    assert L.msfm_sgm_create(ctx._h, 64, 5, 64, 10, 120, 0.96, None) == INV
    D, w, h, _ = X.CASES["flat64"]
    left, right = X.case_pair("flat64")
    want = X.expected("flat64")
    with ctx.stereo_sgm(w, h, D) as sgm:
        out = np.full((h, w, D), 9, np.uint8)
        vp = out.ctypes.data_as(C.c_void_p)
        st = np.full(len(A.SGM_STATS), -1, np.int64)
        stp = A.ptr(st, C.POINTER(C.c_int64))
        lp, rp = C.cast(left.ctypes.data, A.c_u8_p), C.cast(right.ctypes.data, A.c_u8_p)
        # before the first execute
        assert L.msfm_sgm_fetch(sgm._h, 7, 0, vp) == INV
        assert L.msfm_sgm_depth(sgm._h, 1.0, 1.0, C.cast(vp, A.c_u8_p)) == INV
        # execute
        assert L.msfm_sgm_execute(sgm._h, None, w, rp, w, stp) == INV
        assert L.msfm_sgm_execute(sgm._h, lp, w, None, w, stp) == INV
        assert L.msfm_sgm_execute(sgm._h, lp, w - 1, rp, w, stp) == INV
        assert L.msfm_sgm_execute(sgm._h, lp, w, rp, w - 1, stp) == INV
        assert (st == -1).all()
        assert L.msfm_sgm_fetch(sgm._h, 7, 0, vp) == INV   # still nothing executed
        assert L.msfm_sgm_execute(sgm._h, lp, w, rp, w, None) == 0   # stats may be NULL
        # fetch and depth
        for kind, index in ((-1, 0), (8, 0), (2, 8), (2, -1), (0, 1), (7, 1)):
            assert L.msfm_sgm_fetch(sgm._h, kind, index, vp) == INV, (kind, index)
        assert L.msfm_sgm_fetch(sgm._h, 7, 0, None) == INV
        assert L.msfm_sgm_depth(sgm._h, 1.0, 1.0, None) == INV
        for b, f in ((float("nan"), 1.0), (1.0, float("inf")), (float("-inf"), 1.0)):
            assert L.msfm_sgm_depth(sgm._h, b, f, C.cast(vp, A.c_u8_p)) == INV
        assert (out == 9).all()
        with pytest.raises(capi.MsfmError):
            sgm.fetch(9)
        assert "kind" in L.msfm_last_error(ctx._h).decode()
        # and the object still works
        sgm.execute(left, right)
        assert_planes(fetch_all(sgm), want)


def test_sgm_dense_equals_single_runs(ctx):
    D, w, h, _ = X.CASES["odd128"]
    pairs = [X.case_pair("odd128", v) for v in range(3)]
    Ks = np.stack([np.diag([500.0 + 100 * i, 480.0, 1.0]) for i in range(4)])
    ts = np.array([[0, 0, 0], [0.03, 0.04, 0], [0.03, 0.04, 0.1], [0.5, 0.04, 0.1]], np.float64)
    got = dense.sgm_dense(ctx, pairs, Ks, ts, disp_size=D)
    assert len(got) == 3
    baselines = [0.05, 0.1, 0.47]
    for i, (disp, dep) in enumerate(got):
        with ctx.stereo_sgm(w, h, D) as one:
            one.execute(*pairs[i])
            assert np.array_equal(disp, one.disparity())
            assert abs(np.linalg.norm(ts[i + 1] - ts[i]) - baselines[i]) < 1e-12
            assert np.array_equal(dep, one.depth(float(np.sqrt(((ts[i + 1] - ts[i]) ** 2).sum())), float(Ks[i + 1][0, 0])))
        assert np.array_equal(disp, X.expected("odd128", variant=i)["disparity"])
    assert any(d.any() for _, d in got)
