"""Stereo rectification on the device against the sequential restatement tests/rectify_ref.cpp: every plane msfm_rectifier_fetch
returns, maps bit for bit and planes byte for byte, on every case and shape of tests/rectify_data.py; the closed-form cases
against their formulas; strides, reuse, the stats; the matching chain on the rectified planes (msfm_sgm_execute_rectified) against
tests/sgm_ref.cpp; dense.sgm_dense_posed; and every refusal."""
import ctypes as C

import numpy as np
import pytest

from metricsfm_amd import _abi as A
from metricsfm_amd import capi, dense
from tests import rectify_data as D
from tests import sgm_data as X

pytestmark = pytest.mark.gpu
GEOMETRY = (("R_left", "R1"), ("R_right", "R2"), ("P_left", "P1"), ("P_right", "P2"))


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def fetch_all(rect, maps=True):
    return {name: rect.fetch(kind) for kind, name, _ in A.RECTIFY_FETCH if maps or kind < 2}


def assert_planes(got, want, what=""):
    for _, name, _ in A.RECTIFY_FETCH:
        if name in got:
            assert same_bits(got[name], want[name]), (what, name)


def fetch_sgm(sgm):
    return {name: (np.stack([sgm.fetch(kind, r) for r in range(8)]) if kind == 2 else sgm.fetch(kind)) for kind, name, _ in A.SGM_FETCH}


def assert_sgm_planes(got, want, what=""):
    for _, name, _ in A.SGM_FETCH:
        assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), (what, name)


@pytest.mark.parametrize("shape_name", D.SHAPES)
@pytest.mark.parametrize("case", D.CASES)
def test_every_plane_equals_the_restatement(ctx, case, shape_name):
    w, h = D.shape(shape_name)
    left, right = D.pair(shape_name)
    want = D.expected(case, shape_name)
    with ctx.rectifier(w, h) as rect:
        out = rect.rectify(left, right, *D.pose_list(D.poses(case, w, h)), keep_maps=True)
        got = fetch_all(rect)
        assert rect.size() == dict(width=w, height=h, device_bytes=A.RECTIFY_PARAM_BYTES + 20 * w * h)
    assert_planes(got, want, (case, shape_name))
    for mine, theirs in GEOMETRY:
        assert same_bits(out[mine], want[theirs]), mine
    assert out["stats"] == dict(host_waits=0, h2d_bytes=2 * w * h + A.RECTIFY_PARAM_BYTES, kernel_launches=1)
    if case in D.CLOSED or case == "huge":      # and what the formulas say, without the restatement
        form = D.closed_form(case, left, right)
        for name in ("left", "right", "mapx_left", "mapx_right"):
            assert np.array_equal(got[name], form[name]), name
        assert np.array_equal(got["mapy_left"], form["mapy"]) and np.array_equal(got["mapy_right"], form["mapy"])
    if case in ("identity", "tie"):
        assert np.array_equal(got["left"], left) and np.array_equal(got["right"], right)
    if case.startswith("convergent"):
        assert out["P_right"][0, 3] < 0
        if shape_name == "odd64":
            D.border_coverage(shape_name)
    if case == "vertical":
        assert capi.stereo_rectify(*D.pose_list(D.poses(case, w, h)), w, h)["idx"] == 1


def test_strided_input_equals_packed(ctx):
    w, h = D.shape("odd64")
    left, right = D.pair("odd64")
    wide_l, wide_r = np.full((h, w + 13), 255, np.uint8), np.full((h, w + 5), 0, np.uint8)
    wide_l[:, :w], wide_r[:, :w] = left, right
    with ctx.rectifier(w, h) as rect:
        rect.rectify(wide_l[:, :w], wide_r[:, :w], *D.pose_list(D.poses("convergent", w, h)), keep_maps=True)
        assert_planes(fetch_all(rect), D.expected("convergent", "odd64"))


def test_reuse_and_maps_on_request(ctx):
    """A second rectify on the same object equals a fresh object; without keep_maps the planes are the same and the maps refused."""
    w, h = D.shape("odd128")
    left, right = D.pair("odd128")
    first, second = D.pose_list(D.poses("convergent", w, h)), D.pose_list(D.poses("vertical", w, h))
    with ctx.rectifier(w, h) as rect:
        rect.rectify(left, right, *first, keep_maps=True)
        assert_planes(fetch_all(rect), D.expected("convergent", "odd128"))
        st = rect.rectify(left, right, *second)["stats"]
        assert st == dict(host_waits=0, h2d_bytes=2 * w * h + A.RECTIFY_PARAM_BYTES, kernel_launches=1)
        again = fetch_all(rect, maps=False)
        for kind in (2, 3, 4, 5):
            with pytest.raises(capi.MsfmError) as e:
                rect.fetch(kind)
            assert e.value.code == A.MSFM_E_INVAL and "maps" in str(e.value)
        rect.rectify(left, right, *second, keep_maps=1)
        with_maps = fetch_all(rect)
    with ctx.rectifier(w, h) as fresh:
        fresh.rectify(left, right, *second, keep_maps=True)
        want = fetch_all(fresh)
    assert_planes(again, want)
    assert_planes(with_maps, want)
    assert_planes(want, D.expected("vertical", "odd128"))
    assert not np.array_equal(want["left"], D.expected("convergent", "odd128")["left"])


@pytest.mark.parametrize("name", ["odd64", "groups128"])
def test_execute_rectified_with_identity_poses(ctx, name):
    """The identity case copies the pair, so the chain behind it gives the restatement's planes of the pair itself."""
    Dn, w, h, _ = X.CASES[name]
    left, right = X.case_pair(name)
    with ctx.rectifier(w, h) as rect, ctx.stereo_sgm(w, h, Dn) as sgm:
        rect.rectify(left, right, *D.pose_list(D.poses("identity", w, h)))
        st = sgm.execute_rectified(rect)
        assert st == dict(host_waits=0, h2d_bytes=0, kernel_launches=7)
        assert_sgm_planes(fetch_sgm(sgm), X.expected(name), name)
        assert sgm.size()["device_bytes"] == w * h * (2 + 8 + 8 * Dn + 8 + 1)


@pytest.mark.parametrize("shape_name,disp", [("odd128", 128), ("odd64", 64)])
def test_execute_rectified_on_the_convergent_case(ctx, shape_name, disp):
    w, h = D.shape(shape_name)
    left, right = D.pair(shape_name)
    r = D.expected("convergent", shape_name)
    want = X.run_ref_cpp(r["left"], r["right"], disp)
    with ctx.rectifier(w, h) as rect, ctx.stereo_sgm(w, h, disp) as sgm:
        rect.rectify(left, right, *D.pose_list(D.poses("convergent", w, h)))
        sgm.execute_rectified(rect)
        assert_sgm_planes(fetch_sgm(sgm), want, shape_name)
    assert want["disparity"].any()


def test_both_executes_on_one_object(ctx):
    """msfm_sgm_execute on host arrays directly after an execute_rectified, and the other way round."""
    Dn, w, h, _ = X.CASES["odd64"]
    r = D.expected("convergent", "odd64")
    from_rect = X.run_ref_cpp(r["left"], r["right"], Dn)
    with ctx.rectifier(w, h) as rect, ctx.stereo_sgm(w, h, Dn) as sgm:
        rect.rectify(*D.pair("odd64"), *D.pose_list(D.poses("convergent", w, h)))
        sgm.execute_rectified(rect)
        st = sgm.execute(*X.case_pair("odd64"))
        assert st == dict(host_waits=0, h2d_bytes=2 * w * h, kernel_launches=7)
        assert_sgm_planes(fetch_sgm(sgm), X.expected("odd64"))
        sgm.execute_rectified(rect)
        assert_sgm_planes(fetch_sgm(sgm), from_rect)
        sgm.execute(*X.case_pair("odd64", 1))
        assert_sgm_planes(fetch_sgm(sgm), X.expected("odd64", variant=1))


def test_sgm_dense_posed_equals_single_calls(ctx):
    Dn, w, h, _ = X.CASES["odd64"]
    images = [X.case_pair("odd64", v)[v % 2] for v in range(3)]
    a, b = D.poses("convergent", w, h), D.poses("convergent_mirrored", w, h)
    # image 0 is the right image of pair 0; image 1 its left image and the right image of pair 1; camera 2 stands left of both
    Ks = np.stack([a["K2"], a["K1"], b["K2"]])
    Rs = np.stack([a["R2"], a["R1"], D.rot(0.02, 0.05, -0.03)])
    ts = np.stack([a["t2"], a["t1"], -Rs[2] @ np.array([-0.8, 0.03, 0.02])])
    got = dense.sgm_dense_posed(ctx, images, Ks, Rs, ts, disp_size=Dn)
    assert len(got["disparity"]) == 2 and got["P_right_sign"] == [-1, -1]
    with ctx.rectifier(w, h) as rect, ctx.stereo_sgm(w, h, Dn) as sgm:
        for i in range(2):
            Rl, Rr, g = dense.epipolar_rectification(rect, images[i + 1], Ks[i + 1], Rs[i + 1], ts[i + 1], images[i], Ks[i], Rs[i], ts[i])
            sgm.execute_rectified(rect)
            assert np.array_equal(got["disparity"][i], sgm.disparity())
            baseline = float(np.sqrt(((ts[i + 1] - ts[i]) ** 2).sum()))
            assert np.array_equal(got["depth"][i], sgm.depth(baseline, float(Ks[i + 1][0, 0])))
            assert same_bits(got["R_left"][i], Rl) and same_bits(got["R_right"][i], Rr)
            assert same_bits(Rl, capi.stereo_rectify(Ks[i + 1], Rs[i + 1], ts[i + 1], Ks[i], Rs[i], ts[i], w, h)["R_left"])
    assert same_bits(got["R_left"][0], D.expected("convergent", "odd64")["R1"])
    Rn, tn = dense.epipolar_poses(Rs, ts, got["R_left"])
    assert np.array_equal(got["Rs_new"], Rn) and np.array_equal(got["ts_new"], tn) and not Rn[0].any()
    assert dense.sgm_dense_posed(ctx, images[:1], Ks, Rs, ts, disp_size=Dn)["disparity"] == []


def test_refusals_leave_the_object_usable(ctx):
    L = capi.lib()
    INV = A.MSFM_E_INVAL
    h_ = C.c_void_p()
    for args in ((0, 5), (5, 0), (16385, 5), (5, 16385), (-1, 5)):
        assert L.msfm_rectifier_create(ctx._h, *args, C.byref(h_)) == INV and not h_.value, args
    assert L.msfm_rectifier_create(ctx._h, 64, 5, None) == INV
    Dn, w, h, _ = X.CASES["odd64"]
    left, right = D.pair("odd64")
    good = D.pose_list(D.poses("convergent", w, h))
    want = D.expected("convergent", "odd64")
    i64p = C.POINTER(C.c_int64)
    with ctx.rectifier(w, h) as rect, ctx.stereo_sgm(w, h, Dn) as sgm:
        out = np.full((h, w), 9, np.float32)
        vp = out.ctypes.data_as(C.c_void_p)
        st = np.full(len(A.RECTIFY_STATS), -1, np.int64)
        geo = [np.full(n, 7.5) for n in (9, 9, 12, 12)]
        lp, rp = C.cast(left.ctypes.data, A.c_u8_p), C.cast(right.ctypes.data, A.c_u8_p)

        def rectify(l=lp, ls=w, r=rp, rs=w, poses=good, stats=st):
            ptrs = [None if a is None else A.ptr(a, A.c_double_p) for a in poses]
            return L.msfm_rectifier_rectify(rect._h, l, ls, r, rs, *ptrs, 1, *[A.ptr(g, A.c_double_p) for g in geo], A.ptr(stats, i64p))
        # before the first rectify
        assert L.msfm_rectifier_fetch(rect._h, 0, vp) == INV
        assert L.msfm_sgm_execute_rectified(sgm._h, rect._h, A.ptr(st, i64p)) == INV
        assert "not rectified" in L.msfm_last_error(ctx._h).decode()
        # rectify
        assert rectify(l=None) == INV and rectify(r=None) == INV
        assert rectify(ls=w - 1) == INV and rectify(rs=w - 1) == INV
        for k in range(6):
            assert rectify(poses=good[:k] + [None] + good[k + 1:]) == INV, k
        nan_k = [a.copy() for a in good]
        nan_k[0][0, 2] = np.nan
        inf_k = [a.copy() for a in good]
        inf_k[3][1, 1] = np.inf
        one_centre = [a.copy() for a in good]
        one_centre[5] = np.zeros(3)                     # (t1 is zero too: both centres at the origin)
        for bad in (nan_k, inf_k, one_centre):
            assert rectify(poses=bad) == INV
        assert "baseline" in L.msfm_last_error(ctx._h).decode()
        assert (st == -1).all() and all((g == 7.5).all() for g in geo)
        assert L.msfm_rectifier_fetch(rect._h, 0, vp) == INV       # still nothing rectified
        assert rectify(stats=None) == 0                            # stats may be NULL
        # fetch
        for kind in (-1, 6, 100):
            assert L.msfm_rectifier_fetch(rect._h, kind, vp) == INV, kind
        assert L.msfm_rectifier_fetch(rect._h, 0, None) == INV
        assert (out == 9).all()
        with pytest.raises(capi.MsfmError):
            rect.fetch(6)
        assert "kind" in L.msfm_last_error(ctx._h).decode()
        # execute_rectified: a rectifier of another size, of a second context, none
        assert L.msfm_sgm_execute_rectified(sgm._h, None, A.ptr(st, i64p)) == INV
        with ctx.rectifier(w + 1, h) as other:
            other.rectify(np.zeros((h, w + 1), np.uint8), np.zeros((h, w + 1), np.uint8), *good)
            assert L.msfm_sgm_execute_rectified(sgm._h, other._h, A.ptr(st, i64p)) == INV
        second = capi.Context(0)
        try:
            with second.rectifier(w, h) as foreign:
                foreign.rectify(left, right, *good)
                assert L.msfm_sgm_execute_rectified(sgm._h, foreign._h, A.ptr(st, i64p)) == INV
                assert "context" in L.msfm_last_error(ctx._h).decode()
        finally:
            second.close()
        assert (st == -1).all()
        assert L.msfm_sgm_fetch(sgm._h, 7, 0, vp) == INV           # and nothing has been executed
        # and the objects still work
        rect.rectify(left, right, *good, keep_maps=True)
        assert_planes(fetch_all(rect), want)
        sgm.execute_rectified(rect)
        assert np.array_equal(sgm.disparity(), X.run_ref_cpp(want["left"], want["right"], Dn, volumes=False)["disparity"])
