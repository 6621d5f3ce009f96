"""msfm_scalespace_* and msfm_descset_describe / _fetch against the sequential restatement tests/sift_ref.cpp: every level, every
gradient plane and every descriptor row bit for bit, then the hand-over of the resident rows to the matcher and the refusals."""
import ctypes as C

import numpy as np
import pytest

from metricsfm_amd import _abi as A
from metricsfm_amd import capi
from tests import sift_data as D

pytestmark = pytest.mark.gpu
F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def make_ss(ctx, name):
    w, h, stride, O, S, seed, patch = D.CASES[name]
    return ctx.scalespace(D.case_image(name), O, S, stride=stride if stride != w else None)


def empty_set(ctx, n_images):
    return ctx.descset([np.zeros((0, 128), F32)] * n_images)


@pytest.mark.parametrize("name", list(D.CASES))
def test_levels_and_gradients_equal_the_restatement(ctx, name):
    w, h, stride, O, S, seed, patch = D.CASES[name]
    e = D.expected(name)
    with make_ss(ctx, name) as ss:
        for o in range(O):
            z = ss.size(o)
            assert (z["w"], z["h"]) == (w >> o, h >> o)
            for s in range(-1, S + 2):
                assert np.array_equal(bits(ss.level(o, s)), bits(e["gss"][o][s + 1])), (o, s)
            for s in range(S):
                mod, ang = ss.gradient(o, s)
                assert np.array_equal(bits(mod), bits(e["mod"][o][s])), (o, s)
                assert np.array_equal(bits(ang), bits(e["ang"][o][s])), (o, s)
        assert h * stride <= ss.size(0)["h2d_bytes"] + stride <= h * stride + stride + 4096   # the image, the taps and the table


@pytest.mark.parametrize("quantize", [0, 1])
@pytest.mark.parametrize("name", list(D.CASES))
def test_rows_and_keypoints_equal_the_restatement(ctx, name, quantize):
    e = D.expected(name)
    frames, want = e["frames"], e["rows"][quantize]
    n = len(frames)
    assert 1 <= n <= 300
    with make_ss(ctx, name) as ss, empty_set(ctx, 2) as ds:
        sent = ds.describe(1, ss, frames, quantize)
        assert sent <= 64 * n + 4096
        rows, xy = ds.fetch(1)
        bad = np.flatnonzero((bits(rows) != bits(want)).any(axis=1))
        assert bad.size == 0, (bad[:10], e["records"][bad[:10]])
        assert np.array_equal(bits(xy), bits(frames[:, :2]))
        assert capi.lib().msfm_descset_count(ds._h, 1) == n and capi.lib().msfm_descset_count(ds._h, 0) == 0
        # the same call again: the same bytes
        ds.describe(1, ss, frames, quantize)
        rows2, xy2 = ds.fetch(1)
        assert rows2.tobytes() == rows.tobytes() and xy2.tobytes() == xy.tobytes()
        # n = 1, every frame kind once
        for f in (0, e["idx"]["clamp_high"], e["idx"]["outside"][0], e["idx"]["twins"][0]):
            assert ds.describe(0, ss, frames[f:f + 1], quantize) <= 64 + 4096
            one, oxy = ds.fetch(0)
            assert np.array_equal(bits(one), bits(want[f:f + 1])) and np.array_equal(bits(oxy), bits(frames[f:f + 1, :2])), f
        # n = 0 empties the image
        ds.describe(0, ss, np.zeros((0, 4), F32), quantize)
        assert ds.fetch(0)[0].shape == (0, 128)


@pytest.mark.parametrize("quantize", [1, 0])
def test_described_rows_match_like_uploaded_rows(ctx, quantize):
    ea, ec = D.expected("a"), D.expected("c")
    pairs = [[0, 1], [1, 0]]
    with make_ss(ctx, "a") as sa, make_ss(ctx, "c") as sc, empty_set(ctx, 2) as ds:
        ds.describe(0, sa, ea["frames"], quantize)
        ds.describe(1, sc, ec["frames"], quantize)
        fetched = [ds.fetch(i) for i in range(2)]
        with ds.match_pairs(pairs, keep_knn=True) as res:
            got = [res.fetch(p) for p in range(2)]
            got_counts, stats = res.counts(), res.stats()
            with ctx.descset([r for r, _ in fetched], [xy for _, xy in fetched]) as up, up.match_pairs(pairs, keep_knn=True) as ref:
                want_counts = ref.counts()
                for p in range(2):
                    for g, w in zip(got[p], ref.fetch(p)):
                        assert np.array_equal(g, w), p
                assert ref.stats() == stats
            assert all(np.array_equal(g, w) for g, w in zip(got_counts, want_counts))
            assert stats["queries"] == len(ea["frames"]) + len(ec["frames"])
            if quantize:
                assert stats["slow_path"] == 0   # integer rows in [0, 255]: the int8 kernel took them
            # a result made before a describe of one of its images is stale
            res.rerun()
            ds.describe(1, sc, ec["frames"][:5], quantize)
            with pytest.raises(capi.MsfmError) as err:
                res.rerun()
            assert err.value.code == A.MSFM_E_INVAL


def test_refusals_leave_everything_usable(ctx):
    L = capi.lib()
    e = D.expected("a")
    w, h, stride, O, S, seed, patch = D.CASES["a"]
    img = np.ascontiguousarray(D.case_image("a"))
    gp = A.ptr(img, A.c_u8_p)
    out = C.c_void_p()
    flat = np.full((16, 16), 9, np.uint8)
    small = np.ascontiguousarray(img[:12, :12])
    for args in ((None, w, h, w, O, S), (gp, 1, h, w, O, S), (gp, w, 1, w, O, S), (gp, 16385, h, 16385, O, S), (gp, w, 16385, w, O, S),
                 (gp, w, h, w - 1, O, S), (gp, w, h, w, 0, S), (gp, w, h, w, 9, S), (gp, w, h, w, O, 0), (gp, w, h, w, O, 9),
                 (A.ptr(small, A.c_u8_p), 12, 12, 12, 4, S), (A.ptr(flat, A.c_u8_p), 16, 16, 16, 2, S)):
        assert L.msfm_scalespace_create(ctx._h, *args, C.byref(out)) == A.MSFM_E_INVAL, args[1:]
        assert not out.value
    assert L.msfm_scalespace_create(ctx._h, gp, w, h, w, O, S, None) == A.MSFM_E_INVAL
    assert L.msfm_descset_create(ctx._h, 1, 64, C.byref(out)) == A.MSFM_E_INVAL and not out.value   # dim != 128
    frames = e["frames"]
    fp = A.ptr(frames, A.c_float_p)
    big = np.ones((65536, 4), F32)
    other = capi.Context(0)
    try:
        with make_ss(ctx, "a") as ss, other.scalespace(img, 2, 3) as foreign, empty_set(ctx, 2) as ds:
            plane = np.zeros((h, w), F32)
            pp = A.ptr(plane, A.c_float_p)
            for o, s, kind, dst in ((-1, 0, 0, pp), (O, 0, 0, pp), (0, -2, 0, pp), (0, S + 2, 0, pp), (0, -1, 1, pp), (0, S, 1, pp), (0, -1, 2, pp),
                                    (0, S, 2, pp), (0, 0, 3, pp), (0, 0, -1, pp), (0, 0, 0, None)):
                assert L.msfm_scalespace_fetch(ss._h, o, s, kind, dst) == A.MSFM_E_INVAL, (o, s, kind)
            assert L.msfm_scalespace_size(ss._h, O, None, None, None) == A.MSFM_E_INVAL
            ds.describe(0, ss, frames[:7], 0)
            before = ds.fetch(0)[0].copy()
            bad_frames = []
            for col, val in ((0, np.nan), (1, np.inf), (2, np.nan), (3, -np.inf), (2, 0.0), (2, -1.5)):
                b = frames[:4].copy()
                b[2, col] = val
                bad_frames.append(b)
            calls = [(ds._h, 0, None, fp, 3), (ds._h, 0, ss._h, None, 3), (ds._h, 0, ss._h, fp, -1), (ds._h, 0, ss._h, A.ptr(big, A.c_float_p), 65536),
                     (ds._h, -1, ss._h, fp, 3), (ds._h, 2, ss._h, fp, 3), (ds._h, 0, foreign._h, fp, 3), (None, 0, ss._h, fp, 3)]
            calls += [(ds._h, 0, ss._h, A.ptr(b, A.c_float_p), 4) for b in bad_frames]
            for set_h, image, ss_h, frames_p, n in calls:
                assert L.msfm_descset_describe(set_h, image, ss_h, frames_p, n, 0, None) == A.MSFM_E_INVAL, (image, n)
                assert np.array_equal(bits(ds.fetch(0)[0]), bits(before))   # found before the first write
            assert L.msfm_descset_fetch(ds._h, 2, None, None) == A.MSFM_E_INVAL
            # the same objects still give the restatement's bits
            ds.describe(0, ss, frames, 0)
            assert np.array_equal(bits(ds.fetch(0)[0]), bits(e["rows"][0]))
            assert np.array_equal(bits(ss.level(O - 1, S + 1)), bits(e["gss"][O - 1][S + 2]))
            assert np.array_equal(bits(foreign.level(1, 0)), bits(D.run_ref_cpp(img, 2, 3, np.zeros((0, 4), F32))["gss"][1][1]))
    finally:
        other.close()
