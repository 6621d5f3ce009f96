"""msfm_scalespace_detect and msfm_descset_extract against the sequential restatement tests/siftdetect_ref.cpp: every frame bit
for bit in order and every counter, at the reference's thresholds and at others, at every capacity; extract against detect
followed by describe; extract_all's set against the same rows uploaded from the host; and the refusals."""
import ctypes as C

import numpy as np
import pytest

from metricsfm_amd import _abi as A
from metricsfm_amd import capi, extract, featurefiles
from tests import siftdetect_data as X

pytestmark = pytest.mark.gpu
F32 = np.float32
I64P = C.POINTER(C.c_int64)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def make_ss(ctx, name):
    w, h, stride, O, S, seed, patch = X.CASES[name]
    return ctx.scalespace(X.case_image(name), O, S, stride=stride if stride != w else None)


def empty_set(ctx, n_images):
    return ctx.descset([np.zeros((0, 128), F32)] * n_images)


def assert_same(got_frames, got_stats, e, max_frames=65535):
    n = min(e["stats"]["n_found"], max_frames)
    assert got_frames.shape == (n, 4)
    bad = np.flatnonzero((bits(got_frames) != bits(e["frames"][:n])).any(axis=1))
    assert bad.size == 0, (bad[:10], got_frames[bad[:10]], e["frames"][bad[:10]])
    assert X.counters(got_stats) == X.counters(e["stats"])
    nc, nk = e["stats"]["candidates"], e["stats"]["keypoints"]
    assert got_stats["d2h_bytes"] == 4 + 32 * nc + 20 * nk and (got_stats["h2d_bytes"] == 20 * nk if nk else got_stats["h2d_bytes"] == 0)


@pytest.mark.parametrize("name", list(X.CASES))
def test_frames_and_counters_equal_the_restatement(ctx, name):
    e = X.expected(name)
    assert e["stats"]["n_found"] >= 10
    with make_ss(ctx, name) as ss:
        frames, stats = ss.detect()
        assert_same(frames, stats, e)
        frames2, stats2 = ss.detect()   # the same call again: the same bytes
        assert frames2.tobytes() == frames.tobytes() and stats2 == stats


def test_thresholds_and_capacity(ctx):
    e0 = X.expected("d")
    accepted = np.sort(np.abs(e0["vals"][(e0["raw"]["flags"] & X.KP_STATUS) == 0]))
    lo, hi = accepted[len(accepted) // 2 - 1], accepted[len(accepted) // 2]
    assert lo < hi
    peak = float(F32(0.5) * (lo + hi))
    assert lo < F32(peak) < hi
    e = X.expected("d", peak, 5.0)
    assert 0 < e["stats"]["n_found"] < e0["stats"]["n_found"] and e["stats"]["rejected_peak"] > 0
    assert e["stats"]["rejected_edge"] > X.expected("d", peak, 10.0)["stats"]["rejected_edge"]
    with make_ss(ctx, "d") as ss:
        assert_same(*ss.detect(peak, 5.0), e)
        for cap in (0, 1, e0["stats"]["n_found"] - 1):
            assert_same(*ss.detect(max_frames=cap), e0, cap)


@pytest.mark.parametrize("quantize", [0, 1])
def test_extract_is_detect_then_describe(ctx, quantize):
    n_found = X.expected("d")["stats"]["n_found"]
    with make_ss(ctx, "d") as ss, make_ss(ctx, "c") as sc, empty_set(ctx, 2) as ds, empty_set(ctx, 2) as two:
        for cap in (65535, 7):
            frames, dstats = ss.detect(max_frames=cap)
            sent = two.describe(1, ss, frames, quantize)
            want_rows, want_xy = two.fetch(1)
            stats = ds.extract(1, ss, max_frames=cap, quantize=quantize)
            rows, xy = ds.fetch(1)
            assert len(rows) == min(cap, n_found)
            assert np.array_equal(bits(rows), bits(want_rows)) and np.array_equal(bits(xy), bits(want_xy))
            assert np.array_equal(bits(xy), bits(frames[:, :2]))
            assert capi.lib().msfm_descset_count(ds._h, 1) == len(frames) and capi.lib().msfm_descset_count(ds._h, 0) == 0
            assert X.counters(stats) == dict(X.counters(dstats), host_waits=dstats["host_waits"] + 2)
            assert stats["h2d_bytes"] == dstats["h2d_bytes"] + sent and stats["d2h_bytes"] == dstats["d2h_bytes"]
        # a match result made before an extract of one of its images is stale
        ds.extract(0, sc, quantize=quantize)
        with ds.match_pairs([[0, 1]]) as res:
            res.rerun()
            ds.extract(1, ss, max_frames=9, quantize=quantize)
            with pytest.raises(capi.MsfmError) as err:
                res.rerun()
            assert err.value.code == A.MSFM_E_INVAL


@pytest.mark.parametrize("quantize", [1, 0])
def test_extracted_rows_match_like_uploaded_rows(ctx, quantize, tmp_path):
    names = ("c", "d")
    grays = [X.case_image(n) for n in names]
    pairs = [[0, 1], [1, 0]]
    with pytest.raises(capi.MsfmError):
        extract.extract_all(ctx, grays, n_octaves=9)   # a refusal closes the set it made
    ds = extract.extract_all(ctx, grays, n_octaves=3, n_levels=3, quantize=quantize, fold=str(tmp_path))
    with ds:
        assert [st["n_found"] for st in ds.extract_stats] == [X.expected(n)["stats"]["n_found"] for n in names] == ds.counts
        fetched = [ds.fetch(i) for i in range(2)]
        for i, (rows, xy) in enumerate(fetched):   # the feature file of the reference's format holds the same rows
            info, kp, desc = featurefiles.read_image_feature(str(tmp_path), i)
            h, w = grays[i].shape
            assert (info["rows"], info["cols"]) == (h, w) and np.array_equal(bits(desc), bits(rows))
            assert np.array_equal(kp, (xy.astype(np.float64) - [w / 2.0, h / 2.0]).astype(F32))
            assert np.array_equal(bits(xy), bits(X.expected(names[i])["frames"][:, :2]))
        with ds.match_pairs(pairs, keep_knn=True) as res:
            got = [res.fetch(p) for p in range(2)]
            got_counts, stats = res.counts(), res.stats()
            with ctx.descset([r for r, _ in fetched], [xy for _, xy in fetched]) as up, up.match_pairs(pairs, keep_knn=True) as ref:
                want_counts = ref.counts()
                for p in range(2):
                    for g, w_ in zip(got[p], ref.fetch(p)):
                        assert np.array_equal(g, w_), p
                assert ref.stats() == stats
            assert all(np.array_equal(g, w_) for g, w_ in zip(got_counts, want_counts))
            assert stats["queries"] == sum(ds.counts)
            if quantize:
                assert stats["slow_path"] == 0   # integer rows in [0, 255]: the int8 kernel took them


def test_refusals_leave_everything_usable(ctx):
    L = capi.lib()
    e = X.expected("a")
    w, h, stride, O, S, seed, patch = X.CASES["a"]
    other = capi.Context(0)
    try:
        with make_ss(ctx, "a") as ss, other.scalespace(X.case_image("a"), 2, 3) as foreign, empty_set(ctx, 2) as ds:
            frames = np.zeros((65535, 4), F32)
            fp, n, st = A.ptr(frames, A.c_float_p), C.c_int32(-7), np.full(len(A.SIFT_DETECT_STATS), -1, np.int64)
            sp = A.ptr(st, I64P)
            level_before = ss.level(O - 1, S + 1).copy()
            ds.extract(0, ss)
            before = ds.fetch(0)
            assert len(before[0]) == e["stats"]["n_found"]
            nan, inf = float("nan"), float("inf")
            bad_thresholds = ((nan, 10.0), (inf, 10.0), (-1.0, 10.0), (0.0, nan), (0.0, inf), (0.0, -0.5), (-inf, 10.0))
            calls = [(None, 0.0, 10.0, 10, fp, C.byref(n), sp), (ss._h, 0.0, 10.0, 10, None, C.byref(n), sp), (ss._h, 0.0, 10.0, 10, fp, None, sp),
                     (ss._h, 0.0, 10.0, -1, fp, C.byref(n), sp), (ss._h, 0.0, 10.0, 65536, fp, C.byref(n), sp)]
            calls += [(ss._h, p, ed, 10, fp, C.byref(n), sp) for p, ed in bad_thresholds]
            for args in calls:
                assert L.msfm_scalespace_detect(*args) == A.MSFM_E_INVAL, args[1:4]
                assert n.value == -7 and (st == -1).all() and not frames.any()
            calls = [(None, 0, ss._h, 0.0, 10.0, 10), (ds._h, 0, None, 0.0, 10.0, 10), (ds._h, -1, ss._h, 0.0, 10.0, 10), (ds._h, 2, ss._h, 0.0, 10.0, 10),
                     (ds._h, 0, foreign._h, 0.0, 10.0, 10), (ds._h, 0, ss._h, 0.0, 10.0, -1), (ds._h, 0, ss._h, 0.0, 10.0, 65536)]
            calls += [(ds._h, 0, ss._h, p, ed, 10) for p, ed in bad_thresholds]
            for args in calls:
                assert L.msfm_descset_extract(*args, 0, sp) == A.MSFM_E_INVAL, args[1:]
                assert (st == -1).all()
                rows, xy = ds.fetch(0)   # found before the first write
                assert np.array_equal(bits(rows), bits(before[0])) and np.array_equal(bits(xy), bits(before[1]))
            # stats may be NULL; the same objects still give the restatement's bits
            assert L.msfm_scalespace_detect(ss._h, 0.0, 10.0, 65535, fp, C.byref(n), None) == A.MSFM_OK and n.value == e["stats"]["n_found"]
            assert np.array_equal(bits(frames[:n.value]), bits(e["frames"]))
            assert L.msfm_descset_extract(ds._h, 1, ss._h, 0.0, 10.0, 65535, 0, None) == A.MSFM_OK
            assert np.array_equal(bits(ds.fetch(1)[0]), bits(before[0]))
            assert np.array_equal(bits(ss.level(O - 1, S + 1)), bits(level_before))
            assert len(foreign.detect()[0]) > 0
    finally:
        other.close()
