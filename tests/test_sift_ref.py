"""The two restatements of "Describing given SIFT frames" (tests/sift_ref.cpp, tests/sift_ref.py) against each other and against
the properties the definitions imply.  No device."""
import numpy as np

from tests import sift_data as D
from tests import sift_ref as R

F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def test_restatements_agree_bit_for_bit():
    O, S = 2, 5
    img = D.image(40, 33, 5)
    planes = D.run_ref_cpp(img, O, S, np.zeros((0, 4), F32))
    rng = np.random.default_rng(6)
    frames = [(rng.uniform(8, 32), rng.uniform(8, 25), D.sigma_for(S, o, i_s), rng.uniform(-4, 4)) for o in range(O) for i_s in range(S)]
    frames += [(1.5, 30.5, 1.2, 0.0), (-3.0, 5.0, 2.0, 1.0), (20.0, 16.0, 500.0, -2.0), (20.0, 16.0, 0.01, 2.0)]
    frames = np.array(frames, F32)
    cpp = D.run_ref_cpp(img, O, S, frames)
    taps, T = R.host_numbers(S)
    gss, mod, ang = R.scalespace(img, O, S, taps)
    for o in range(O):
        for s in range(S + 3):
            assert np.array_equal(bits(gss[o][s]), bits(cpp["gss"][o][s])), (o, s - 1)
        for s in range(S):
            assert np.array_equal(bits(mod[o][s]), bits(cpp["mod"][o][s])), (o, s)
            assert np.array_equal(bits(ang[o][s]), bits(cpp["ang"][o][s])), (o, s)
    assert np.array_equal(bits(planes["gss"][1][3]), bits(cpp["gss"][1][3]))   # the planes do not depend on the frames
    rec = R.frame_records(frames, O, S)
    assert sorted(set(zip(rec["o"].tolist(), rec["is"].tolist()))) == [(o, i_s) for o in range(O) for i_s in range(S)]
    for q in (0, 1):
        for f, F in enumerate(rec):
            row = R.describe(F, mod[F["o"]][F["is"]], ang[F["o"]][F["is"]], T, q)
            assert np.array_equal(bits(row), bits(cpp["rows"][q][f])), (q, f)
    assert not cpp["rows"][0][len(frames) - 3].any() and cpp["rows"][0][0].any()   # the frame left of the image / an interior one


def test_blur_keeps_a_constant_image_constant():
    """A constant image stays constant under every blur of every level count: all pixels equal (the borders clamp, so every pixel is
    the same ordered sum), far inside the 1 ulp of 255 (2^-16) that is allowed between them.  The common value itself is not 255
    to 1 ulp, and the definitions do not promise that: the taps are rounded after their normalisation and the n = 2 W + 1 products
    are added one by one, so a pass may move the value by (n / 2 + 2) ulp - 2^-17 per addition, 2^-16 for the taps' rounding, 2^-16
    for the products' - and a blur is two passes: (n + 4) ulp, asserted.  Measured: one pass at most 1 ulp for every tap set of
    S = 5 and at most 2 ulp over S = 1 .. 8; rows and columns together at most 2 ulp at S = 5 (3 ulp at S = 1 and S = 6)."""
    ulp = 2.0 ** -16
    for S in range(1, 9):
        taps, _ = R.host_numbers(S)
        moved = []
        for g in taps:
            out = R.blur(np.full((23, 31), 255.0, F32), g)
            assert float(out.max()) - float(out.min()) <= ulp, (S, len(g))
            moved.append(float(np.abs(out.astype(np.float64) - 255.0).max()) / ulp)
            assert moved[-1] <= len(g) + 4, (S, len(g), moved[-1])
        print("S = %d: the value moves by %s ulp of 255" % (S, moved))


def test_rows_are_normalised_and_clipped():
    for name in D.CASES:
        e = D.expected(name)
        rows = e["rows"][0].astype(np.float64) / 512.0
        live = rows.any(axis=1)
        assert live.sum() >= len(rows) - 8
        n2 = (rows[live] ** 2).sum(axis=1)
        assert np.abs(n2 - 1.0).max() < 1e-5, np.abs(n2 - 1.0).max()
        assert (e["rows"][1] <= 255).all() and (e["rows"][1] == np.trunc(e["rows"][1])).all()
        if "constant" in e["idx"]:
            assert not e["rows"][0][e["idx"]["constant"]].any()
        for f in e["idx"]["outside"]:
            assert not e["rows"][0][f].any()
        a, b = e["idx"]["twins"]
        assert np.array_equal(e["rows"][0][a], e["rows"][0][b]) and e["rows"][0][a].any()
        rec = e["records"]
        O, S = D.CASES[name][3], D.CASES[name][4]
        assert set(zip(rec["o"].tolist(), rec["is"].tolist())) == {(o, i_s) for o in range(O) for i_s in range(S)}
        assert rec["o"][e["idx"]["clamp_low"]] == 0 and rec["is"][e["idx"]["clamp_low"]] == 0
        assert rec["o"][e["idx"]["clamp_high"]] == O - 1 and rec["is"][e["idx"]["clamp_high"]] == S - 1


def test_no_entry_above_the_clip_over_the_second_norm():
    e = D.expected("a")
    _, T = R.host_numbers(5)
    for f in (0, 7, 14, 21, 29, e["idx"]["clamp_low"]):
        F, norms = e["records"][f], []
        row = R.describe(F, e["mod"][F["o"]][F["is"]], e["ang"][F["o"]][F["is"]], T, 0, norms)
        assert np.array_equal(bits(row), bits(e["rows"][0][f])), f
        assert row.any() and row.max() <= F32(512.0) * (F32(0.2) / norms[1]), f
        assert abs(float(norms[1]) - 1.0) < 1.0   # the clipped vector's norm: at most the unit norm it was cut from


def test_transpose_permutation_is_an_involution():
    assert sorted(R.PERM.tolist()) == list(range(128))
    assert np.array_equal(R.PERM[R.PERM], np.arange(128))


def test_restatement_under_the_host_sanitizers():
    exe = D.ref_exe(("-O1", "-g", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    img = D.image(40, 33, 5)
    frames = np.array([(20.0, 16.0, 2.0, 0.5), (1.0, 1.0, 9.0, 3.0), (38.6, 30.9, 0.3, -1.0), (-9.0, 4.0, 2.0, 0.0), (20.0, 16.0, 3.0e38, 1.0)], F32)
    out = D.run_ref_cpp(img, 2, 5, frames, exe=exe)
    assert np.array_equal(bits(out["rows"][0]), bits(D.run_ref_cpp(img, 2, 5, frames)["rows"][0]))
