"""The sequential restatement of the SIFT detector (tests/siftdetect_ref.cpp) on its own: the cases meet every rule the GPU test
compares on, so that it cannot pass on empty ground, and two properties that follow from the definitions of include/msfm.h."""
import numpy as np

from metricsfm_amd import _abi as A
from metricsfm_amd import capi
from tests import sift_data as D
from tests import siftdetect_data as X

F32 = np.float32


def test_the_stats_names_are_the_headers():
    assert X.STATS == A.SIFT_DETECT_STATS and len(X.STATS) == 18
    assert "#define MSFM_SIFT_DETECT_STATS 18" in open(capi._header.HEADER).read()


def test_the_cases_meet_every_rule():
    total = {k: 0 for k in X.STATS}
    every_cell = left = right = accepted_unconverged = 0
    for name, (w, h, stride, O, S, seed, patch) in X.CASES.items():
        e = X.expected(name)
        st, cells, raw = e["stats"], e["cells"], e["raw"]
        print(name, st)
        for k in X.STATS:
            total[k] += st[k]
        status = raw["flags"] & X.KP_STATUS
        assert st["candidates"] == len(raw) == len(cells)
        assert st["candidates"] == st["keypoints"] + sum(st[k] for k in X.STATS if k.startswith("rejected_"))
        assert st["keypoints"] == int((status == 0).sum()) == sum(st["angles_%d" % a] for a in range(5))
        assert st["n_found"] == len(e["frames"]) == sum(a * st["angles_%d" % a] for a in range(5))
        # ascending (o, is, iy, ix) of the detection cell, every cell once
        key = ((cells[:, 0].astype(np.int64) * 8 + cells[:, 1]) * 16384 + cells[:, 2]) * 16384 + cells[:, 3]
        assert np.all(np.diff(key) > 0)
        widths = np.array([w >> o for o in cells[:, 0]])
        left += int((cells[:, 3] == 1).sum())
        right += int((cells[:, 3] == widths - 2).sum())
        every_cell += all(((cells[:, 0] == o) & (cells[:, 1] == s)).any() for o in range(O) for s in range(S))
        accepted_unconverged += int(((status == 0) & ((raw["flags"] & X.KP_UNCONVERGED) != 0)).sum())
        assert st["moved"] == int(((status == 0) & ((raw["flags"] & X.KP_MOVED) != 0)).sum())
        assert np.isfinite(e["frames"]).all() and (e["frames"][:, 2] > 0).all()
    print("together", total, "x = 1:", left, "x = w - 2:", right)
    assert every_cell >= 1, "no case has a candidate in every (o, s)"
    assert total["moved"] >= 1 and total["rejected_edge"] >= 1 and total["rejected_offset"] >= 1 and total["rejected_bounds"] >= 1
    assert accepted_unconverged >= 1 and total["unconverged"] == accepted_unconverged
    assert total["angles_2"] >= 1 and total["angles_3"] + total["angles_4"] >= 1
    assert left >= 1 and right >= 1
    assert 200 <= X.expected("d")["stats"]["candidates"] + X.expected("d")["stats"]["n_found"] < 5000


def test_the_wide_case_crosses_the_kernels_blocks():
    """Case d: three 256-pixel workgroups of the extremum kernel in x, several in y, and candidates in mask words on both sides of
    the scan's 1024-word blocks (a level of octave 0 is 130 rows of 10 words)."""
    w, h, stride, O, S, seed, patch = X.CASES["d"]
    cells = X.expected("d")["cells"]
    c0 = cells[cells[:, 0] == 0]
    assert -(-w // 256) == 3 and -(-h // 8) > 4
    assert {int(x) // 256 for x in c0[:, 3]} == {0, 1, 2}
    word = (c0[:, 1] * h + c0[:, 2]) * -(-w // 64) + c0[:, 3] // 64
    assert len(set(int(b) for b in word // 1024)) >= 3


def test_no_candidate_inside_a_constant_patch():
    """Case a's patch is one value.  Further inside it than the blurs reach, every level is spatially constant (its value moves
    by an ulp or two from level to level, so D differs between levels but not inside one): a cell there ties with its eight
    neighbours of its own DoG level, and ties are not extrema."""
    w, h, stride, O, S, seed, (x0, y0, x1, y1) = X.CASES["a"]
    g = X.planes_of("a")["gss"][0]
    cells = X.expected("a")["cells"]
    c0 = cells[cells[:, 0] == 0]
    D3 = np.stack([g[i + 1] - g[i] for i in range(len(g) - 1)])   # D(-1 .. S)
    flat = 0
    for s in range(S):
        for y in range(max(y0, 1), h - 1):
            for x in range(max(x0, 1), w - 1):
                if np.ptp(D3[s + 1, y - 1:y + 2, x - 1:x + 2]) == 0:
                    flat += 1
                    assert not ((c0[:, 1] == s) & (c0[:, 2] == y) & (c0[:, 3] == x)).any(), (s, y, x)
    print("cells of the patch that tie with their level's neighbours:", flat)
    assert flat >= 100


def test_one_symmetric_blob_gives_one_keypoint():
    """A blob of width 4 centred on a pixel, peak_thresh 0.  (A narrower blob need not give one: at width 3 the ring of DoG minima
    around the centre has eight lattice minima that pass every rule, by symmetry all or none; at width 2 the extremum in scale
    lies below level 0 and there is no candidate.  Both are printed.)"""
    O, S = 2, 3
    for width in (2.0, 3.0):
        img = X.blob_image(width=width)
        st = X.run_detect_cpp(D.run_ref_cpp(img, O, S, np.zeros((0, 4), F32)), img.shape[1], img.shape[0], O, S)["stats"]
        print("width", width, "candidates", st["candidates"], "keypoints", st["keypoints"])
    img = X.blob_image(width=4.0)
    h, w = img.shape
    planes = D.run_ref_cpp(img, O, S, np.zeros((0, 4), F32))
    e = X.run_detect_cpp(planes, w, h, O, S)
    raw = e["raw"][(e["raw"]["flags"] & X.KP_STATUS) == 0]
    assert e["stats"]["keypoints"] == 1 == len(raw), e["stats"]
    k = raw[0]
    g = planes["gss"][k["o"]]
    Dk = np.stack([g[i + 1] - g[i] for i in range(len(g) - 1)])
    # the detection level of its extremum: the cell is the strict extremum of its neighbourhood
    nb = Dk[k["is"]:k["is"] + 3, k["iy"] - 1:k["iy"] + 2, k["ix"] - 1:k["ix"] + 2]
    centre = nb[1, 1, 1]
    assert (np.abs(nb) < abs(centre)).sum() == 26
    sc = 1 << int(k["o"])
    assert abs(k["xn"] * sc - 32) < 0.5 and abs(k["yn"] * sc - 32) < 0.5
    assert k["is"] - 1.5 < k["sn"] < k["is"] + 1.5
    print("blob of width 4.0: sigma", e["frames"][0, 2] if len(e["frames"]) else None, "angles", e["stats"]["n_found"])
