"""tests/newpoints_ref.cpp - the sequential restatement of IncrementalSfM::GenerateNew3DPoints (sfm_incremental.cc:755-915)
that the GPU tests hold msfm_new_points to, bit for bit - against the oracle's literal loop (oracle.generate_new_points: one
contracted Trianglate2 per candidate): same selection and order, X and mse to 1e-9 relative.  The margins that make this
comparison fair are asserted on the restatement's own values: no sqrt(mse) within 1e-6 of the gate, no accepted mse within 1e-6
of an integer (the sort key truncates it), no ray cosine within 1e-9 of the cosine it is compared with."""
import os

import numpy as np
import pytest

from tests import newpoints_data as D
from tests import newpoints_ref as NR

GOLD = os.path.join(os.path.dirname(__file__), "golden", "newpoints_golden.npz")
SEED_WALK, SEED_CLAIMS, SEED_DEGENERATE = D.SEED_WALK, D.SEED_CLAIMS, D.SEED_DEGENERATE


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return NR.build_ref(tmp_path_factory.mktemp("newpoints_ref"))


def margins(r, th=3.0, nan_entries=()):
    """Two kinds of value have no rounding to guard against and are left out: a NaN (the rays of two cameras at one centre,
    whose LLT got through on a rounding residue) fails `sqrt(mse) > th` and `cos < cos_min` alike under any rounding, so such
    a candidate is rejected either way; and the 100000.0 of a point behind a camera is an assigned constant.  A NaN may occur
    only in the visible entries `nan_entries` (the coincident-centre entry of the degenerate case), nowhere else."""
    d = r["diag"]
    solved = (d["state"] > 0) & np.isfinite(d["rmse"]) & np.isfinite(d["cos"])
    assert (d["state"][(d["state"] > 0) & ~solved] == 1).all()
    entry = np.repeat(np.arange(len(r["n_candidates"])), r["n_candidates"])      # the diagnostics are one row per candidate, in walk order
    assert len(entry) == len(d["state"]) and set(entry[(d["state"] > 0) & ~solved].tolist()) <= set(nan_entries)
    assert (np.abs(d["rmse"][solved] - th) >= 1e-6).all()
    assert (np.abs(d["cos"][solved] - d["cos_min"][solved]) >= 1e-9).all()
    m = r["mse"][r["mse"] != 100000.0]
    assert (np.abs(m - np.rint(m)) >= 1e-6).all()


def against_oracle(O, L, c, th=3.0, nan_entries=(), **opts):
    r = NR.new_points(L, *D.ref_args(c), diagnostics=True, **opts)
    margins(r, th, nan_entries)
    for k in range(len(c["new_cam"])):
        X, mse, cam2, f1, f2 = O.generate_new_points(*D.legacy_args(c, k), **opts)
        b, e = r["pt_off"][k], r["pt_off"][k + 1]
        assert e - b == len(mse)
        np.testing.assert_array_equal(r["cam2"][b:e], cam2)
        np.testing.assert_array_equal(r["feat1"][b:e], f1)
        np.testing.assert_array_equal(r["feat2"][b:e], f2)
        np.testing.assert_allclose(r["X"][b:e], X, rtol=1e-9, atol=0)
        np.testing.assert_allclose(r["mse"][b:e], mse, rtol=1e-9, atol=0)
    return r


def test_walk_against_the_oracle(oracle, L):
    c = D.walk_case(SEED_WALK)
    r = against_oracle(oracle, L, c)
    n = len(D.WALK_VISIBLE)
    assert r["n_matches"][:n].tolist() == D.WALK_N_MATCHES and r["large"][:n].tolist() == D.WALK_LARGE
    assert r["n_candidates"][:n].tolist() == D.WALK_N_CANDIDATES and r["n_accepted"][:n].tolist() == D.WALK_N_ACCEPTED
    keys = r["mse"][:r["pt_off"][1]].astype(np.int64)
    assert (np.diff(keys) >= 0).all() and len(np.unique(keys)) >= 3 and np.bincount(keys).max() > 1      # several integers, with ties
    # ties keep the walk order
    walk = r["vis_entry"][:r["pt_off"][1]].astype(np.int64) * 1000 + r["pt_match"][:r["pt_off"][1]]
    assert all((np.diff(walk[keys == v]) > 0).all() for v in np.unique(keys))
    # the new camera listed twice is walked twice: both halves of new camera 2's entries [3, 0, 0] agree
    assert r["n_accepted"][-1] == r["n_accepted"][-2] > 0


def test_claims_against_the_oracle(oracle, L):
    c = D.claims_case(SEED_CLAIMS)
    r = against_oracle(oracle, L, c)
    sel = np.nonzero(r["feat1"] == c["shared_f1"])[0]
    assert len(sel) == 3 and r["takes1"][sel].tolist() == [1, 0, 0]
    assert r["vis_entry"][sel].tolist() == [1, 2, 0] and r["mse"][sel].astype(int).tolist() == [0, 0, 2]   # the tie goes to the earlier entry
    sel = np.nonzero((r["feat2"] == c["shared_f2"]) & (r["cam2"] == c["shared_f2_cam"]))[0]
    assert len(sel) == 2 and r["takes2"][sel].tolist() == [1, 0] and r["pt_match"][sel[0]] > r["pt_match"][sel[1]]
    other = np.ones(len(r["feat1"]), bool)
    other[sel] = False
    assert r["takes2"][other].all()


def test_degenerate_against_the_oracle(oracle, L):
    c = D.degenerate_case(SEED_DEGENERATE)
    r = against_oracle(oracle, L, c, nan_entries=(0,))      # entry 0: the visible camera at the new camera's centre
    assert r["n_matches"].tolist() == D.DEGENERATE_N_MATCHES and r["n_accepted"].tolist() == D.DEGENERATE_N_ACCEPTED
    r = against_oracle(oracle, L, c, th=400.0, nan_entries=(0,), th_mse_reprojection=400.0)
    assert r["n_accepted"].tolist() == D.DEGENERATE_N_ACCEPTED_400
    behind = r["vis_entry"] == 1
    assert (r["mse"][behind] == 100000.0).all() and behind[-12:].all()     # the key 100000 sorts last


def test_golden_fixture_reproduces(L):
    g = np.load(GOLD)
    c = {k: g[k] for k in D.INPUTS}
    fresh = D.golden_case()
    for k in D.INPUTS:
        np.testing.assert_array_equal(c[k], fresh[k], err_msg=k)
    r = NR.new_points(L, *D.ref_args(c), diagnostics=True, **D.GOLDEN_OPTS)
    margins(r)
    for k in NR.FETCHED:
        np.testing.assert_array_equal(r[k], g["want_" + k], err_msg=k)
    assert g["want_large"].tolist() == [0, 0, 0, 1, 0, 0, 0] and np.diff(g["want_pt_off"]).tolist() == [66, 17]
