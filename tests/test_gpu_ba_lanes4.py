"""Points of up to 4 rows get 4 lanes each in k_point and k_backsub, 64 to a workgroup (ba_device.h, PtMap: the class in front
of S).  Small scenes - 16 cameras, at most a few hundred points - around everything that is particular to that class: only
tracks of 2, only tracks of 4, exactly 64 / 63 / 65 / 129 short points (workgroups full, one short, one over), all four
classes each ending part-way, no short point at all, a camera that sees a point twice, frozen cameras and points with GPS
rows and two intrinsics blocks whose rows meet in one point.  With one intrinsics block and the fold tables on, the
intrinsics x camera products read the Tm of a 4-lane point from beside the record store, not from inside it; with two blocks
a point has two Tm entries, each a sum over part of its four lanes, and those products stay on the gather lists.  Each scene
with the fold tables forced on and on the gather path: parity with the CPU oracle at check_parity's own tolerances, two runs
bitwise, host-built structures against device-built ones bitwise, and layout() against numpy."""
import numpy as np
import pytest

from metricsfm_amd import _abi as A
from metricsfm_amd import scene

from tests.test_gpu_ba import check_parity

pytestmark = pytest.mark.gpu

N_CAMS = 16


def _scene(lengths, seed, twice=()):
    """A ring scene (every camera sees every point) thinned to the given track lengths.  Point p keeps lengths[p] cameras; a
    track longer than the camera count keeps them all and sees some a second time (another feature of the same image: the same
    projection, its own noise).  Points listed in `twice` have their second row moved to the camera of their first."""
    lengths = np.asarray(lengths, np.int64)
    sc = scene.make_ring_scene(N_CAMS, len(lengths), seed=seed, rot_sigma=0.02, trans_sigma=0.2, point_sigma=0.2)
    rng = np.random.default_rng(seed)
    rows = []   # (the ring scene's observations are point-major with the cameras in order: row p * N_CAMS + c)
    for p, k in enumerate(lengths):
        cams = np.sort(rng.choice(N_CAMS, min(int(k), N_CAMS), replace=False))
        if k > N_CAMS:
            cams = np.concatenate([cams, np.sort(rng.choice(N_CAMS, int(k) - N_CAMS, replace=False))])
        if p in twice:
            cams[1] = cams[0]
        rows.append(p * N_CAMS + cams)
    rows = np.concatenate(rows)
    again = np.ones(len(rows), bool)   # a second sighting of the point by the camera
    again[np.unique(rows, return_index=True)[1]] = False
    sc.obs_cam, sc.obs_pt = sc.obs_cam[rows], sc.obs_pt[rows]
    sc.obs_xy = sc.obs_xy[rows] + again[:, None] * rng.standard_normal((len(rows), 2)) * 0.5
    assert (np.bincount(sc.obs_pt, minlength=len(lengths)) == lengths).all()
    return sc


def _cycle(values, n):
    return [values[i % len(values)] for i in range(n)]


_MIX4 = [2, 8, 9, 17, 3, 5, 16, 20, 4, 6, 12, 18, 2, 7]   # per 14: Q 4, S 4, L 3, X 3, in no order


def _cases():
    # name, track lengths, what else (None, "twice", "masks")
    yield "all_two_rows", [2] * 200, None                         # (one equation per point beyond its own unknowns: enough of them for the cameras)
    yield "all_four_rows", [4] * 70, None                         # 640 entries and up to 136 slots in the full workgroup: more than one pass
    yield "short_64", _cycle([2, 3, 4], 64), None                  # one full workgroup
    yield "short_63", _cycle([3, 4, 2], 63), None                  # one short
    yield "short_65", _cycle([4, 2, 3], 65), None                  # one over
    yield "short_129", _cycle([2, 4, 3, 3], 129), None             # two and one over
    yield "four_classes_partly_filled", _cycle(_MIX4, 250), None   # Q 71, S 71, L 54, X 54: every class ends part-way
    yield "no_short_point", _cycle([5, 8, 9, 16, 17, 6, 12, 21, 7], 120), None
    yield "camera_twice", _cycle([2, 3, 4, 4, 3], 90), "twice"
    yield "masks_gps_two_models", _cycle(_MIX4[:12] + [3, 4, 2, 4], 200), "masks"


def _arrays_factory(lengths, extra):
    twice = set(range(0, len(lengths), 4)) if extra == "twice" else ()
    sc = _scene(lengths, seed=900 + len(lengths), twice=twice)
    kw = {}
    if extra == "masks":
        rng = np.random.default_rng(11)
        sc.cam_model = np.tile(sc.cam_model, (2, 1))
        sc.cam_model_of_cam = (np.arange(N_CAMS) % 2).astype(np.int32)   # neighbouring cameras differ: the rows of a point meet both
        gps = sc.cam_pose_gt[:, 3:] + rng.standard_normal((N_CAMS, 3)) * 0.5
        kw = dict(cam_mutable=(np.arange(N_CAMS) % 7 != 3).astype(np.uint8), pt_mutable=(rng.random(len(lengths)) > 0.15).astype(np.uint8),
                  gps_xyz=gps, gps_weight=40.0)
    return sc, kw, (lambda: A.BaArrays.from_scene(sc, **kw))


def _solve(ctx, arrays):
    from metricsfm_amd import capi
    a = arrays()
    r = ctx.ba_solve(a, capi.default_options(max_num_iterations=8))
    return r["iterations"]["cost"].copy(), r["iterations"]["gradient_max_norm"].copy(), a.cam_pose, a.cam_model, a.point


def _same(x, y):
    for u, v in zip(x, y):
        np.testing.assert_array_equal(u, v)


@pytest.mark.parametrize("name,lengths,extra", list(_cases()), ids=[c[0] for c in _cases()])
def test_ba_four_lanes_for_short_tracks(ctx, oracle, monkeypatch, name, lengths, extra):
    sc, kw, arrays = _arrays_factory(lengths, extra)
    lengths = np.asarray(lengths)
    if extra == "masks":   # points whose rows belong to both intrinsics blocks, short ones among them
        both = np.array([len(set(sc.cam_model_of_cam[sc.obs_cam[sc.obs_pt == p]])) == 2 for p in range(len(lengths))])
        assert (both & (lengths <= 4)).sum() > 20
    # the class counts: every free point with a row is eliminated, and every row of it counts
    free = np.ones(len(lengths), bool) if "pt_mutable" not in kw else kw["pt_mutable"].astype(bool)
    want = dict(npb_S4=int((free & (lengths <= 4)).sum()), npb_S=int((free & (lengths <= 8)).sum()),
                npb_L=int((free & (lengths > 8) & (lengths <= 16)).sum()), npb_X=int((free & (lengths > 16)).sum()))
    if name == "no_short_point":
        assert want["npb_S4"] == 0
    opts = dict(max_num_iterations=10)
    monkeypatch.setenv("MSFM_LANES4_MIN", "0")   # (a problem this small would keep its short points in the 8-lane class)
    # fold forced on (the 4-, 8- and 16-lane workgroups form their Schur products themselves, the X ones stay on the gather lists)
    monkeypatch.setenv("MSFM_FOLD_MIN", "0")
    ba = ctx.ba(arrays())
    lay = ba.layout()
    ba.close()
    print(name, {k: lay[k] for k in want}, lay["fold"])
    assert {k: lay[k] for k in want} == want
    assert lay["fold"]["cc_entries_folded"] > 0
    if want["npb_X"] == 0:   # (no workgroup is too large to stage: a full 4-lane workgroup is split into passes)
        assert lay["fold"]["cc_entries_folded"] == lay["fold"]["cc_entries"] and lay["fold"]["mc_entries_folded"] == lay["fold"]["mc_entries"]
    else:
        assert lay["fold"]["cc_entries_folded"] < lay["fold"]["cc_entries"]
    check_parity(ctx, oracle, arrays, opts)
    dev = _solve(ctx, arrays)
    _same(dev, _solve(ctx, arrays))                    # the same problem twice
    monkeypatch.setenv("MSFM_CREATE_HOST", "1")
    ba = ctx.ba(arrays())
    assert {k: ba.layout()[k] for k in want} == want
    ba.close()
    _same(dev, _solve(ctx, arrays))                    # host-built structures
    monkeypatch.delenv("MSFM_CREATE_HOST")
    # the gather path
    monkeypatch.delenv("MSFM_FOLD_MIN")
    monkeypatch.setenv("MSFM_NO_FOLD", "1")
    ba = ctx.ba(arrays())
    assert ba.layout()["fold"]["cc_entries_folded"] == 0
    ba.close()
    check_parity(ctx, oracle, arrays, opts)
    gat = _solve(ctx, arrays)
    _same(gat, _solve(ctx, arrays))
    monkeypatch.setenv("MSFM_CREATE_HOST", "1")
    _same(gat, _solve(ctx, arrays))
