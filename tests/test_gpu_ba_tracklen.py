"""The point kernels group the eliminated points by track length (ba.hip, PtMap): up to 8 rows (S: 8 lanes per point), 9..16
rows (L: 16 lanes per point), more (X: rounds of 8), class-major, no workgroup mixing classes.  Small scenes with every mix
of lengths - partly filled and exactly filled workgroups, frozen cameras and points, GPS rows, two intrinsics blocks - each
against the CPU oracle with the Schur products folded into k_point and on the gather path, the host-built structures against
the device-built ones bitwise, two runs bitwise, and the class counts of layout() against numpy."""
import numpy as np
import pytest

from metricsfm_amd import _abi as A
from metricsfm_amd import scene

from tests.test_gpu_ba import check_parity

pytestmark = pytest.mark.gpu

N_CAMS = 30


def _scene(lengths, seed):
    """A ring scene (every camera sees every point) thinned to the given track lengths: point p keeps lengths[p] cameras."""
    lengths = np.asarray(lengths, np.int64)
    sc = scene.make_ring_scene(N_CAMS, len(lengths), seed=seed, rot_sigma=0.02, trans_sigma=0.2, point_sigma=0.2)
    rng = np.random.default_rng(seed)
    keep = np.zeros((len(lengths), N_CAMS), bool)
    for p, k in enumerate(lengths):
        keep[p, rng.choice(N_CAMS, int(k), replace=False)] = True
    keep = keep.reshape(-1)   # (the ring scene's observations are point-major with the cameras in order)
    sc.obs_cam, sc.obs_pt, sc.obs_xy = sc.obs_cam[keep], sc.obs_pt[keep], sc.obs_xy[keep]
    assert (np.bincount(sc.obs_pt, minlength=len(lengths)) == lengths).all()
    return sc


def _cycle(values, n):
    return [values[i % len(values)] for i in range(n)]


_MIX = [8, 9, 16, 17, 24, 30, 2, 5, 12, 3, 8, 16, 17, 9, 4]   # S: 6 of 15, L: 5 of 15, X: 4 of 15, in no order


def _cases():
    # name, track lengths, keyword arguments of BaArrays (built from the scene)
    yield "short_partly_filled", _cycle([2, 3, 4, 5, 6, 7, 8], 101), None          # 3 S workgroups + 5 points
    yield "long_partly_filled", _cycle([9, 10, 11, 12, 13, 14, 15, 16], 37), None   # 2 L workgroups + 5 points
    yield "mixed_partly_filled", _cycle(_MIX, 150), None                            # 60 S, 50 L, 40 X: every class ends part-way
    yield "mixed_exactly_filled", [8] * 64 + [17] * 32 + [9, 16] * 16, None         # 2 S, 2 L, 1 X workgroup, all full
    yield "mixed_masks_gps_two_models", _cycle(_MIX, 170), "masks"


def _arrays_factory(name, lengths, extra):
    sc = _scene(lengths, seed=500 + len(lengths))
    kw = {}
    if extra == "masks":
        rng = np.random.default_rng(9)
        sc.cam_model = np.tile(sc.cam_model, (2, 1))
        sc.cam_model_of_cam = (np.arange(N_CAMS) % 2).astype(np.int32)
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
def test_ba_points_grouped_by_track_length(ctx, oracle, monkeypatch, name, lengths, extra):
    sc, kw, arrays = _arrays_factory(name, lengths, extra)
    lengths = np.asarray(lengths)
    # the class counts: every free point with a row is eliminated, and every row of it counts
    free = np.ones(len(lengths), bool) if "pt_mutable" not in kw else kw["pt_mutable"].astype(bool)
    want = dict(npb_S=int((free & (lengths <= 8)).sum()), npb_L=int((free & (lengths > 8) & (lengths <= 16)).sum()),
                npb_X=int((free & (lengths > 16)).sum()))
    opts = dict(max_num_iterations=10)
    # fold forced on (the S and L workgroups form their camera x camera products themselves, the X ones stay on the gather lists)
    monkeypatch.setenv("MSFM_FOLD_MIN", "0")
    ba = ctx.ba(arrays())
    lay = ba.layout()
    ba.close()
    assert {k: lay[k] for k in want} == want
    if want["npb_S"] + want["npb_L"] > 0:
        assert lay["fold"]["cc_entries_folded"] > 0
    if want["npb_X"] > 0:
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
    assert ctx.ba(arrays()).layout()["fold"]["cc_entries_folded"] == 0
    check_parity(ctx, oracle, arrays, opts)
    gat = _solve(ctx, arrays)
    _same(gat, _solve(ctx, arrays))
    monkeypatch.setenv("MSFM_CREATE_HOST", "1")
    _same(gat, _solve(ctx, arrays))
