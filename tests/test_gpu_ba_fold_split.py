"""The fold phase of k_point cuts a long slot into parts (ba.hip: fold_parts, k_fold_passes): up to four quads of one 16-lane
row sum contiguous ranges of the slot's entries, the quad of part 0 adds the parts up in a fixed order and stores the slot's one
partial.  Small scenes on 16 cameras around everything that is particular to the cut: every slot filling four parts exactly,
one point more (a second workgroup with nothing to cut), slot lengths on both sides of each boundary of the rule, 16-lane and
4-lane workgroups with several passes, a camera that sees a point twice (cross entries in a cut diagonal slot), the intrinsics
x camera products inside the cut diagonal slots (one intrinsics block) and on the gather lists (two blocks, with frozen cameras
and points and GPS rows), and a scene in which no slot is cut.  Each scene with the fold tables forced on: parity with
the CPU oracle at check_parity's own tolerances, folded and on the gather path; two runs bitwise; host-built structures against
device-built ones bitwise; and layout()["fold"] against the rule applied in numpy to the slots of the scene."""
import numpy as np
import pytest

from metricsfm_amd import _abi as A
from metricsfm_amd import scene

from tests.test_gpu_ba import check_parity

pytestmark = pytest.mark.gpu

N_CAMS = 16
# the rule (ba.hip): a slot of more than CAP entries is cut into parts of CAP entries and the rest in the last one, MAX_PARTS at
# the most - a slot of more than MAX_PARTS * CAP entries into MAX_PARTS parts as equal as they come; a workgroup with a cut slot fills up to QUADS_CUT quads per pass and turns the wave order round in
# the odd rounds, one without keeps SLOTS_UNCUT slots per pass; a pass holds WORDS words (quad headers in fours + entries)
CAP, MAX_PARTS, QUADS_CUT, SLOTS_UNCUT, WORDS = 8, 4, 256, 128, 1024
POINTS_PER_WG = {4: 64, 8: 32, 16: 16}


def _scene(cams_of_point, seed):
    """A ring scene (every camera sees every point) thinned to the given cameras of every point.  A camera listed twice sees the
    point a second time (another feature of the same image: the same projection, its own noise)."""
    sc = scene.make_ring_scene(N_CAMS, len(cams_of_point), seed=seed, rot_sigma=0.02, trans_sigma=0.2, point_sigma=0.2)
    rng = np.random.default_rng(seed)
    # (the ring scene's observations are point-major with the cameras in order: row p * N_CAMS + c)
    rows = np.concatenate([p * N_CAMS + np.asarray(c, np.int64) for p, c in enumerate(cams_of_point)])
    again = np.ones(len(rows), bool)
    again[np.unique(rows, return_index=True)[1]] = False
    sc.obs_cam, sc.obs_pt = sc.obs_cam[rows], sc.obs_pt[rows]
    sc.obs_xy = sc.obs_xy[rows] + again[:, None] * rng.standard_normal((len(rows), 2)) * 0.5
    assert (np.bincount(sc.obs_pt, minlength=len(cams_of_point)) == [len(c) for c in cams_of_point]).all()
    return sc


def _upper_cameras(n):
    """n points of 4 rows on cameras 8..15, every camera in at most 8 of them: they give the upper cameras their rows from a
    4-lane workgroup in which no slot is cut."""
    assert n <= 16
    return [sorted(8 + (p + k) % 8 for k in range(4)) for p in range(n)]


def _with_counts(want, n_points=64):
    """n_points points of 3 or 4 rows such that camera c is seen by want[c] of them (largest remaining demand first)."""
    left = np.array(want)
    total = int(left.sum())
    assert 3 * n_points <= total <= 4 * n_points
    out = []
    for p in range(n_points):
        k = 4 if p < total - 3 * n_points else 3
        cams = np.argsort(-left, kind="stable")[:k]
        left[cams] -= 1
        out.append(sorted(int(c) for c in cams))
    assert (left == 0).all()
    return out


# slots of 40 entries (more than four caps: parts of 10), 33 (9 + 8 + 8 + 8), 25 (8 + 8 + 8 + 1), 24 (three caps), 17
# (8 + 8 + 1), 16, 9 (one more than the cap: 8 + 1) and 8 (the cap: not cut) on the camera diagonals of one 4-lane workgroup
_BOUNDARY_COUNTS = [40, 9, 8, 33, 17, 25, 24, 16, 8, 8, 8, 8, 8, 8, 8, 8]


def _cases():
    # name, cameras of every point, what else (None, "masks"), whether a slot is cut
    same8 = list(range(8))
    yield "exact_fill", [same8] * 32 + _upper_cameras(16), None, True
    yield "one_point_over", [same8] * 33 + _upper_cameras(16), None, True
    yield "rule_boundaries", _with_counts(_BOUNDARY_COUNTS), None, True
    yield "sixteen_lanes", [list(range(16))] * 16, None, True
    rng = np.random.default_rng(70)
    yield "four_lanes_passes", [sorted(rng.choice(N_CAMS, 4, replace=False)) for _ in range(70)], None, True
    yield "camera_twice", [([0] + same8[:7]) if p % 4 == 0 else same8 for p in range(32)] + _upper_cameras(16), None, True
    yield "masks_gps_two_models", [same8] * 40 + [list(range(4, 16))] * 20 + _upper_cameras(16) + [[0, 1, 2], [3, 9]] * 10, "masks", True
    yield "nothing_to_cut", [sorted((p + k) % N_CAMS for k in range(8)) for p in range(16)], None, False


def _parts(c):
    if c > MAX_PARTS * CAP:
        return [c // MAX_PARTS + (1 if k < c % MAX_PARTS else 0) for k in range(MAX_PARTS)]
    return [CAP] * (c // CAP) + ([c % CAP] if c % CAP else [])


def _wave_steps(quads, flip):
    """Entry steps of the four waves over the quads of one pass, in position order: sixteen quads per wave and round."""
    w = [0, 0, 0, 0]
    for b in range(0, len(quads), 16):
        rd, wv = b // 64, (b // 16) % 4
        w[3 - wv if flip and rd % 2 else wv] += max(quads[b:b + 16])
    return w


def _model(cams_of_point):
    """layout()["fold"]'s slots / passes / parts / crit_steps / crit_steps_unsplit / wave_steps from the scene alone.  Points
    by class (4, 8, 16 lanes), inside a class by their four smallest cameras, then by index; workgroups of 64 / 32 / 16; a
    slot per (workgroup, camera pair), the camera diagonals first, then by falling entry count, then by pair."""
    fig = dict(slots=0, passes=0, parts=0, crit_steps=0, crit_steps_unsplit=0, wave_steps=0)
    for lanes, per in POINTS_PER_WG.items():
        pts = [p for p, c in enumerate(cams_of_point) if lanes // 2 < len(c) <= lanes or (lanes == 4 and len(c) <= 4)]
        pts.sort(key=lambda p: ((sorted(cams_of_point[p]) + [0xFFFF] * 4)[:4], p))
        for a in range(0, len(pts), per):
            count = {}
            for p in pts[a:a + per]:
                for ci in cams_of_point[p]:
                    for cj in cams_of_point[p]:
                        if ci >= cj:
                            count[(ci, cj)] = count.get((ci, cj), 0) + 1
            slots = sorted(count.items(), key=lambda s: (s[0][0] != s[0][1], -s[1], s[0]))
            cut = any(c > CAP for _, c in slots)
            fig["slots"] += len(slots)

            def passes(parts_of, bound):
                out, quads, ent = [], [], 0
                for _, c in slots:
                    p = parts_of(c)
                    idle = 4 - len(quads) % 4 if len(p) > 1 and len(quads) % 4 + len(p) > 4 else 0
                    n = len(quads) + idle + len(p)
                    if quads and (n > bound or -(-n // 4) * 4 + ent + c > WORDS):
                        out.append(quads)
                        quads, ent, idle = [], 0, 0
                    quads, ent = quads + [0] * idle + p, ent + c
                return out + [quads]
            built = passes(_parts, QUADS_CUT if cut else SLOTS_UNCUT)
            fig["passes"] += len(built)
            fig["parts"] += sum(q > 0 for quads in built for q in quads)
            fig["crit_steps"] += sum(max(_wave_steps(quads, cut)) for quads in built)
            fig["wave_steps"] += sum(sum(_wave_steps(quads, cut)) for quads in built)
            fig["crit_steps_unsplit"] += sum(max(_wave_steps(quads, False)) for quads in passes(lambda c: [c], SLOTS_UNCUT))
    return fig


def test_the_rule_in_numpy():
    assert [_parts(c) for c in (8, 9, 16, 17, 24, 25, 32, 33, 40)] == [[8], [8, 1], [8, 8], [8, 8, 1], [8, 8, 8], [8, 8, 8, 1], [8] * 4, [9, 8, 8, 8], [10] * 4]
    m = _model([list(range(8))] * 32)   # 36 slots of 32 entries: 28 in the first pass, 8 in the second
    assert m == dict(slots=36, passes=2, parts=144, crit_steps=24, crit_steps_unsplit=64, wave_steps=32 + 24 + 16)


def _arrays_factory(cams_of_point, extra, seed):
    sc = _scene(cams_of_point, seed)
    kw = {}
    if extra == "masks":
        rng = np.random.default_rng(11)
        sc.cam_model = np.tile(sc.cam_model, (2, 1))
        sc.cam_model_of_cam = (np.arange(N_CAMS) % 2).astype(np.int32)   # neighbouring cameras differ: the rows of a point meet both
        gps = sc.cam_pose_gt[:, 3:] + rng.standard_normal((N_CAMS, 3)) * 0.5
        kw = dict(cam_mutable=(np.arange(N_CAMS) % 7 != 3).astype(np.uint8), pt_mutable=(rng.random(len(cams_of_point)) > 0.15).astype(np.uint8),
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


@pytest.mark.parametrize("name,cams_of_point,extra,cut", list(_cases()), ids=[c[0] for c in _cases()])
def test_ba_fold_cuts_long_slots(ctx, oracle, monkeypatch, name, cams_of_point, extra, cut):
    sc, kw, arrays = _arrays_factory(cams_of_point, extra, seed=1200 + len(cams_of_point))
    opts = dict(max_num_iterations=10)
    monkeypatch.setenv("MSFM_LANES4_MIN", "0")   # (a problem this small would keep its short points in the 8-lane class)
    monkeypatch.setenv("MSFM_FOLD_MIN", "0")     # (and on the gather path)
    ba = ctx.ba(arrays())
    fold = ba.layout()["fold"]
    ba.close()
    print(name, fold)
    assert fold["cc_entries_folded"] == fold["cc_entries"] > 0
    if extra == "masks":   # two intrinsics blocks: the intrinsics x camera products stay on the gather lists
        assert fold["mc_entries_folded"] == 0 and fold["mc_slots"] == 0
    else:                  # one: they are formed in the diagonal slots, cut or not
        assert fold["mc_entries_folded"] == fold["mc_entries"] > 0
        want = _model(cams_of_point)
        print(name, want)
        assert {k: fold[k] for k in want} == want
    assert fold["slots"] <= fold["parts"] <= QUADS_CUT * fold["passes"]
    assert fold["crit_steps"] <= fold["crit_steps_unsplit"] and fold["crit_steps"] <= fold["wave_steps"] <= 4 * fold["crit_steps"]
    if cut:
        assert fold["parts"] > fold["slots"]
    else:
        assert fold["parts"] == fold["slots"] and fold["crit_steps"] == fold["crit_steps_unsplit"]
    if name == "exact_fill":
        assert fold["crit_steps"] * 2 <= fold["crit_steps_unsplit"]
    if name == "one_point_over":
        # the second workgroup of the 8-lane class holds one point: 36 slots of one entry, one step in each of three waves, and
        # the same figures cut and uncut
        alone = _model([list(range(8))])
        assert alone["parts"] == alone["slots"] == 36 and alone["crit_steps"] == alone["crit_steps_unsplit"] == 1
        first = _model(cams_of_point[:32] + cams_of_point[33:])
        assert {k: fold[k] - first[k] for k in alone} == alone
    if name == "sixteen_lanes":       # 136 slots of 16 entries in one workgroup: three passes by their words
        assert fold["passes"] == 3
    check_parity(ctx, oracle, arrays, opts)
    dev = _solve(ctx, arrays)
    _same(dev, _solve(ctx, arrays))                    # the same problem twice
    monkeypatch.setenv("MSFM_CREATE_HOST", "1")
    ba = ctx.ba(arrays())
    assert ba.layout()["fold"] == fold
    ba.close()
    _same(dev, _solve(ctx, arrays))                    # host-built structures
    monkeypatch.delenv("MSFM_CREATE_HOST")
    # the gather path
    monkeypatch.delenv("MSFM_FOLD_MIN")
    monkeypatch.setenv("MSFM_NO_FOLD", "1")
    ba = ctx.ba(arrays())
    assert ba.layout()["fold"]["cc_entries_folded"] == 0 and ba.layout()["fold"]["parts"] == 0
    ba.close()
    check_parity(ctx, oracle, arrays, opts)
