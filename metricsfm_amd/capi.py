"""ctypes binding of libmsfm.so (include/msfm.h).  There is no CPU fallback: if the HIP
library is missing or no GPU is visible, every entry point fails loudly."""
import ctypes as C
import os

import numpy as np

from . import _abi as A
from . import _header
from ._header import ALLREDUCE_FN  # noqa: F401  (part of this module's interface)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MSFM_LIB") or os.path.join(_HERE, "libmsfm.so")   # (MSFM_LIB: a differently built libmsfm, for A/B timing)
_lib = None

# {name: (restype, argtypes)} of every function include/msfm.h declares, and their names
with open(_header.HEADER) as _f:
    PROTOTYPES = _header.prototypes(_f.read())
SYMBOLS = list(PROTOTYPES)


class MsfmError(RuntimeError):
    def __init__(self, code, text):
        super().__init__("libmsfm error %d: %s" % (code, text))
        self.code = code


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s not built: run `python -c 'import __graft_entry__ as g; g.build()'` or "
                              "`make -C metricsfm_amd/csrc` (no CPU fallback exists)" % LIB_PATH)
        _lib = _header.bind(C.CDLL(LIB_PATH), PROTOTYPES)
    return _lib


def _set_fields(o, kw):
    for k, v in kw.items():
        if not hasattr(o, k):
            raise AttributeError(k)
        if isinstance(v, dict) and isinstance(getattr(o, k), C.Structure):
            _set_fields(getattr(o, k), v)
        else:
            setattr(o, k, v)


def _options(struct_cls, default_fn_name, kw):
    """struct_cls as the library's default function fills it, then the fields kw names; a nested struct takes a dict of its fields."""
    o = struct_cls()
    getattr(lib(), default_fn_name)(C.byref(o))
    _set_fields(o, kw)
    return o


class _Handle:
    """Owns the library handle `_h`; `close` (also at the end of a `with` block and on collection) hands it to the destroy
    function `_destroy` names.  As it stands it holds a short-lived result: `with _Handle(h, "msfm_x_set_destroy"): ...`."""
    _destroy = None

    def __init__(self, h, destroy):
        self._h, self._destroy = h, destroy

    def close(self):
        if self._h:
            getattr(lib(), self._destroy)(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def default_options(**kw):
    return _options(A.BaOptions, "msfm_ba_options_default", kw)


def epnpf_options(**kw):
    """msfm_epnpf_options with the reference's values (0.5, 4.0, 0.01, 200 samples); keywords override fields."""
    return _options(A.EpnpfOptions, "msfm_epnpf_default_options", kw)


def localize_pose_options(**kw):
    """msfm_localize_pose_options with the reference's values (5.0 px, 20 correspondences, 200 samples, the default sweep, 16 tries);
    keywords override fields, `sweep` takes a dict of msfm_epnpf_options fields."""
    return _options(A.LocalizePoseOptions, "msfm_localize_pose_default_options", kw)


def seed_options(**kw):
    """msfm_seed_options with the reference's values (3.0 px, 3 degrees, 20 points, 100 / 200 samples); keywords override fields."""
    return _options(A.SeedOptions, "msfm_seed_default_options", kw)


def new_points_options(**kw):
    """msfm_new_points_options with the reference's values (3.0 px, 3 and 5 degrees, 500 matches); keywords override fields."""
    return _options(A.NewPointsOptions, "msfm_new_points_default_options", kw)


def round_options(**kw):
    """msfm_round_options with the reference's values (100 iterations for both solves, weights 2.0 / 1.0, 1.0 px); keywords
    override fields, `partial` / `full` take a dict of msfm_ba_options fields."""
    return _options(A.RoundOptions, "msfm_round_default_options", kw)


def epnpf_num_steps(**kw):
    """Candidate focal lengths of the sweep these options describe: (int)((f_ratio_max - f_ratio_min) / f_ratio_step), < 0 if invalid."""
    return lib().msfm_epnpf_num_steps(C.byref(epnpf_options(**kw)))


def gpsreg_options(**kw):
    """msfm_gpsreg_options with the reference's values (window 20, min_views 3, clip 80 degrees, th_outlier 3.0)."""
    return _options(A.GpsregOptions, "msfm_gpsreg_default_options", kw)


def gps_orient_global(cam_R, cam_c, gps, **opts):
    """msfm_gps_orient_global (host only, no context): AbsoluteOrientationWithGPSGlobal, slam_gps.cc:1596-1674.  Returns a
    dict: the transformed cameras cam_R / cam_t / cam_c / cam_aa, the shifted gps, weight, Rg, tg, scale, err, offset."""
    R = A.as_c(np.asarray(cam_R, dtype=np.float64).reshape(-1, 9), np.float64)
    c = A.as_c(np.asarray(cam_c, dtype=np.float64).reshape(-1, 3), np.float64)
    g = A.as_c(np.asarray(gps, dtype=np.float64).reshape(-1, 3), np.float64)
    n = len(c)
    if len(R) != n or len(g) != n:
        raise ValueError("gps_orient_global: cam_R, cam_c and gps must have one row per camera")
    o = gpsreg_options(**opts)
    out = dict(cam_R=np.zeros((n, 9)), cam_t=np.zeros((n, 3)), cam_c=np.zeros((n, 3)), cam_aa=np.zeros((n, 3)), gps=np.zeros((n, 3)),
               weight=np.zeros(n))
    r = A.GpsOrientResult()
    for k, v in out.items():
        setattr(r, k, A.ptr(v, A.c_double_p))
    rc = lib().msfm_gps_orient_global(n, A.ptr(R, A.c_double_p), A.ptr(c, A.c_double_p), A.ptr(g, A.c_double_p), C.byref(o), C.byref(r))
    if rc != 0:
        raise MsfmError(rc, "msfm_gps_orient_global: invalid input (fewer than 3 cameras?)")
    out.update(Rg=np.array(r.Rg).reshape(3, 3), tg=np.array(r.tg), scale=r.scale, err=r.err, offset=np.array(r.offset))
    return out


def _flatten_matches(n_features, pairs, matches_per_pair):
    nf = A.as_c(np.asarray(n_features, dtype=np.int32), np.int32)
    pr = A.as_c(np.asarray(pairs, dtype=np.int32).reshape(-1, 2), np.int32)
    lens = np.array([len(m) for m in matches_per_pair], dtype=np.int64)
    off = np.zeros(len(pr) + 1, dtype=np.int32)
    off[1:] = np.cumsum(lens)
    nonempty = [np.asarray(m, dtype=np.int32).reshape(-1, 2) for m in matches_per_pair if len(m)]
    flat = np.concatenate(nonempty) if nonempty else np.zeros((1, 2), dtype=np.int32)
    return nf, pr, off, A.as_c(flat, np.int32)


def _fetch_track_set(h):
    with _Handle(h, "msfm_track_set_destroy"):
        nt, no = C.c_int32(), C.c_int32()
        lib().msfm_track_set_size(h, C.byref(nt), C.byref(no))
        toff = np.zeros(nt.value + 1, dtype=np.int32)
        oi, of = np.zeros(max(1, no.value), dtype=np.int32), np.zeros(max(1, no.value), dtype=np.int32)
        lib().msfm_track_set_fetch(h, A.ptr(toff, A.c_int_p), A.ptr(oi, A.c_int_p), A.ptr(of, A.c_int_p))
    return toff, oi[:no.value], of[:no.value]


def build_tracks(n_features, pairs, matches_per_pair):
    """SLAMGPS::Triangulation's data association (slam_gps.cc:565-635), the walk over the match lists on the host as the
    reference does it.  n_features[image]; pairs [(idx1, idx2)] in visiting order; matches_per_pair[p] = int array [m][2]
    (feature in idx1, feature in idx2).
    Returns CSR tracks: track_off, obs_image, obs_feature (observations in ascending image order).
    `Context.build_tracks` returns the same from the GPU."""
    nf, pr, off, flat = _flatten_matches(n_features, pairs, matches_per_pair)
    h = C.c_void_p()
    rc = lib().msfm_tracks_build(len(nf), A.ptr(nf, A.c_int_p), len(pr), A.ptr(pr, A.c_int_p), A.ptr(off, A.c_int_p),
                                 A.ptr(flat, A.c_int_p), C.byref(h))
    if rc != 0:
        raise MsfmError(rc, "msfm_tracks_build: invalid input")
    return _fetch_track_set(h)


def build_tracks_flat(n_features, pairs, match_off, matches):
    """`build_tracks` on flat int32 arrays (pairs [P][2], match_off [P+1], matches [M][2])."""
    nf, pr, off = (A.as_c(np.asarray(x, dtype=np.int32), np.int32) for x in (n_features, pairs, match_off))
    fl = A.as_c(np.asarray(matches, dtype=np.int32).reshape(-1, 2), np.int32)
    h = C.c_void_p()
    rc = lib().msfm_tracks_build(len(nf), A.ptr(nf, A.c_int_p), len(pr), A.ptr(pr, A.c_int_p), A.ptr(off, A.c_int_p),
                                 A.ptr(fl, A.c_int_p), C.byref(h))
    if rc != 0:
        raise MsfmError(rc, "msfm_tracks_build: invalid input")
    return _fetch_track_set(h)


def fransac_options(**kw):
    return _options(A.FransacOptions, "msfm_fransac_default_options", kw)


def pair_select_options(**kw):
    """msfm_pair_select_options with the reference's values (30 joined matches, more than 20 inliers, the set's K); keywords
    override fields, and the fields of msfm_fransac_options go to `fransac`."""
    own = {k: v for k, v in kw.items() if k != "fransac" and hasattr(A.PairSelectOptions, k)}
    return _options(A.PairSelectOptions, "msfm_pair_select_default_options", dict(own, fransac={k: kw[k] for k in kw if k not in own}))


def hransac_options(**kw):
    return _options(A.HransacOptions, "msfm_hransac_default_options", kw)


def slam_prior_options(**kw):
    return _options(A.SlamPriorOptions, "msfm_slam_prior_default_options", kw)


def _new_points_set_result(h, nn):
    """The dict `Context.new_points` documents from a msfm_new_points_set of nn new cameras (the caller destroys it)."""
    dp, ip, up = A.c_double_p, A.c_int_p, A.c_u8_p
    n1, npt, ne, nb = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
    lib().msfm_new_points_set_size(h, C.byref(n1), C.byref(npt), C.byref(ne), C.byref(nb))
    npt, ne = npt.value, ne.value
    m, e = max(1, npt), max(1, ne)
    poff = np.zeros(nn + 1, np.int32)
    cam2, f1, f2, ve, ptm = (np.zeros(m, np.int32) for _ in range(5))
    X, mse, t1, t2 = np.zeros((m, 3)), np.zeros(m), np.zeros(m, np.uint8), np.zeros(m, np.uint8)
    nm, ncand, nacc, large = np.zeros(e, np.int32), np.zeros(e, np.int32), np.zeros(e, np.int32), np.zeros(e, np.uint8)
    lib().msfm_new_points_set_fetch(h, A.ptr(poff, ip), A.ptr(cam2, ip), A.ptr(f1, ip), A.ptr(f2, ip), A.ptr(ve, ip), A.ptr(ptm, ip),
                                    A.ptr(X, dp), A.ptr(mse, dp), A.ptr(t1, up), A.ptr(t2, up), A.ptr(nm, ip), A.ptr(large, up),
                                    A.ptr(ncand, ip), A.ptr(nacc, ip))
    return {"pt_off": poff, "cam2": cam2[:npt], "feat1": f1[:npt], "feat2": f2[:npt], "vis_entry": ve[:npt], "pt_match": ptm[:npt],
            "X": X[:npt], "mse": mse[:npt], "takes1": t1[:npt], "takes2": t2[:npt], "n_matches": nm[:ne], "large": large[:ne],
            "n_candidates": ncand[:ne], "n_accepted": nacc[:ne], "h2d_bytes": nb.value}


def _round_set_result(ctx, h, nc, nm, npt, partial, full, keep_problem, capacity):
    """The dict `Context.round_adjust` documents from a msfm_round_set (the caller destroys it)."""
    ip, dp, up = A.c_int_p, A.c_double_p, A.c_u8_p
    nb = C.c_int64()
    lib().msfm_round_set_size(h, None, None, None, C.byref(nb))
    c1, m1, p1 = max(1, nc), max(1, nm), max(1, npt)
    o_pose, o_model, o_R = np.zeros((c1, 6)), np.zeros((m1, 3)), np.zeros((c1, 3, 3))
    o_t, o_c, o_fk, o_xyz, o_mse = np.zeros((c1, 3)), np.zeros((c1, 3)), np.zeros((c1, 3)), np.zeros((p1, 3)), np.zeros(p1)
    o_mut, o_bad, o_added, o_views = np.zeros(p1, np.uint8), np.zeros(p1, np.uint8), np.zeros(p1, np.uint8), np.zeros(p1, np.int32)
    counts, adjust, solved = np.zeros(3, np.int32), np.zeros((2, 2), np.int32), np.zeros(2, np.int32)
    bufs = [A.SummaryBuf(capacity), A.SummaryBuf(capacity)]
    sums = (A.BaSummary * 2)()
    for k in range(2):
        sums[k].iterations, sums[k].iterations_capacity = bufs[k].struct.iterations, capacity
    ctx.check(lib().msfm_round_set_fetch(h, A.ptr(o_pose, dp), A.ptr(o_model, dp), A.ptr(o_R, dp), A.ptr(o_t, dp), A.ptr(o_c, dp), A.ptr(o_fk, dp),
                                         A.ptr(o_xyz, dp), A.ptr(o_mut, up), A.ptr(o_bad, up), A.ptr(o_mse, dp), A.ptr(o_added, up),
                                         A.ptr(o_views, ip), A.ptr(counts, ip), A.ptr(adjust, ip), A.ptr(solved, ip), sums))
    summary = []
    for k in range(2):
        C.memmove(C.byref(bufs[k].struct), C.byref(sums[k]), C.sizeof(A.BaSummary))
        summary.append(bufs[k].result() if solved[k] else None)
    out = {"cam_pose": o_pose[:nc], "cam_model": o_model[:nm], "cam_R": o_R[:nc], "cam_t": o_t[:nc], "cam_c": o_c[:nc], "cam_fk": o_fk[:nc],
           "point_xyz": o_xyz[:npt], "pt_mutable": o_mut[:npt], "pt_bad": o_bad[:npt], "pt_mse": o_mse[:npt], "pt_new_added": o_added[:npt],
           "pt_views": o_views[:npt], "count_outliers": int(counts[0]), "count_new_add": int(counts[1]),
           "count_outliers_new_add": int(counts[2]), "adjust_cams": adjust[:, 0].copy(), "adjust_pts": adjust[:, 1].copy(), "solved": solved,
           "summary": summary, "h2d_bytes": nb.value}
    if keep_problem:
        out["problem"] = []
        for stage in range(2):
            n_p, n_o = C.c_int32(), C.c_int32()
            ctx.check(lib().msfm_round_set_fetch_problem(h, stage, C.byref(n_p), C.byref(n_o), None, None, None, None, None, None, None))
            n_p, n_o = n_p.value, n_o.value
            kept, q_cam, q_pt = np.zeros(max(1, n_p), np.int32), np.zeros(max(1, n_o), np.int32), np.zeros(max(1, n_o), np.int32)
            q_xy, q_w = np.zeros((max(1, n_o), 2)), np.zeros(max(1, n_p))
            q_cm, q_pm = np.zeros(c1, np.uint8), np.zeros(max(1, n_p), np.uint8)
            ran = bool(partial) if stage == 0 else bool(full)
            if ran:
                ctx.check(lib().msfm_round_set_fetch_problem(h, stage, None, None, A.ptr(kept, ip), A.ptr(q_cam, ip), A.ptr(q_pt, ip), A.ptr(q_xy, dp),
                                                             A.ptr(q_w, dp), A.ptr(q_cm, up), A.ptr(q_pm, up)))
            out["problem"].append({"kept": kept[:n_p], "obs_cam": q_cam[:n_o], "obs_pt": q_pt[:n_o], "obs_xy": q_xy[:n_o], "pt_weight": q_w[:n_p],
                                   "cam_mutable": q_cm[:nc if ran else 0], "pt_mutable": q_pm[:n_p]})
    return out


class Context(_Handle):
    """One per GPU (one process per GPU)."""
    _destroy = "msfm_ctx_destroy"

    def __init__(self, device=-1):
        self._h = C.c_void_p()
        rc = lib().msfm_ctx_create(device, C.byref(self._h))
        if rc != 0:
            raise MsfmError(rc, "msfm_ctx_create failed (no visible GPU? libmsfm has no CPU fallback)")
        self._cb = None

    def check(self, rc):
        if rc != 0:
            raise MsfmError(rc, lib().msfm_last_error(self._h).decode())

    @property
    def stream(self):
        return lib().msfm_ctx_stream(self._h)

    def synchronize(self):
        self.check(lib().msfm_ctx_synchronize(self._h))

    # -- profiling --
    def profile(self, enable=True):
        self.check(lib().msfm_ctx_profile_enable(self._h, int(enable)))

    def profile_reset(self):
        self.check(lib().msfm_ctx_profile_reset(self._h))

    def profile_get(self):
        arr = (A.KernelStat * A.MSFM_MAX_KERNEL_STATS)()
        n = C.c_int()
        self.check(lib().msfm_ctx_profile_get(self._h, arr, A.MSFM_MAX_KERNEL_STATS, C.byref(n)))
        return {arr[k].name.decode(): dict(launches=int(arr[k].launches), total_ms=float(arr[k].total_ms))
                for k in range(n.value)}

    def set_allreduce(self, fn, rank, world_size):
        """fn(buf_ptr:int, count:int, op:int, stream_ptr:int) -> int (0 ok); op 0 = sum, 1 = max."""
        if fn is None:
            self._cb = ALLREDUCE_FN()
        else:
            def tramp(user, buf, count, op, stream):
                try:
                    return int(fn(buf, count, op, stream) or 0)
                except Exception:  # never let an exception cross the C boundary
                    import traceback
                    traceback.print_exc()
                    return -1
            self._cb = ALLREDUCE_FN(tramp)
        self.check(lib().msfm_ctx_set_allreduce(self._h, self._cb, None, rank, world_size))

    def rccl_unique_id(self):
        """128 opaque bytes (ncclUniqueId) from rank 0, to be handed to every rank's init_rccl."""
        buf = (C.c_ubyte * 128)()
        self.check(lib().msfm_rccl_get_unique_id(self._h, buf))
        return bytes(buf)

    def init_rccl(self, unique_id, rank, world_size):
        """Collective: the library creates its own RCCL communicator and reduces with ncclAllReduce on its stream -
        no Python in the LM loop (msfm_ctx_init_rccl)."""
        buf = (C.c_ubyte * 128).from_buffer_copy(unique_id)
        self.check(lib().msfm_ctx_init_rccl(self._h, buf, rank, world_size))

    def allreduce(self, dev_ptr, count, op=0):
        """msfm_ctx_allreduce on a device buffer of doubles (op 0 = sum, 1 = max), ordered on the context's stream."""
        self.check(lib().msfm_ctx_allreduce(self._h, C.cast(dev_ptr, A.c_double_p), count, op))

    # -- matching --
    def knn2(self, train, query):
        """fine_matching_graph.cc:99 shaped call: returns ids [nq,2] i32, sqdists [nq,2] f32."""
        train, query = A.as_c(train, np.float32), A.as_c(query, np.float32)
        if train.ndim != 2 or query.ndim != 2 or train.shape[1] != query.shape[1]:
            raise ValueError("train/query must be [n, dim] with equal dim")
        ids = np.zeros((len(query), 2), dtype=np.int32)
        d = np.zeros((len(query), 2), dtype=np.float32)
        self.check(lib().msfm_knn2_f32(self._h, A.ptr(train, A.c_float_p), len(train), A.ptr(query, A.c_float_p),
                                       len(query), train.shape[1], A.ptr(ids, A.c_int_p), A.ptr(d, A.c_float_p)))
        return ids, d

    def descset(self, descs, keypoints=None):
        return DescSet(self, descs, keypoints)

    # -- bundle adjustment --
    def ba_solve(self, arrays: A.BaArrays, options=None, capacity=512):
        """msfm_ba_solve: optimises `arrays` IN PLACE; returns the summary dict."""
        options = options or default_options()
        buf = A.SummaryBuf(capacity)
        self.check(lib().msfm_ba_solve(self._h, C.byref(arrays.struct), C.byref(options), C.byref(buf.struct)))
        return buf.result()

    def ba(self, arrays: A.BaArrays):
        return BaResident(self, arrays)

    # -- triangulation --
    def _tri(self, fn, tracks, th_error, th_angle, X0):
        n = tracks.struct.n_tracks
        X = np.zeros((n, 3)) if X0 is None else np.array(X0, dtype=np.float64, order="C")
        mse, ok = np.zeros(n), np.zeros(n, dtype=np.uint8)
        self.check(fn(self._h, C.byref(tracks.struct), th_error, th_angle, A.ptr(X, A.c_double_p),
                      A.ptr(mse, A.c_double_p), A.ptr(ok, A.c_u8_p)))
        return X, mse, ok

    def build_tracks(self, n_features, pairs, matches_per_pair, flat=None):
        """`build_tracks` on the GPU (msfm_tracks_build_device): identical output.  `flat` = (n_features, pairs [p][2],
        match_off [p+1], matches [m][2]) int32 arrays skips the per-pair Python lists."""
        nf, pr, off, fl = flat if flat is not None else _flatten_matches(n_features, pairs, matches_per_pair)
        h = C.c_void_p()
        self.check(lib().msfm_tracks_build_device(self._h, len(nf), A.ptr(nf, A.c_int_p), len(pr), A.ptr(pr, A.c_int_p),
                                                  A.ptr(off, A.c_int_p), A.ptr(fl, A.c_int_p), C.byref(h)))
        return _fetch_track_set(h)

    def match_store(self, n_features, pairs, match_off, matches):
        """msfm_match_store_create: the verified matches resident on the device (pairs [P][2] strictly ascending in (idx1, idx2),
        match_off [P+1], matches [M][2]: the flat layout of `build_tracks`)."""
        return MatchStore(self, n_features, pairs, match_off, matches)

    def wordset(self, n_features, words, num_words, keypoints, max_hypotheses=0):
        """msfm_wordset_create: word tables, similarity matrix and ranked hypotheses of an image set, resident as a `Wordset`.
        words: per image the word id of every feature, or None / empty for an image without words (`<i>_words` empty)."""
        return Wordset(self, n_features, words, num_words, keypoints, max_hypotheses)

    def voctree(self, k, block_n, node_desc, node_link, node_weight):
        """msfm_voctree_create: a vocabulary tree (featurefiles.read_voctree) resident as a `VocTree`."""
        return VocTree(self, k, block_n, node_desc, node_link, node_weight)

    def scalespace(self, gray, n_octaves=4, n_levels=5, stride=None):
        """msfm_scalespace_create: the Gaussian scale space and gradients of a uint8 image [h][w] resident as a `ScaleSpace`;
        stride (>= w) hands the image over in a buffer of that many bytes per row."""
        return ScaleSpace(self, gray, n_octaves, n_levels, stride)

    def stereo_sgm(self, width, height, disp_size=128, p1=10, p2=120, uniqueness=0.96):
        """msfm_sgm_create: a dense-stereo object for rectified uint8 pairs of width x height, resident as a `StereoSGM` and reused
        pair after pair; the defaults are the reference's call."""
        return StereoSGM(self, width, height, disp_size, p1, p2, uniqueness)

    def rectifier(self, width, height):
        """msfm_rectifier_create: a stereo rectifier for posed uint8 pairs of width x height, resident as a `Rectifier` and reused
        pair after pair; `StereoSGM.execute_rectified` reads its planes on the device."""
        return Rectifier(self, width, height)

    def recon(self, store, state, cam_pose, cam_model, cam_model_of_cam, keypoints=None, reserve_points=0, reserve_obs=0, *, model_mutable=None):
        """msfm_recon_create: the flat state `newpoints.py` documents, with its point side and pt_new_added, resident on the device
        as a `Recon`; cam_pose / cam_model / cam_model_of_cam are the solver's parameter blocks as `adjust.adjust_round` takes
        them.  keypoints: every image's rows, for a store that was not made from a chain.  Close it before its store."""
        return Recon(self, store, state, cam_pose, cam_model, cam_model_of_cam, keypoints, model_mutable, reserve_points, reserve_obs)

    def localize_set(self, store, cam_img, feat_point, pt_bad, pt_mse, pt_views, cand_img, fail_times, point_xyz=None, keypoints=None):
        """msfm_localize_candidates, the result kept as a `LocalizeSet`: `fetch()` is the dict of `localize_candidates`, and with
        point_xyz the correspondences stay on the device for `poses(...)` (msfm_localize_poses).  Close it before the context."""
        cam_img, feat_point, pt_views, cand_img, fail_times = (A.as_c(np.asarray(x, dtype=np.int32), np.int32)
                                                               for x in (cam_img, feat_point, pt_views, cand_img, fail_times))
        pt_bad = A.as_c(np.asarray(pt_bad, dtype=np.uint8), np.uint8)
        pt_mse = A.as_c(np.asarray(pt_mse, dtype=np.float64), np.float64)
        if not (len(pt_bad) == len(pt_mse) == len(pt_views)) or len(cand_img) != len(fail_times):
            raise ValueError("pt_bad / pt_mse / pt_views and cand_img / fail_times must have equal lengths")
        in_store = (cam_img >= 0) & (cam_img < len(store.n_features))     # (an image outside the store: the library reports it)
        if in_store.all() and len(feat_point) != int(store.n_features[cam_img].sum()):
            raise ValueError("feat_point must hold one entry per feature of every registered image")
        xyz = None if point_xyz is None else A.as_c(np.asarray(point_xyz, dtype=np.float64).reshape(-1, 3), np.float64)
        if xyz is not None and len(xyz) != len(pt_bad):
            raise ValueError("point_xyz must hold one row per point")
        kp = None if keypoints is None else A.as_c(np.asarray(keypoints, dtype=np.float32).reshape(-1, 2), np.float32)
        if kp is not None and len(kp) != int(store.n_features.sum()):
            raise ValueError("keypoints must hold one row per feature of every image")
        P = A.LocalizeProblem(len(cam_img), A.ptr(cam_img, A.c_int_p), A.ptr(feat_point, A.c_int_p), len(pt_bad), A.ptr(pt_bad, A.c_u8_p),
                              A.ptr(pt_mse, A.c_double_p), A.ptr(pt_views, A.c_int_p), len(cand_img), A.ptr(cand_img, A.c_int_p),
                              A.ptr(fail_times, A.c_int_p), A.ptr(xyz, A.c_double_p), A.ptr(kp, A.c_float_p))
        h = C.c_void_p()
        self.check(lib().msfm_localize_candidates(self._h, store._h, C.byref(P), C.byref(h)))
        return LocalizeSet(self, h)

    def localize_candidates(self, store, cam_img, feat_point, pt_bad, pt_mse, pt_views, cand_img, fail_times, point_xyz=None, keypoints=None):
        """msfm_localize_candidates (sfm_incremental.cc:440-562): the 2D-3D correspondences and visible cameras of every candidate
        image, ranked.  Returns a dict: rank [n_kept] (indices into cand_img), corr_off, corr_feat, corr_point, vis_off, vis_cam,
        h2d_bytes and, with point_xyz, pts_w [n_corr][3] / pts_2d [n_corr][2] (offsets = corr_off for `epnp_ransac`).
        keypoints: flat float [sum of n_features][2] for a store that was not made from a chain."""
        with self.localize_set(store, cam_img, feat_point, pt_bad, pt_mse, pt_views, cand_img, fail_times, point_xyz=point_xyz,
                               keypoints=keypoints) as st:
            return st.fetch()

    def seed_hypotheses(self, store, hyp_img, cam_fk, same_model, keypoints=None, keep=False, **opts):
        """msfm_seed_hypotheses (sfm_incremental.cc:235-390): pose, two-view points and the two gates of every seed-pair
        hypothesis, on the resident store.  hyp_img [n][2], cam_fk [n][2][3] (f with 0 = unknown, k1, k2), same_model [n];
        opts: fields of msfm_seed_options.  Returns a dict: arm, pose_ok, pass, n_matches, f [n][2], R [n][3][3], t, c [n][3],
        pt_off [n+1], pt_match, X [..][3], mse, winner (-1: none), h2d_bytes.  keep=True: the dict also holds the live `SeedSet`
        under "set", whose winner's points stay on the device for `Recon.from_seed`; close it before the context."""
        hyp = A.as_c(np.asarray(hyp_img, dtype=np.int32).reshape(-1, 2), np.int32)
        n = len(hyp)
        fk = A.as_c(np.asarray(cam_fk, dtype=np.float64).reshape(-1, 2, 3), np.float64)
        same = A.as_c(np.asarray(same_model, dtype=np.uint8).reshape(-1), np.uint8)
        if len(fk) != n or len(same) != n:
            raise ValueError("hyp_img, cam_fk and same_model must describe the same number of hypotheses")
        kp = None if keypoints is None else A.as_c(np.asarray(keypoints, dtype=np.float32).reshape(-1, 2), np.float32)
        if kp is not None and len(kp) != int(store.n_features.sum()):
            raise ValueError("keypoints must hold one row per feature of every image")
        P = A.SeedProblem(n, A.ptr(hyp, A.c_int_p), A.ptr(fk, A.c_double_p), A.ptr(same, A.c_u8_p), A.ptr(kp, A.c_float_p))
        o = seed_options(**opts)
        h = C.c_void_p()
        self.check(lib().msfm_seed_hypotheses(self._h, store._h, C.byref(P), C.byref(o), C.byref(h)))
        st = SeedSet(self, store, h)
        try:
            nh, npt, win, nb = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
            lib().msfm_seed_set_size(h, C.byref(nh), C.byref(npt), C.byref(win), C.byref(nb))
            npt, m = npt.value, max(1, n)
            arm, pok, pas = (np.zeros(m, np.uint8) for _ in range(3))
            nm, poff, ptm = np.zeros(m, np.int32), np.zeros(n + 1, np.int32), np.zeros(max(1, npt), np.int32)
            f, R, t, c = np.zeros((m, 2)), np.zeros((m, 3, 3)), np.zeros((m, 3)), np.zeros((m, 3))
            X, mse = np.zeros((max(1, npt), 3)), np.zeros(max(1, npt))
            dp = A.c_double_p
            lib().msfm_seed_set_fetch(h, A.ptr(arm, A.c_u8_p), A.ptr(pok, A.c_u8_p), A.ptr(pas, A.c_u8_p), A.ptr(nm, A.c_int_p), A.ptr(f, dp),
                                      A.ptr(R, dp), A.ptr(t, dp), A.ptr(c, dp), A.ptr(poff, A.c_int_p), A.ptr(ptm, A.c_int_p), A.ptr(X, dp),
                                      A.ptr(mse, dp))
        finally:
            if not keep:
                st.close()
        out = {"arm": arm[:n], "pose_ok": pok[:n], "pass": pas[:n], "n_matches": nm[:n], "f": f[:n], "R": R[:n], "t": t[:n], "c": c[:n],
               "pt_off": poff, "pt_match": ptm[:npt], "X": X[:npt], "mse": mse[:npt], "winner": win.value, "h2d_bytes": nb.value}
        if keep:
            out["set"] = st
        return out

    def new_points(self, store, cam_img, feat_point, n_points, cam_R, cam_t, cam_c, cam_fk, new_cam, vis_off, vis_cam, keypoints=None, **opts):
        """msfm_new_points (sfm_incremental.cc:755-915): the new two-view points of every new camera against its visible cameras,
        on the resident store.  cam_img [n_cams], feat_point (flat, one entry per feature of every camera's image, -1 = no
        point), cam_R [n][3][3], cam_t / cam_c / cam_fk [n][3], new_cam [n_new], vis_off [n_new+1], vis_cam; opts: fields of
        msfm_new_points_options.  Returns a dict: pt_off [n_new+1]; per point cam2, feat1, feat2, vis_entry, pt_match, X [..][3],
        mse, takes1, takes2; per visible entry n_matches, large, n_candidates, n_accepted; h2d_bytes."""
        cam_img, feat_point, new_cam, vis_off, vis_cam = (A.as_c(np.asarray(x, dtype=np.int32).reshape(-1), np.int32)
                                                          for x in (cam_img, feat_point, new_cam, vis_off, vis_cam))
        nc, nn = len(cam_img), len(new_cam)
        R = A.as_c(np.asarray(cam_R, dtype=np.float64).reshape(-1, 9), np.float64)
        t, c, fk = (A.as_c(np.asarray(x, dtype=np.float64).reshape(-1, 3), np.float64) for x in (cam_t, cam_c, cam_fk))
        if not (len(R) == len(t) == len(c) == len(fk) == nc):
            raise ValueError("cam_img, cam_R, cam_t, cam_c and cam_fk must describe the same number of cameras")
        if len(vis_off) != nn + 1:
            raise ValueError("vis_off must hold n_new + 1 offsets")
        if nn and 0 <= vis_off[-1] and len(vis_cam) != vis_off[-1]:
            raise ValueError("vis_cam must hold vis_off[n_new] entries")
        in_store = (cam_img >= 0) & (cam_img < len(store.n_features))     # (an image outside the store: the library reports it)
        if in_store.all() and len(feat_point) != int(store.n_features[cam_img].sum()):
            raise ValueError("feat_point must hold one entry per feature of every camera's image")
        kp = None if keypoints is None else A.as_c(np.asarray(keypoints, dtype=np.float32).reshape(-1, 2), np.float32)
        if kp is not None and len(kp) != int(store.n_features.sum()):
            raise ValueError("keypoints must hold one row per feature of every image")
        dp, ip, up = A.c_double_p, A.c_int_p, A.c_u8_p
        P = A.NewPointsProblem(nc, A.ptr(cam_img, ip), A.ptr(feat_point, ip), int(n_points), A.ptr(R, dp), A.ptr(t, dp), A.ptr(c, dp),
                               A.ptr(fk, dp), nn, A.ptr(new_cam, ip), A.ptr(vis_off, ip), A.ptr(vis_cam, ip), A.ptr(kp, A.c_float_p))
        o = new_points_options(**opts)
        h = C.c_void_p()
        self.check(lib().msfm_new_points(self._h, store._h, C.byref(P), C.byref(o), C.byref(h)))
        with _Handle(h, "msfm_new_points_set_destroy"):
            return _new_points_set_result(h, nn)

    def round_adjust(self, store, cam_img, feat_point, obs_point, obs_cam, obs_feat, cam_pose, cam_model, cam_model_of_cam, point_xyz, pt_bad,
                     pt_mse, pt_mutable, pt_new_added=None, new_cam=-1, visible=(), partial=True, full=False, outliers=True, model_mutable=None,
                     keypoints=None, capacity=512, **opts):
        """msfm_round_adjust (sfm_incremental.cc:172-186): PartialBundleAdjustment(new_cam), FullBundleAdjustment and
        RemovePointOutliers - the stages `partial` / `full` / `outliers` switch on, in that order - on the flat state with both of
        its sides: feat_point (Camera::pts_) and the rows obs_point / obs_cam / obs_feat (Point3D::cams_).  opts: fields of
        msfm_round_options (`partial_options` / `full_options`: dicts of msfm_ba_options fields).  Returns a dict: cam_pose,
        cam_model, cam_R [n][3][3], cam_t, cam_c, cam_fk, point_xyz, pt_mutable, pt_bad, pt_mse, pt_new_added, pt_views,
        count_outliers, count_new_add, count_outliers_new_add, adjust_cams / adjust_pts [2], solved [2], summary (a list of two:
        the summary dict of `ba_solve`, or None for a stage that did not solve), h2d_bytes and, with keep_problem=1, problem (a
        list of two dicts: kept, obs_cam, obs_pt, obs_xy, pt_weight, cam_mutable, pt_mutable)."""
        ip, dp, up = A.c_int_p, A.c_double_p, A.c_u8_p
        cam_img, feat_point, obs_point, obs_cam, obs_feat, mcam, visible = (A.as_c(np.asarray(x, dtype=np.int32).reshape(-1), np.int32) for x in (
            cam_img, feat_point, obs_point, obs_cam, obs_feat, cam_model_of_cam, visible))
        nc, no = len(cam_img), len(obs_point)
        pose = A.as_c(np.asarray(cam_pose, dtype=np.float64).reshape(-1, 6), np.float64)
        model = A.as_c(np.asarray(cam_model, dtype=np.float64).reshape(-1, 3), np.float64)
        xyz = A.as_c(np.asarray(point_xyz, dtype=np.float64).reshape(-1, 3), np.float64)
        mse = A.as_c(np.asarray(pt_mse, dtype=np.float64).reshape(-1), np.float64)
        bad, mut = (A.as_c(np.asarray(x, dtype=np.uint8).reshape(-1), np.uint8) for x in (pt_bad, pt_mutable))
        added = None if pt_new_added is None else A.as_c(np.asarray(pt_new_added, dtype=np.uint8).reshape(-1), np.uint8)
        mm = None if model_mutable is None else A.as_c(np.asarray(model_mutable, dtype=np.uint8).reshape(-1), np.uint8)
        npt, nm = len(xyz), len(model)
        if not (len(pose) == len(mcam) == nc):
            raise ValueError("cam_img, cam_pose and cam_model_of_cam must describe the same number of cameras")
        if not (len(obs_cam) == len(obs_feat) == no):
            raise ValueError("obs_point, obs_cam and obs_feat must hold one entry per observation")
        if not (len(mse) == len(bad) == len(mut) == npt) or (added is not None and len(added) != npt):
            raise ValueError("point_xyz, pt_bad, pt_mse, pt_mutable and pt_new_added must hold one entry per point")
        if mm is not None and len(mm) != nm:
            raise ValueError("model_mutable must hold one entry per model")
        in_store = (cam_img >= 0) & (cam_img < len(store.n_features))     # (an image outside the store: the library reports it)
        if in_store.all() and len(feat_point) != int(store.n_features[cam_img].sum()):
            raise ValueError("feat_point must hold one entry per feature of every camera's image")
        kp = None if keypoints is None else A.as_c(np.asarray(keypoints, dtype=np.float32).reshape(-1, 2), np.float32)
        if kp is not None and len(kp) != int(store.n_features.sum()):
            raise ValueError("keypoints must hold one row per feature of every image")
        P = A.RoundProblem(nc, A.ptr(cam_img, ip), A.ptr(feat_point, ip), npt, A.ptr(kp, A.c_float_p), no, A.ptr(obs_point, ip), A.ptr(obs_cam, ip),
                           A.ptr(obs_feat, ip), A.ptr(pose, dp), nm, A.ptr(model, dp), A.ptr(mcam, ip), A.ptr(mm, up), A.ptr(xyz, dp), A.ptr(bad, up),
                           A.ptr(mse, dp), A.ptr(mut, up), A.ptr(added, up), int(new_cam), len(visible), A.ptr(visible, ip), int(bool(partial)),
                           int(bool(full)), int(bool(outliers)))
        opts = dict(opts)
        for k in ("partial", "full"):
            if k + "_options" in opts:
                opts[k] = opts.pop(k + "_options")
        o = round_options(**opts)
        h = C.c_void_p()
        self.check(lib().msfm_round_adjust(self._h, store._h, C.byref(P), C.byref(o), C.byref(h)))
        with _Handle(h, "msfm_round_set_destroy"):
            return _round_set_result(self, h, nc, nm, npt, partial, full, o.keep_problem, capacity)

    def triangulate_midpoint(self, tracks, th_error, th_angle, X0=None):
        return self._tri(lib().msfm_triangulate_midpoint_batch, tracks, th_error, th_angle, X0)

    def triangulate_dlt(self, tracks, th_error, th_angle, X0=None):
        return self._tri(lib().msfm_triangulate_dlt_batch, tracks, th_error, th_angle, X0)

    def reproject_mse(self, tracks, X):
        X = A.as_c(X, np.float64)
        mse = np.zeros(tracks.struct.n_tracks)
        self.check(lib().msfm_reproject_mse_batch(self._h, C.byref(tracks.struct), A.ptr(X, A.c_double_p),
                                                  A.ptr(mse, A.c_double_p)))
        return mse

    def point_accuracy(self, tracks, X, ok_in, cam_dc=None, min_views=3, th_outlier=3.0):
        """msfm_point_accuracy_batch (GetAccuracy, slam_gps.cc:1573-1594): e_avg, e_mse, n_used, ok_out, n_outliers, n_inliers."""
        n = tracks.struct.n_tracks
        X, ok_in, dc = A.as_c(X, np.float64), A.as_c(ok_in, np.uint8), A.as_c(cam_dc, np.float64)
        e_avg, e_mse, n_used, ok = np.zeros(n), np.zeros(n), np.zeros(n, np.int32), np.zeros(n, np.uint8)
        n_out, n_in = C.c_int32(), C.c_int32()
        self.check(lib().msfm_point_accuracy_batch(self._h, C.byref(tracks.struct), A.ptr(dc, A.c_double_p), A.ptr(X, A.c_double_p),
                                                   A.ptr(ok_in, A.c_u8_p), min_views, th_outlier, A.ptr(e_avg, A.c_double_p),
                                                   A.ptr(e_mse, A.c_double_p), A.ptr(n_used, A.c_int_p), A.ptr(ok, A.c_u8_p),
                                                   C.byref(n_out), C.byref(n_in)))
        return e_avg, e_mse, n_used, ok, n_out.value, n_in.value

    def gps_register_points(self, track_off, track_cam, ok, cam_c, gps, X):
        """msfm_gps_register_points (the point loop of GPSRegistration2, slam_gps.cc:933-978): the shifted copy of X."""
        off, cam, ok = A.as_c(track_off, np.int32), A.as_c(track_cam, np.int32), A.as_c(ok, np.uint8)
        c, g = A.as_c(np.asarray(cam_c, dtype=np.float64).reshape(-1, 3), np.float64), A.as_c(np.asarray(gps, dtype=np.float64).reshape(-1, 3), np.float64)
        X = np.array(X, dtype=np.float64, order="C")
        self.check(lib().msfm_gps_register_points(self._h, len(off) - 1, A.ptr(off, A.c_int_p), A.ptr(cam, A.c_int_p), A.ptr(ok, A.c_u8_p), len(c),
                                                  A.ptr(c, A.c_double_p), A.ptr(g, A.c_double_p), A.ptr(X, A.c_double_p)))
        return X

    def epipolar_filter(self, pt1, pt2, F, th=3.0):
        pt1, pt2 = A.as_c(pt1, np.float32), A.as_c(pt2, np.float32)
        F = A.as_c(np.asarray(F, dtype=np.float64).reshape(9), np.float64)
        out = np.zeros(len(pt1), dtype=np.uint8)
        self.check(lib().msfm_epipolar_filter(self._h, A.ptr(pt1, A.c_float_p), A.ptr(pt2, A.c_float_p), len(pt1),
                                              A.ptr(F, A.c_double_p), th, A.ptr(out, A.c_u8_p)))
        return out

    def fundamental_ransac(self, offsets, pt1, pt2, **opts):
        """GeoVerification::GeoVerificationFundamental for a batch of pairs (geo_verification.cc:30-58).
        offsets[n_pairs+1] delimit each pair's matches in pt1/pt2 (float32 [total][2]).
        Returns F [n_pairs][3][3], inlier mask [total], n_inliers [n_pairs], ok [n_pairs]."""
        offsets = A.as_c(offsets, np.int32)
        pt1, pt2 = A.as_c(np.asarray(pt1, dtype=np.float32).reshape(-1, 2), np.float32), A.as_c(np.asarray(pt2, dtype=np.float32).reshape(-1, 2), np.float32)
        n_pairs = len(offsets) - 1
        o = fransac_options(**opts)
        F = np.zeros((n_pairs, 3, 3), dtype=np.float64)
        inl = np.zeros(max(1, len(pt1)), dtype=np.uint8)
        nin = np.zeros(max(1, n_pairs), dtype=np.int32)
        ok = np.zeros(max(1, n_pairs), dtype=np.uint8)
        self.check(lib().msfm_fundamental_ransac_batch(self._h, n_pairs, A.ptr(offsets, A.c_int_p), A.ptr(pt1, A.c_float_p),
                                                       A.ptr(pt2, A.c_float_p), C.byref(o), A.ptr(F, A.c_double_p),
                                                       A.ptr(inl, A.c_u8_p), A.ptr(nin, A.c_int_p), A.ptr(ok, A.c_u8_p)))
        return F, inl[:len(pt1)], nin[:n_pairs], ok[:n_pairs]

    def homography_ransac(self, offsets, pt1, pt2, **opts):
        """cv::findHomography(pt1, pt2, mask, RANSAC, threshold) for a batch of pairs (slam_gps.cc:402).
        offsets[n_pairs+1] delimit each pair's correspondences in pt1/pt2 (float32 [total][2]).
        Returns H [n_pairs][3][3] (H[2,2] = 1, zeros when no model), inlier mask [total], n_inliers [n_pairs], ok [n_pairs]."""
        offsets = A.as_c(offsets, np.int32)
        pt1 = A.as_c(np.asarray(pt1, dtype=np.float32).reshape(-1, 2), np.float32)
        pt2 = A.as_c(np.asarray(pt2, dtype=np.float32).reshape(-1, 2), np.float32)
        n_pairs = len(offsets) - 1
        o = hransac_options(**opts)
        H = np.zeros((max(1, n_pairs), 3, 3), dtype=np.float64)
        inl = np.zeros(max(1, len(pt1)), dtype=np.uint8)
        nin = np.zeros(max(1, n_pairs), dtype=np.int32)
        ok = np.zeros(max(1, n_pairs), dtype=np.uint8)
        self.check(lib().msfm_homography_ransac_batch(self._h, n_pairs, A.ptr(offsets, A.c_int_p), A.ptr(pt1, A.c_float_p),
                                                      A.ptr(pt2, A.c_float_p), C.byref(o), A.ptr(H, A.c_double_p),
                                                      A.ptr(inl, A.c_u8_p), A.ptr(nin, A.c_int_p), A.ptr(ok, A.c_u8_p)))
        return H[:n_pairs], inl[:len(pt1)], nin[:n_pairs], ok[:n_pairs]

    def slam_priors(self, n_cams, track_off, track_cam, track_xy, **opts):
        """SLAMGPS::FeatureMatching step 1 (slam_gps.cc:323-423): the SLAM points as CSR tracks (track_off [n+1], track_cam,
        track_xy [obs][2]) of n_cams cameras.  Returns (pairs [k][2], F [k][3][3], H [k][3][3], candidates [slots][6] =
        i, j, n_shared, n_inliers_f, n_inliers_h, verdict) - pairs / F / H are what match_pairs_slam takes."""
        o = slam_prior_options(**opts)
        toff = A.as_c(np.asarray(track_off, dtype=np.int32), np.int32)
        tcam = A.as_c(np.asarray(track_cam, dtype=np.int32).reshape(-1), np.int32)
        txy = A.as_c(np.asarray(track_xy, dtype=np.float64).reshape(-1, 2), np.float64)
        t = A.Tracks()
        t.n_tracks, t.n_cams = len(toff) - 1, int(n_cams)
        t.track_off, t.track_cam, t.track_xy = A.ptr(toff, A.c_int_p), A.ptr(tcam, A.c_int_p), A.ptr(txy, A.c_double_p)
        cap = max(1, int(n_cams) * (2 * max(1, o.win_size) - 1))
        pairs = np.zeros((cap, 2), dtype=np.int32)
        F = np.zeros((cap, 3, 3)); H = np.zeros((cap, 3, 3))
        cand = np.zeros((cap, 6), dtype=np.int32)
        n, nc = C.c_int(0), C.c_int(0)
        self.check(lib().msfm_slam_priors(self._h, C.byref(t), C.byref(o), C.byref(n), A.ptr(pairs, A.c_int_p), A.ptr(F, A.c_double_p),
                                          A.ptr(H, A.c_double_p), C.byref(nc), A.ptr(cand, A.c_int_p)))
        k = n.value
        return pairs[:k], F[:k], H[:k], cand[:nc.value]

    def epnp_ransac(self, offsets, pts_w, pts_2d, f, max_iter=200, seed=0x4D53464D50):
        """AbsolutePoseEstimation::AbsolutePoseWithFocalLength for a batch of images (absolute_pose_estimation.cc:42-58):
        EPnP RANSAC over 4-point samples + the reprojection errors of all correspondences.
        Returns R [n][3][3], t [n][3], errors [total], avg_error [n], best_iter [n]."""
        offsets = A.as_c(offsets, np.int32)
        pts_w = A.as_c(np.asarray(pts_w, dtype=np.float64).reshape(-1, 3), np.float64)
        pts_2d = A.as_c(np.asarray(pts_2d, dtype=np.float64).reshape(-1, 2), np.float64)
        n = len(offsets) - 1
        f = A.as_c(np.broadcast_to(np.asarray(f, dtype=np.float64), (n,)).copy(), np.float64)
        R = np.zeros((max(1, n), 3, 3)); t = np.zeros((max(1, n), 3)); err = np.zeros(max(1, len(pts_w))); avg = np.zeros(max(1, n))
        best = np.zeros(max(1, n), dtype=np.int32)
        self.check(lib().msfm_epnp_ransac_batch(self._h, n, A.ptr(offsets, A.c_int_p), A.ptr(pts_w, A.c_double_p), A.ptr(pts_2d, A.c_double_p),
                                                A.ptr(f, A.c_double_p), max_iter, seed, A.ptr(R, A.c_double_p), A.ptr(t, A.c_double_p),
                                                A.ptr(err, A.c_double_p), A.ptr(avg, A.c_double_p), A.ptr(best, A.c_int_p)))
        return R[:n], t[:n], err[:len(pts_w)], avg[:n], best[:n]

    def epnpf_sweep(self, offsets, pts_w, pts_2d, f_init, f_ratio_min=0.5, f_ratio_max=4.0, f_ratio_step=0.01, max_iter=200,
                    seed=0x4D53464D50, keep_step_errors=False):
        """AbsolutePoseEstimation::AbsolutePoseWithoutFocalLength for a batch of images (absolute_pose_estimation.cc:28-40):
        the EPNPF focal sweep (absolute_pose_via_epnpf.cc:34-63) - an EPnP RANSAC at every candidate
        (f_ratio_min + i * f_ratio_step) * f_init - + the reprojection errors of all correspondences at the kept candidate.
        Returns f [n], R [n][3][3], t [n][3], errors [total], avg_error [n], best_step [n], best_iter [n]
        [, step_error [n][n_steps] with keep_step_errors]."""
        offsets = A.as_c(offsets, np.int32)
        pts_w = A.as_c(np.asarray(pts_w, dtype=np.float64).reshape(-1, 3), np.float64)
        pts_2d = A.as_c(np.asarray(pts_2d, dtype=np.float64).reshape(-1, 2), np.float64)
        n = len(offsets) - 1
        f_init = A.as_c(np.broadcast_to(np.asarray(f_init, dtype=np.float64), (n,)).copy(), np.float64)
        o = A.EpnpfOptions(f_ratio_min, f_ratio_max, f_ratio_step, max_iter, seed)
        n_steps = lib().msfm_epnpf_num_steps(C.byref(o))
        f = np.zeros(max(1, n)); R = np.zeros((max(1, n), 3, 3)); t = np.zeros((max(1, n), 3)); err = np.zeros(max(1, len(pts_w)))
        avg = np.zeros(max(1, n)); bstep = np.zeros(max(1, n), dtype=np.int32); biter = np.zeros(max(1, n), dtype=np.int32)
        # invalid options: the call below reports them (no step array is touched before its checks)
        serr = np.zeros((max(1, n), max(1, n_steps))) if keep_step_errors else None
        self.check(lib().msfm_epnpf_sweep_batch(self._h, n, A.ptr(offsets, A.c_int_p), A.ptr(pts_w, A.c_double_p), A.ptr(pts_2d, A.c_double_p),
                                                A.ptr(f_init, A.c_double_p), C.byref(o), A.ptr(f, A.c_double_p), A.ptr(R, A.c_double_p),
                                                A.ptr(t, A.c_double_p), A.ptr(err, A.c_double_p), A.ptr(avg, A.c_double_p),
                                                A.ptr(bstep, A.c_int_p), A.ptr(biter, A.c_int_p), A.ptr(serr, A.c_double_p)))
        out = (f[:n], R[:n], t[:n], err[:len(pts_w)], avg[:n], bstep[:n], biter[:n])
        return out + (serr[:n],) if keep_step_errors else out

    def relpose_5pt(self, offsets, pts_ref, pts_cur, f_ref, f_cur, ransac_times=100, seed=0x4D53464D45):
        """RelativePoseEstimation::RelativePoseWithFocalLength for a batch of image pairs (relative_pose_estimation.cc:91-120):
        five-point RANSAC + decomposition of the best essential matrix.
        Returns E [n][3][3], R [n][3][3], t [n][3], ok [n], n_candidates [n]."""
        offsets = A.as_c(offsets, np.int32)
        pts_ref = A.as_c(np.asarray(pts_ref, dtype=np.float64).reshape(-1, 2), np.float64)
        pts_cur = A.as_c(np.asarray(pts_cur, dtype=np.float64).reshape(-1, 2), np.float64)
        n = len(offsets) - 1
        f_ref = A.as_c(np.broadcast_to(np.asarray(f_ref, dtype=np.float64), (n,)).copy(), np.float64)
        f_cur = A.as_c(np.broadcast_to(np.asarray(f_cur, dtype=np.float64), (n,)).copy(), np.float64)
        E = np.zeros((max(1, n), 3, 3)); R = np.zeros((max(1, n), 3, 3)); t = np.zeros((max(1, n), 3))
        ok = np.zeros(max(1, n), dtype=np.uint8); nc = np.zeros(max(1, n), dtype=np.int32)
        self.check(lib().msfm_relpose_5pt_batch(self._h, n, A.ptr(offsets, A.c_int_p), A.ptr(pts_ref, A.c_double_p), A.ptr(pts_cur, A.c_double_p),
                                                A.ptr(f_ref, A.c_double_p), A.ptr(f_cur, A.c_double_p), ransac_times, seed,
                                                A.ptr(E, A.c_double_p), A.ptr(R, A.c_double_p), A.ptr(t, A.c_double_p), A.ptr(ok, A.c_u8_p),
                                                A.ptr(nc, A.c_int_p)))
        return E[:n], R[:n], t[:n], ok[:n], nc[:n]

    def relpose_8pt(self, offsets, pts_ref, pts_cur, ransac_times=200, seed=0x4D53464D38, diagnostics=True):
        """RelativePoseEstimation::RelativePoseWithoutFocalLength for a batch of image pairs (relative_pose_estimation.cc:29-83):
        normalised eight-point F RANSAC on centred pixels, both focal lengths from F, E, and the decomposition of E.
        Returns F [n][3][3], f_ref [n], f_cur [n], E [n][3][3], R [n][3][3], t [n][3], ok [n], best_iter [n], best_error [n],
        n_candidates [n]; the last three are None with diagnostics=False (the library is then handed NULL for them)."""
        offsets = A.as_c(offsets, np.int32)
        pts_ref = A.as_c(np.asarray(pts_ref, dtype=np.float64).reshape(-1, 2), np.float64)
        pts_cur = A.as_c(np.asarray(pts_cur, dtype=np.float64).reshape(-1, 2), np.float64)
        n = len(offsets) - 1
        m = max(1, n)
        F = np.zeros((m, 3, 3)); E = np.zeros((m, 3, 3)); R = np.zeros((m, 3, 3)); t = np.zeros((m, 3))
        f1 = np.zeros(m); f2 = np.zeros(m); ok = np.zeros(m, dtype=np.uint8)
        bi = np.zeros(m, dtype=np.int32) if diagnostics else None
        be = np.zeros(m) if diagnostics else None
        nc = np.zeros(m, dtype=np.int32) if diagnostics else None
        self.check(lib().msfm_relpose_8pt_batch(self._h, n, A.ptr(offsets, A.c_int_p), A.ptr(pts_ref, A.c_double_p), A.ptr(pts_cur, A.c_double_p),
                                                ransac_times, seed, A.ptr(F, A.c_double_p), A.ptr(f1, A.c_double_p), A.ptr(f2, A.c_double_p),
                                                A.ptr(E, A.c_double_p), A.ptr(R, A.c_double_p), A.ptr(t, A.c_double_p), A.ptr(ok, A.c_u8_p),
                                                A.ptr(bi, A.c_int_p), A.ptr(be, A.c_double_p), A.ptr(nc, A.c_int_p)))
        out = (F[:n], f1[:n], f2[:n], E[:n], R[:n], t[:n], ok[:n])
        return out + ((bi[:n], be[:n], nc[:n]) if diagnostics else (None, None, None))

    def epipolar_filter_batch(self, offsets, pt1, pt2, F, ok=None, th=3.0):
        offsets = A.as_c(offsets, np.int32)
        pt1, pt2 = A.as_c(np.asarray(pt1, dtype=np.float32).reshape(-1, 2), np.float32), A.as_c(np.asarray(pt2, dtype=np.float32).reshape(-1, 2), np.float32)
        F = A.as_c(np.asarray(F, dtype=np.float64).reshape(-1, 9), np.float64)
        okp = None
        if ok is not None:
            ok = A.as_c(ok, np.uint8)
            okp = A.ptr(ok, A.c_u8_p)
        out = np.zeros(max(1, len(pt1)), dtype=np.uint8)
        self.check(lib().msfm_epipolar_filter_batch(self._h, len(offsets) - 1, A.ptr(offsets, A.c_int_p), A.ptr(pt1, A.c_float_p),
                                                    A.ptr(pt2, A.c_float_p), A.ptr(F, A.c_double_p), okp, th, A.ptr(out, A.c_u8_p)))
        return out[:len(pt1)]


class DescSet(_Handle):
    """Device-resident descriptors of a set of images (msfm_descset)."""
    _destroy = "msfm_descset_destroy"

    def __init__(self, ctx: Context, descs, keypoints=None):
        self.ctx = ctx
        self._h = C.c_void_p()
        dim = descs[0].shape[1]
        ctx.check(lib().msfm_descset_create(ctx._h, len(descs), dim, C.byref(self._h)))
        for i, d in enumerate(descs):
            d = A.as_c(d, np.float32)
            ctx.check(lib().msfm_descset_upload(self._h, i, A.ptr(d, A.c_float_p), len(d)))
        self.counts = [len(d) for d in descs]
        if keypoints is not None:
            for i, xy in enumerate(keypoints):
                if xy is not None:
                    self.upload_keypoints(i, xy)

    def upload_keypoints(self, image, xy):
        """msfm_descset_upload_keypoints: [count][2] float positions of the image's features (cv::Point2f)."""
        xy = A.as_c(np.asarray(xy).reshape(-1, 2), np.float32)
        self.ctx.check(lib().msfm_descset_upload_keypoints(self._h, image, A.ptr(xy, A.c_float_p), len(xy)))

    def match_pairs(self, pairs, ratio_good=0.6, ratio_all=0.85, keep_knn=False):
        return MatchResult(self, pairs, ratio_good, ratio_all, keep_knn)

    def match_pairs_slam(self, pairs, F, H, keep_knn=False, **opts):
        """msfm_match_pairs_slam (slam_gps.cc:455-503): ratio test `> th`, then the prior F / H gates; F, H [n_pairs][3][3]."""
        return MatchResult(self, pairs, None, None, keep_knn, slam=(F, H, opts))

    def words(self, tree, min_features=300):
        """msfm_descset_words (Database::BuildWords): the word of every feature of every image with more than min_features
        features, as a `WordResult`."""
        return WordResult(self, tree, min_features)

    def describe(self, image, ss, frames, quantize=False):
        """msfm_descset_describe: the image's descriptors and keypoints become those of the frames [n][4] (x, y, sigma, angle)
        on the scale space `ss`, device to device.  -> the bytes sent (frames and per-frame host values)."""
        fr = A.as_c(np.asarray(frames, dtype=np.float32).reshape(-1, 4), np.float32)
        hb = C.c_int64()
        self.ctx.check(lib().msfm_descset_describe(self._h, int(image), ss._h, A.ptr(fr, A.c_float_p), len(fr), int(bool(quantize)), C.byref(hb)))
        self.counts[image] = len(fr)
        return hb.value

    def extract(self, image, ss, peak_thresh=0.0, edge_thresh=10.0, max_frames=65535, quantize=False):
        """msfm_descset_extract: the keypoints `ss.detect` finds, described into the image of this set without leaving the device
        (the frames alone pass through the host).  -> the stats dict of `ScaleSpace.detect`, describe's waits and bytes added."""
        st = np.zeros(len(A.SIFT_DETECT_STATS), np.int64)
        self.ctx.check(lib().msfm_descset_extract(self._h, int(image), ss._h, float(peak_thresh), float(edge_thresh), int(max_frames),
                                                  int(bool(quantize)), A.ptr(st, C.POINTER(C.c_int64))))
        st = A.sift_detect_stats(st)
        self.counts[image] = min(st["n_found"], int(max_frames))
        return st

    def fetch(self, image):
        """msfm_descset_fetch -> (rows [count][128], xy [count][2] or None for an image without keypoints): what
        featurefiles.write_feature takes."""
        n = lib().msfm_descset_count(self._h, int(image))
        if n < 0:
            raise MsfmError(n, "image %d outside the set" % image)
        rows, xy = np.zeros((n, 128), np.float32), np.zeros((n, 2), np.float32)
        if lib().msfm_descset_fetch(self._h, int(image), A.ptr(rows, A.c_float_p), A.ptr(xy, A.c_float_p)) != 0:
            xy = None
            self.ctx.check(lib().msfm_descset_fetch(self._h, int(image), A.ptr(rows, A.c_float_p), None))
        return rows, xy

    def train_voctree(self, k=10, levels=6, max_iters=11, image_step=1, seed=0):
        """msfm_descset_voctree_train (Database::BuildVocabularyTree): hierarchical k-means over the descriptors of every
        image_step-th image, on the device; the defaults are the reference's.  -> a `VocTree` whose `stats` holds the training's
        statistics (msfm_voctree_train_stats) as a dict."""
        h = C.c_void_p()
        self.ctx.check(lib().msfm_descset_voctree_train(self._h, int(k), int(levels), int(max_iters), int(image_step), int(seed), C.byref(h)))
        return VocTree._adopt(self.ctx, h)


class ScaleSpace(_Handle):
    """msfm_scalespace: the Gaussian levels s = -1 .. S + 1 and the gradient levels 0 .. S - 1 of every octave of one image, on the
    device (include/msfm.h states the definitions).  gray: uint8 [h][w]; stride: bytes per row of the buffer gray is a view of."""
    _destroy = "msfm_scalespace_destroy"

    def __init__(self, ctx: Context, gray, n_octaves=4, n_levels=5, stride=None):
        self.ctx = ctx
        self._h = C.c_void_p()
        gray = np.asarray(gray)
        if gray.dtype != np.uint8 or gray.ndim != 2:
            raise ValueError("gray must be uint8 [h][w]")
        h, w = gray.shape
        if stride is None:
            stride = w
            buf = np.ascontiguousarray(gray)
        else:
            buf = np.zeros((h, max(int(stride), w)), np.uint8)
            buf[:, :w] = gray
            buf[0::2, w:] = 255   # the padding is never read: it would change the range
        self.n_octaves, self.n_levels = int(n_octaves), int(n_levels)
        ctx.check(lib().msfm_scalespace_create(ctx._h, A.ptr(buf, A.c_u8_p), w, h, int(stride), self.n_octaves, self.n_levels, C.byref(self._h)))

    def size(self, octave=0):
        """-> dict(w, h, h2d_bytes) of an octave."""
        w, h, hb = C.c_int32(), C.c_int32(), C.c_int64()
        self.ctx.check(lib().msfm_scalespace_size(self._h, int(octave), C.byref(w), C.byref(h), C.byref(hb)))
        return dict(w=w.value, h=h.value, h2d_bytes=hb.value)

    def detect(self, peak_thresh=0.0, edge_thresh=10.0, max_frames=65535):
        """msfm_scalespace_detect: the DoG extrema of every octave, refined, with their orientations.
        -> (frames [n][4] float32 (x, y, sigma, angle) as `DescSet.describe` takes them, the stats dict: `A.SIFT_DETECT_STATS`)"""
        frames = np.zeros((max(int(max_frames), 0), 4), np.float32)
        n, st = C.c_int32(), np.zeros(len(A.SIFT_DETECT_STATS), np.int64)
        self.ctx.check(lib().msfm_scalespace_detect(self._h, float(peak_thresh), float(edge_thresh), int(max_frames), A.ptr(frames, A.c_float_p),
                                                    C.byref(n), A.ptr(st, C.POINTER(C.c_int64))))
        return frames[:n.value].copy(), A.sift_detect_stats(st)

    def _fetch(self, octave, level, kind):
        z = self.size(octave)
        out = np.zeros((z["h"], z["w"]), np.float32)
        self.ctx.check(lib().msfm_scalespace_fetch(self._h, int(octave), int(level), kind, A.ptr(out, A.c_float_p)))
        return out

    def level(self, octave, level):
        """The GSS level `level` in [-1, S + 1] of an octave, float32 [h_o][w_o]."""
        return self._fetch(octave, level, 0)

    def gradient(self, octave, level):
        """-> (modulus, angle) of level `level` in [0, S - 1] of an octave."""
        return self._fetch(octave, level, 1), self._fetch(octave, level, 2)


class StereoSGM(_Handle):
    """msfm_sgm: census, eight-path semi-global matching and the left disparity of a rectified pair (include/msfm.h, "Dense stereo",
    states the definitions).  It owns its device planes; `execute` replaces the result of the one before."""
    _destroy = "msfm_sgm_destroy"

    def __init__(self, ctx: Context, width, height, disp_size=128, p1=10, p2=120, uniqueness=0.96):
        self.ctx = ctx
        self._h = C.c_void_p()
        self.stats = None
        ctx.check(lib().msfm_sgm_create(ctx._h, int(width), int(height), int(disp_size), int(p1), int(p2), float(uniqueness), C.byref(self._h)))
        self.width, self.height, self.disp_size = int(width), int(height), int(disp_size)

    @staticmethod
    def _image(a, name):
        """-> (the array whose buffer is handed over, its stride in bytes): uint8 [h][w], rows contiguous, any row stride"""
        a = np.asarray(a)
        if a.dtype != np.uint8 or a.ndim != 2:
            raise ValueError("%s must be uint8 [h][w]" % name)
        if a.strides[1] != 1 or a.strides[0] < a.shape[1]:
            a = np.ascontiguousarray(a)
        return a, a.strides[0]

    def execute(self, left, right):
        """msfm_sgm_execute: uploads the pair and enqueues the whole chain without waiting.  -> the stats dict (`A.SGM_STATS`),
        also kept as `self.stats`.  A view with a row stride (a[:, :w] of a wider array) is handed over as it is."""
        (l, ls), (r, rs) = self._image(left, "left"), self._image(right, "right")
        if l.shape != (self.height, self.width) or r.shape != l.shape:
            raise ValueError("the pair must be two images of %d x %d" % (self.width, self.height))
        st = np.zeros(len(A.SGM_STATS), np.int64)
        self.ctx.check(lib().msfm_sgm_execute(self._h, C.cast(l.ctypes.data, A.c_u8_p), int(ls), C.cast(r.ctypes.data, A.c_u8_p), int(rs),
                                              A.ptr(st, C.POINTER(C.c_int64))))
        self.stats = A.sgm_stats(st)
        return self.stats

    def execute_rectified(self, rect):
        """msfm_sgm_execute_rectified: the chain on the rectified planes of a `Rectifier` of this context and size, device to
        device, without waiting.  -> the stats dict (0 bytes to the device), also kept as `self.stats`."""
        st = np.zeros(len(A.SGM_STATS), np.int64)
        self.ctx.check(lib().msfm_sgm_execute_rectified(self._h, rect._h, A.ptr(st, C.POINTER(C.c_int64))))
        self.stats = A.sgm_stats(st)
        return self.stats

    def fetch(self, kind, index=0):
        """msfm_sgm_fetch: waits and returns one plane (`A.SGM_FETCH`): [h][w], the cost volume of path `index` [h][w][D] for kind 2."""
        dt = {k: d for k, _, d in A.SGM_FETCH}.get(int(kind), np.uint8)
        out = np.zeros((self.height, self.width, self.disp_size) if int(kind) == 2 else (self.height, self.width), dt)
        self.ctx.check(lib().msfm_sgm_fetch(self._h, int(kind), int(index), out.ctypes.data_as(C.c_void_p)))
        return out

    def disparity(self):
        """The final left disparity, uint8 [h][w] (0: invalid)."""
        return self.fetch(7)

    def right_disparity(self):
        """The median-filtered right disparity, uint16 [h][w]."""
        return self.fetch(6)

    def depth(self, baseline, focal):
        """msfm_sgm_depth: the depth image of the final disparity, uint8 [h][w]."""
        out = np.zeros((self.height, self.width), np.uint8)
        self.ctx.check(lib().msfm_sgm_depth(self._h, float(baseline), float(focal), A.ptr(out, A.c_u8_p)))
        return out

    def size(self):
        """-> dict(width, height, disp_size, device_bytes)"""
        w, h, d, b = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        self.ctx.check(lib().msfm_sgm_size(self._h, C.byref(w), C.byref(h), C.byref(d), C.byref(b)))
        return dict(width=w.value, height=h.value, disp_size=d.value, device_bytes=b.value)


def _pose_args(K1, R1, t1, K2, R2, t2):
    """-> the six arrays as binary64, row-major, and their pointers in the order the library takes them"""
    arrs = [A.as_c(np.asarray(a, dtype=np.float64).reshape(n), np.float64) for a, n in zip((K1, R1, t1, K2, R2, t2), (9, 9, 3, 9, 9, 3))]
    return arrs, [A.ptr(a, A.c_double_p) for a in arrs]


def stereo_rectify(K1, R1, t1, K2, R2, t2, width, height):
    """msfm_stereo_rectify (host only, no context): the rectification geometry of a posed pair by the definitions of
    include/msfm.h, "Stereo rectification"; camera 1 is the left image.  -> dict(R_left [3][3], R_right [3][3], P_left [3][4],
    P_right [3][4], Q [4][4], idx: 0 a horizontal pair, 1 a vertical one).  MsfmError for poses the header refuses."""
    keep, ptrs = _pose_args(K1, R1, t1, K2, R2, t2)
    out = dict(R_left=np.zeros((3, 3)), R_right=np.zeros((3, 3)), P_left=np.zeros((3, 4)), P_right=np.zeros((3, 4)), Q=np.zeros((4, 4)))
    idx = C.c_int32(-1)
    rc = lib().msfm_stereo_rectify(*ptrs, int(width), int(height), *[A.ptr(v, A.c_double_p) for v in out.values()], C.byref(idx))
    if rc != 0:
        raise MsfmError(rc, "msfm_stereo_rectify: poses or size refused (non-finite, no baseline, a half turn, a side outside [1, 16384])")
    out["idx"] = idx.value
    return out


class Rectifier(_Handle):
    """msfm_rectifier: rectification geometry on the host, maps and bilinear warp of a posed pair on the device (include/msfm.h,
    "Stereo rectification", states the definitions).  It owns its device planes; `rectify` replaces the result of the one before."""
    _destroy = "msfm_rectifier_destroy"

    def __init__(self, ctx: Context, width, height):
        self.ctx = ctx
        self._h = C.c_void_p()
        self.stats = None
        ctx.check(lib().msfm_rectifier_create(ctx._h, int(width), int(height), C.byref(self._h)))
        self.width, self.height = int(width), int(height)

    def rectify(self, left, right, K1, R1, t1, K2, R2, t2, keep_maps=False):
        """msfm_rectifier_rectify: camera 1 (K1, R1, t1) is `left`.  Uploads the pair and enqueues the one launch without waiting.
        -> dict(R_left, R_right, P_left, P_right, stats); the stats (`A.RECTIFY_STATS`) are also kept as `self.stats`."""
        (l, ls), (r, rs) = StereoSGM._image(left, "left"), StereoSGM._image(right, "right")
        if l.shape != (self.height, self.width) or r.shape != l.shape:
            raise ValueError("the pair must be two images of %d x %d" % (self.width, self.height))
        keep, ptrs = _pose_args(K1, R1, t1, K2, R2, t2)
        out = dict(R_left=np.zeros((3, 3)), R_right=np.zeros((3, 3)), P_left=np.zeros((3, 4)), P_right=np.zeros((3, 4)))
        st = np.zeros(len(A.RECTIFY_STATS), np.int64)
        self.ctx.check(lib().msfm_rectifier_rectify(self._h, C.cast(l.ctypes.data, A.c_u8_p), int(ls), C.cast(r.ctypes.data, A.c_u8_p), int(rs),
                                                    *ptrs, int(bool(keep_maps)), *[A.ptr(v, A.c_double_p) for v in out.values()],
                                                    A.ptr(st, C.POINTER(C.c_int64))))
        self.stats = out["stats"] = dict(zip(A.RECTIFY_STATS, (int(v) for v in st)))
        return out

    def fetch(self, kind):
        """msfm_rectifier_fetch: waits and returns one plane [h][w] (`A.RECTIFY_FETCH`): 0 / 1 rectified left / right, 2 .. 5 the maps."""
        dt = {k: d for k, _, d in A.RECTIFY_FETCH}.get(int(kind), np.uint8)
        out = np.zeros((self.height, self.width), dt)
        self.ctx.check(lib().msfm_rectifier_fetch(self._h, int(kind), out.ctypes.data_as(C.c_void_p)))
        return out

    def size(self):
        """-> dict(width, height, device_bytes)"""
        w, h, b = C.c_int32(), C.c_int32(), C.c_int64()
        self.ctx.check(lib().msfm_rectifier_size(self._h, C.byref(w), C.byref(h), C.byref(b)))
        return dict(width=w.value, height=h.value, device_bytes=b.value)


class MatchResult(_Handle):
    _destroy = "msfm_match_result_destroy"

    def __init__(self, ds: DescSet, pairs, ratio_good, ratio_all, keep_knn, slam=None):
        self.ds, self.ctx = ds, ds.ctx
        self.pairs = A.as_c(np.asarray(pairs).reshape(-1, 2), np.int32)
        self.keep_knn = keep_knn
        self.slam = slam is not None
        self._h = C.c_void_p()
        if slam is not None:
            F, H, kw = slam
            F = A.as_c(np.asarray(F, dtype=np.float64).reshape(-1, 9), np.float64)
            H = A.as_c(np.asarray(H, dtype=np.float64).reshape(-1, 9), np.float64)
            if len(F) != len(self.pairs) or len(H) != len(self.pairs):
                raise ValueError("one F and one H per pair")
            o = _options(A.SlamMatchOptions, "msfm_slam_match_default_options", kw)
            self.ctx.check(lib().msfm_match_pairs_slam(ds._h, A.ptr(self.pairs, A.c_int_p), len(self.pairs), A.ptr(F, A.c_double_p),
                                                       A.ptr(H, A.c_double_p), C.byref(o), int(keep_knn), C.byref(self._h)))
            return
        self.ctx.check(lib().msfm_match_pairs(ds._h, A.ptr(self.pairs, A.c_int_p), len(self.pairs), ratio_good,
                                              ratio_all, int(keep_knn), C.byref(self._h)))

    def rerun(self):
        self.ctx.check(lib().msfm_match_pairs_rerun(self.ds._h, self._h))

    def counts(self):
        na, ng = np.zeros(len(self.pairs), np.int32), np.zeros(len(self.pairs), np.int32)
        self.ctx.check(lib().msfm_match_result_counts(self._h, A.ptr(na, A.c_int_p), A.ptr(ng, A.c_int_p)))
        return na, ng

    def stats(self):
        nq, ns = C.c_int32(), C.c_int32()
        self.ctx.check(lib().msfm_match_result_stats(self._h, C.byref(nq), C.byref(ns)))
        return dict(queries=nq.value, slow_path=ns.value)

    def fetch(self, pair):
        nq = self.ds.counts[self.pairs[pair, 1]]
        code = np.zeros(nq, np.int32)
        ids = np.zeros((nq, 2), np.int32) if self.keep_knn else None
        d = np.zeros((nq, 2), np.float32) if self.keep_knn else None
        self.ctx.check(lib().msfm_match_result_fetch(self._h, pair, A.ptr(code, A.c_int_p), A.ptr(ids, A.c_int_p),
                                                     A.ptr(d, A.c_float_p)))
        return code, ids, d


class Chain(_Handle):
    """msfm_chain: match codes -> verification -> tracks -> triangulation -> bundle adjustment, everything resident
    (include/msfm.h).  Built from a MatchResult whose DescSet holds the keypoints."""
    _destroy = "msfm_chain_destroy"

    def __init__(self, res):
        self.ctx, self.res = res.ctx, res
        self.n_pairs = len(res.pairs)
        self._h = C.c_void_p()
        self.ctx.check(lib().msfm_chain_create(res._h, C.byref(self._h)))
        self.slam = bool(getattr(res, "slam", False))

    def verify(self, th_filter=3.0, **opts):
        o = fransac_options(**opts)
        self.ctx.check(lib().msfm_chain_verify(self._h, self.res._h, C.byref(o), th_filter))
        return self._matches()

    def verify_slam(self, res=None, **opts):
        """msfm_chain_verify_slam (slam_gps.cc:503-541): the RANSAC on all survivors of a pair; a pair keeps the entries of the
        mask whatever the verdict, so ok = 0 with n_matches > 0 is a legal outcome.  `res`: the match result to pass (default:
        the one the chain was made from)."""
        o = fransac_options(**opts)
        self.ctx.check(lib().msfm_chain_verify_slam(self._h, (res or self.res)._h, C.byref(o)))
        return self._matches()

    def _matches(self):
        n = np.zeros(max(1, self.n_pairs), np.int32)
        ok = np.zeros(max(1, self.n_pairs), np.uint8)
        F = np.zeros((max(1, self.n_pairs), 3, 3))
        self.ctx.check(lib().msfm_chain_matches(self._h, A.ptr(n, A.c_int_p), A.ptr(ok, A.c_u8_p), A.ptr(F, A.c_double_p)))
        self.n_matches = n[:self.n_pairs]
        return self.n_matches, ok[:self.n_pairs], F[:self.n_pairs]

    def fetch_matches(self, pair):
        m = np.zeros((int(self.n_matches[pair]), 2), np.int32)
        self.ctx.check(lib().msfm_chain_fetch_matches(self._h, pair, A.ptr(m, A.c_int_p)))
        return m

    def build_tracks(self):
        nt, no = C.c_int32(), C.c_int32()
        self.ctx.check(lib().msfm_chain_build_tracks(self._h, C.byref(nt), C.byref(no)))
        self.n_tracks, self.n_obs = nt.value, no.value
        return self.n_tracks, self.n_obs

    def fetch_tracks(self):
        off = np.zeros(self.n_tracks + 1, np.int32)
        img, feat = np.zeros(max(1, self.n_obs), np.int32), np.zeros(max(1, self.n_obs), np.int32)
        self.ctx.check(lib().msfm_chain_fetch_tracks(self._h, A.ptr(off, A.c_int_p), A.ptr(img, A.c_int_p), A.ptr(feat, A.c_int_p)))
        return off, img[:self.n_obs], feat[:self.n_obs]

    def triangulate(self, R, t, c, fk, th_error, th_angle):
        R, t, c, fk = (A.as_c(np.asarray(x, dtype=np.float64), np.float64) for x in (R, t, c, fk))
        n = C.c_int32()
        self.ctx.check(lib().msfm_chain_triangulate(self._h, len(t), A.ptr(R, A.c_double_p), A.ptr(t, A.c_double_p), A.ptr(c, A.c_double_p),
                                                    A.ptr(fk, A.c_double_p), th_error, th_angle, C.byref(n)))
        return n.value

    def fetch_points(self):
        X, mse, ok = np.zeros((max(1, self.n_tracks), 3)), np.zeros(max(1, self.n_tracks)), np.zeros(max(1, self.n_tracks), np.uint8)
        self.ctx.check(lib().msfm_chain_fetch_points(self._h, A.ptr(X, A.c_double_p), A.ptr(mse, A.c_double_p), A.ptr(ok, A.c_u8_p)))
        return X[:self.n_tracks], mse[:self.n_tracks], ok[:self.n_tracks]

    def ba_create(self, cam_pose, cam_model, cam_model_of_cam, min_views=3, weight_ge3=1.0, gps_xyz=None, gps_weight=0.0):
        """msfm_chain_ba_create: returns a BaResident on the accepted tracks (its `.arrays` hold only the camera side: the
        points live on the device; `download()` returns them in `track_of_point` order).  With gps_xyz [n_cams][3]:
        msfm_chain_ba_create_gps, the problem carries the GPS rows of slam_gps.cc:818-830; gps_weight <= 0 is the rule of
        :824 and `gps_weight_used` of the result says what it gave."""
        cam_pose, cam_model = A.as_c(np.array(cam_pose, dtype=np.float64), np.float64), A.as_c(np.array(cam_model, dtype=np.float64), np.float64)
        moc = A.as_c(np.asarray(cam_model_of_cam, dtype=np.int32), np.int32)
        h, npt, nob = C.c_void_p(), C.c_int32(), C.c_int32()
        used = None
        if gps_xyz is None:
            self.ctx.check(lib().msfm_chain_ba_create(self._h, len(cam_pose), len(cam_model), A.ptr(cam_pose, A.c_double_p), A.ptr(cam_model, A.c_double_p),
                                                      A.ptr(moc, A.c_int_p), min_views, weight_ge3, C.byref(h), C.byref(npt), C.byref(nob)))
        else:
            g = A.as_c(np.asarray(gps_xyz, dtype=np.float64).reshape(-1, 3), np.float64)
            if len(g) != len(cam_pose):
                raise ValueError("ba_create: gps_xyz needs one row per camera")
            w = C.c_double()
            self.ctx.check(lib().msfm_chain_ba_create_gps(self._h, len(cam_pose), len(cam_model), A.ptr(cam_pose, A.c_double_p),
                                                          A.ptr(cam_model, A.c_double_p), A.ptr(moc, A.c_int_p), min_views, weight_ge3,
                                                          A.ptr(g, A.c_double_p), gps_weight, C.byref(w), C.byref(h), C.byref(npt), C.byref(nob)))
            used = w.value
        top = np.zeros(npt.value, np.int32)
        self.ctx.check(lib().msfm_chain_fetch_point_tracks(self._h, A.ptr(top, A.c_int_p)))

        class _Shapes:   # what BaResident.download needs to size its buffers
            pass
        sh = _Shapes()
        sh.cam_pose, sh.cam_model, sh.point = cam_pose, cam_model, np.zeros((npt.value, 3))
        ba = BaResident.__new__(BaResident)
        ba.ctx, ba.arrays, ba._h = self.ctx, sh, h
        ba.track_of_point, ba.n_obs = top, nob.value
        if used is not None:
            ba.gps_weight_used = used
        return ba

    def accuracy(self, R, t, fk, cam_dc=None, min_views=3, th_outlier=3.0):
        """msfm_chain_accuracy (GetAccuracy): the resident ok becomes ok_out; returns (n_outliers, n_inliers)."""
        R, t, fk, dc = (A.as_c(None if x is None else np.asarray(x, dtype=np.float64), np.float64) for x in (R, t, fk, cam_dc))
        n_out, n_in = C.c_int32(), C.c_int32()
        self.ctx.check(lib().msfm_chain_accuracy(self._h, len(t), A.ptr(R, A.c_double_p), A.ptr(t, A.c_double_p), A.ptr(fk, A.c_double_p),
                                                 A.ptr(dc, A.c_double_p), min_views, th_outlier, C.byref(n_out), C.byref(n_in)))
        return n_out.value, n_in.value

    def fetch_accuracy(self):
        n = max(1, self.n_tracks)
        e_avg, e_mse, n_used = np.zeros(n), np.zeros(n), np.zeros(n, np.int32)
        self.ctx.check(lib().msfm_chain_fetch_accuracy(self._h, A.ptr(e_avg, A.c_double_p), A.ptr(e_mse, A.c_double_p), A.ptr(n_used, A.c_int_p)))
        return e_avg[:self.n_tracks], e_mse[:self.n_tracks], n_used[:self.n_tracks]

    def gps_register(self, cam_c, gps):
        """msfm_chain_gps_register: the point loop of GPSRegistration2 on the resident X."""
        c, g = (A.as_c(np.asarray(x, dtype=np.float64).reshape(-1, 3), np.float64) for x in (cam_c, gps))
        if len(c) != len(g):
            raise ValueError("gps_register: cam_c and gps need one row per camera")
        self.ctx.check(lib().msfm_chain_gps_register(self._h, len(c), A.ptr(c, A.c_double_p), A.ptr(g, A.c_double_p)))

    def store_points(self, ba):
        """msfm_chain_store_points: the adjusted points of `ba` (the BaResident this chain made last) back into the resident X."""
        self.ctx.check(lib().msfm_chain_store_points(self._h, ba._h))


class MatchStore(_Handle):
    """msfm_match_store: the verified matches of an image set resident on the device, indexed by idx1 (include/msfm.h)."""
    _destroy = "msfm_match_store_destroy"

    def __init__(self, ctx: Context, n_features, pairs, match_off, matches):
        self.ctx = ctx
        self._h = C.c_void_p()
        nf, off = (A.as_c(np.asarray(x, dtype=np.int32), np.int32) for x in (n_features, match_off))
        pr = A.as_c(np.asarray(pairs, dtype=np.int32).reshape(-1, 2), np.int32)
        fl = A.as_c(np.asarray(matches, dtype=np.int32).reshape(-1, 2), np.int32)
        if len(off) != len(pr) + 1 or (len(pr) and len(fl) < off[-1]):
            raise ValueError("match_off must have one entry more than pairs and end inside matches")
        self.n_features = nf
        ctx.check(lib().msfm_match_store_create(ctx._h, len(nf), A.ptr(nf, A.c_int_p), len(pr), A.ptr(pr, A.c_int_p), A.ptr(off, A.c_int_p),
                                                A.ptr(fl, A.c_int_p), C.byref(self._h)))

    @classmethod
    def from_chain(cls, chain):
        """msfm_match_store_from_chain: the matches (and keypoints) of a verified Chain, copied device to device."""
        self = cls.__new__(cls)
        self.ctx, self._h = chain.ctx, C.c_void_p()
        self.n_features = np.asarray(chain.res.ds.counts, dtype=np.int32)
        self.ctx.check(lib().msfm_match_store_from_chain(chain._h, C.byref(self._h)))
        return self


class Wordset(_Handle):
    """msfm_wordset: which image pairs to match, from the word id of every feature (include/msfm.h)."""
    _destroy = "msfm_wordset_destroy"

    def __init__(self, ctx: Context, n_features, words, num_words, keypoints, max_hypotheses=0):
        self.ctx = ctx
        self._h = C.c_void_p()
        nf = A.as_c(np.asarray(n_features, dtype=np.int32).reshape(-1), np.int32)
        if len(words) != len(nf):
            raise ValueError("one word list (or None) per image")
        has = np.array([w is not None and len(w) > 0 for w in words], dtype=np.uint8)
        off = np.concatenate([[0], np.cumsum(nf, dtype=np.int64)])
        flat = np.zeros(max(1, int(off[-1])), dtype=np.int32)
        for k, w in enumerate(words):
            if has[k]:
                if len(w) != nf[k]:
                    raise ValueError("image %d: %d word ids for %d features" % (k, len(w), nf[k]))
                flat[off[k]:off[k + 1]] = w
        kp = A.as_c(np.asarray(keypoints, dtype=np.float32).reshape(-1, 2), np.float32)
        if len(kp) != off[-1]:
            raise ValueError("keypoints must hold one row per feature of every image")
        ctx.check(lib().msfm_wordset_create(ctx._h, len(nf), A.ptr(nf, A.c_int_p), A.ptr(has, A.c_u8_p), A.ptr(flat, A.c_int_p), int(num_words),
                                            A.ptr(kp, A.c_float_p), int(max_hypotheses), C.byref(self._h)))
        self._read_size()

    @classmethod
    def _adopt(cls, ctx, handle):
        """A set the library made by another route (msfm_wordset_create_from_words)."""
        ws = cls.__new__(cls)
        ws.ctx, ws._h = ctx, handle
        ws._read_size()
        return ws

    def _read_size(self):
        n, k, ni, nm, nb = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64(), C.c_int64()
        lib().msfm_wordset_size(self._h, C.byref(n), C.byref(k), C.byref(ni), C.byref(nm), C.byref(nb))
        self.n_images, self.n_hypotheses, self.n_inverted, self.n_mapped, self.h2d_bytes = n.value, k.value, ni.value, nm.value, nb.value

    def fetch(self, similarity=True):
        """msfm_wordset_fetch: dict of similarity [n][n] (or None), hyp_img / hyp_sim [n][K], map_off [n + 1], map_word, map_feat."""
        n, k, m = self.n_images, self.n_hypotheses, max(1, self.n_mapped)
        S = np.zeros((n, n), np.int32) if similarity else None
        hi, hs = np.zeros((n, k), np.int32), np.zeros((n, k), np.int32)
        mo, mw, mf = np.zeros(n + 1, np.int32), np.zeros(m, np.int32), np.zeros(m, np.int32)
        ip = A.c_int_p
        self.ctx.check(lib().msfm_wordset_fetch(self._h, A.ptr(S, ip), A.ptr(hi, ip), A.ptr(hs, ip), A.ptr(mo, ip), A.ptr(mw, ip), A.ptr(mf, ip)))
        return {"similarity": S, "hyp_img": hi, "hyp_sim": hs, "map_off": mo, "map_word": mw[:self.n_mapped], "map_feat": mf[:self.n_mapped]}

    def select(self, first_image=0, n_rows=None, details=True, **opts):
        """msfm_pair_select for the rows [first_image, first_image + n_rows) (default: to the last image); opts: fields of
        msfm_pair_select_options and of its msfm_fransac_options.  Returns a dict: pairs [n_kept][2], n_init / n_inliers /
        verdict [rows][K] and, with details, F [rows][K][3][3], init_off, init_matches [..][2], init_inlier."""
        rows = self.n_images - first_image if n_rows is None else n_rows
        o = pair_select_options(**opts)
        h = C.c_void_p()
        self.ctx.check(lib().msfm_pair_select(self._h, first_image, rows, C.byref(o), C.byref(h)))
        with _Handle(h, "msfm_pair_set_destroy"):
            nr, k, nk, tot = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
            lib().msfm_pair_set_size(h, C.byref(nr), C.byref(k), C.byref(nk), C.byref(tot))
            rows, k, nk, tot = nr.value, k.value, nk.value, tot.value
            ni, nin, ver = np.zeros((rows, k), np.int32), np.zeros((rows, k), np.int32), np.zeros((rows, k), np.uint8)
            pairs = np.zeros((max(1, nk), 2), np.int32)
            F = np.zeros((rows, k, 3, 3)) if details else None
            off = np.zeros(rows * k + 1, np.int32) if details else None
            im = np.zeros((max(1, tot), 2), np.int32) if details else None
            inl = np.zeros(max(1, tot), np.uint8) if details else None
            lib().msfm_pair_set_fetch(h, A.ptr(ni, A.c_int_p), A.ptr(nin, A.c_int_p), A.ptr(ver, A.c_u8_p), A.ptr(pairs, A.c_int_p),
                                      A.ptr(F, A.c_double_p), A.ptr(off, A.c_int_p), A.ptr(im, A.c_int_p), A.ptr(inl, A.c_u8_p))
        out = {"pairs": pairs[:nk], "n_init": ni, "n_inliers": nin, "verdict": ver}
        if details:
            out.update(F=F, init_off=off, init_matches=im[:tot], init_inlier=inl[:tot])
        return out


class VocTree(_Handle):
    """msfm_voctree: a vocabulary tree resident on the device (include/msfm.h).  block_n [n_blocks], node_desc [n_blocks][k][128],
    node_link / node_weight [n_blocks][k]: what featurefiles.read_voctree returns."""
    _destroy = "msfm_voctree_destroy"

    def __init__(self, ctx: Context, k, block_n, node_desc, node_link, node_weight):
        self.ctx = ctx
        self._h = C.c_void_p()
        bn = A.as_c(np.asarray(block_n).reshape(-1), np.uint16)
        nb = len(bn)
        nd = A.as_c(np.asarray(node_desc, dtype=np.float32).reshape(nb, int(k), 128), np.float32)
        nl = A.as_c(np.asarray(node_link).reshape(nb, int(k)), np.uint32)
        nw = A.as_c(np.asarray(node_weight, dtype=np.float32).reshape(nb, int(k)), np.float32)
        ctx.check(lib().msfm_voctree_create(ctx._h, int(k), nb, A.ptr(bn, C.POINTER(C.c_uint16)), A.ptr(nd, A.c_float_p),
                                            A.ptr(nl, C.POINTER(C.c_uint32)), A.ptr(nw, A.c_float_p), C.byref(self._h)))

    stats = None   # msfm_voctree_train_stats of a trained tree (DescSet.train_voctree) as a dict; None for an uploaded one

    @classmethod
    def _adopt(cls, ctx, handle):
        """A tree the library made on the device (msfm_descset_voctree_train)."""
        vt = cls.__new__(cls)
        vt.ctx, vt._h = ctx, handle
        ni, nb, d, ws, ss, hw = (C.c_int32() for _ in range(6))
        nf, nl = C.c_int64(), C.c_int64()
        lv = {name: np.zeros(32, np.int32) for name in ("level_nodes", "level_split", "level_max_iters", "level_capped")}
        ctx.check(lib().msfm_voctree_train_stats(handle, C.byref(ni), C.byref(nf), C.byref(nb), C.byref(nl), C.byref(d), C.byref(ws), C.byref(ss),
                                                 C.byref(hw), *(A.ptr(v, A.c_int_p) for v in lv.values())))
        vt.stats = dict(n_images=ni.value, n_features=nf.value, n_blocks=nb.value, n_leaves=nl.value, depth=d.value, weight_shift=ws.value,
                        sum_shift=ss.value, host_waits=hw.value, **{name: v[:max(1, d.value)].tolist() for name, v in lv.items()})
        return vt

    def fetch(self):
        """msfm_voctree_fetch: dict of k, block_n [nb], node_desc [nb][k][128], node_link / node_weight [nb][k], block_leaf,
        block_parent [nb] - the keywords of featurefiles.write_voctree, and (without the last two) of Context.voctree."""
        z = self.size()
        nb, k = z["n_blocks"], z["k"]
        bn, bl, bp = np.zeros(nb, np.uint16), np.zeros(nb, np.uint16), np.zeros(nb, np.uint32)
        nd, nl, nw = np.zeros((nb, k, 128), np.float32), np.zeros((nb, k), np.uint32), np.zeros((nb, k), np.float32)
        u16, u32 = C.POINTER(C.c_uint16), C.POINTER(C.c_uint32)
        self.ctx.check(lib().msfm_voctree_fetch(self._h, A.ptr(bn, u16), A.ptr(nd, A.c_float_p), A.ptr(nl, u32), A.ptr(nw, A.c_float_p),
                                                A.ptr(bl, u16), A.ptr(bp, u32)))
        return dict(k=k, block_n=bn, node_desc=nd, node_link=nl, node_weight=nw, block_leaf=bl, block_parent=bp)

    def size(self):
        """-> dict(k, n_blocks, depth, n_leaves, h2d_bytes)."""
        k, nb, d, nl, hb = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
        lib().msfm_voctree_size(self._h, C.byref(k), C.byref(nb), C.byref(d), C.byref(nl), C.byref(hb))
        return dict(k=k.value, n_blocks=nb.value, depth=d.value, n_leaves=nl.value, h2d_bytes=hb.value)


class WordResult(_Handle):
    """msfm_word_result: the word of every feature of a descriptor set, its bags of words and maxima, on the device."""
    _destroy = "msfm_word_result_destroy"

    def __init__(self, ds, tree: VocTree, min_features=300):
        self.ctx, self.ds = ds.ctx, ds
        self._h = C.c_void_p()
        self.ctx.check(lib().msfm_descset_words(ds._h, tree._h, int(min_features), C.byref(self._h)))

    def size(self):
        """-> dict(n_images, n_features, n_bow, num_words, n_unassigned)."""
        n, nf, nb, nw, nu = C.c_int32(), C.c_int64(), C.c_int64(), C.c_int32(), C.c_int64()
        lib().msfm_word_result_size(self._h, C.byref(n), C.byref(nf), C.byref(nb), C.byref(nw), C.byref(nu))
        return dict(n_images=n.value, n_features=nf.value, n_bow=nb.value, num_words=nw.value, n_unassigned=nu.value)

    def fetch(self):
        """msfm_word_result_fetch: dict of feat_off [n + 1], has_words [n], word_id [n_features], image_max_id [n], bow_off [n + 1],
        bow_word / bow_weight [n_bow]."""
        z = self.size()
        n, nf, nb = z["n_images"], z["n_features"], z["n_bow"]
        fo, hw, wid = np.zeros(n + 1, np.int32), np.zeros(n, np.uint8), np.zeros(max(1, nf), np.int32)
        mx, bo = np.zeros(n, np.int32), np.zeros(n + 1, np.int32)
        bw, bf = np.zeros(max(1, nb), np.int32), np.zeros(max(1, nb), np.float32)
        ip = A.c_int_p
        self.ctx.check(lib().msfm_word_result_fetch(self._h, A.ptr(fo, ip), A.ptr(hw, A.c_u8_p), A.ptr(wid, ip), A.ptr(mx, ip), A.ptr(bo, ip),
                                                    A.ptr(bw, ip), A.ptr(bf, A.c_float_p)))
        return {"feat_off": fo, "has_words": hw, "word_id": wid[:nf], "image_max_id": mx, "bow_off": bo, "bow_word": bw[:nb],
                "bow_weight": bf[:nb]}

    def wordset(self, max_hypotheses=0):
        """msfm_wordset_create_from_words: the `Wordset` of these words and the descriptor set's resident keypoints."""
        h = C.c_void_p()
        self.ctx.check(lib().msfm_wordset_create_from_words(self.ds._h, self._h, int(max_hypotheses), C.byref(h)))
        return Wordset._adopt(self.ctx, h)


class SeedSet(_Handle):
    """msfm_seed_set kept alive behind `Context.seed_hypotheses(keep=True)`: the winner's points stay on the device."""
    _destroy = "msfm_seed_set_destroy"

    def __init__(self, ctx: Context, store, h):
        self.ctx, self.store, self._h = ctx, store, h


class Recon(_Handle):
    """msfm_recon: a model's flat state resident on the device across its rounds (include/msfm.h)."""
    _destroy = "msfm_recon_destroy"
    INT = ("cam_img", "feat_point", "obs_point", "obs_cam", "obs_feat", "pt_views")
    U8 = ("pt_bad", "pt_mutable", "pt_new_added")

    def __init__(self, ctx: Context, store, state, cam_pose, cam_model, cam_model_of_cam, keypoints=None, model_mutable=None, reserve_points=0,
                 reserve_obs=0):
        self.ctx, self.store, self._h, self._n_visible = ctx, store, C.c_void_p(), 0
        ip, dp, up = A.c_int_p, A.c_double_p, A.c_u8_p
        a = {k: A.as_c(np.asarray(state[k], dtype=np.int32).reshape(-1), np.int32) for k in self.INT}
        a.update({k: A.as_c(np.asarray(state[k], dtype=np.uint8).reshape(-1), np.uint8) for k in self.U8 if state.get(k) is not None})
        a["cam_model_of_cam"] = A.as_c(np.asarray(cam_model_of_cam, dtype=np.int32).reshape(-1), np.int32)
        for k, v, w in (("cam_pose", cam_pose, 6), ("cam_model", cam_model, 3), ("cam_R", state["cam_R"], 9), ("cam_t", state["cam_t"], 3),
                        ("cam_c", state["cam_c"], 3), ("cam_fk", state["cam_fk"], 3), ("point_xyz", state["point_xyz"], 3), ("pt_mse", state["pt_mse"], 1)):
            a[k] = A.as_c(np.asarray(v, dtype=np.float64).reshape(-1, w), np.float64)
        nc, no, npt, nm = len(a["cam_img"]), len(a["obs_point"]), len(a["point_xyz"]), len(a["cam_model"])
        if not all(len(a[k]) == nc for k in ("cam_pose", "cam_model_of_cam", "cam_R", "cam_t", "cam_c", "cam_fk")):
            raise ValueError("cam_img, cam_pose, cam_model_of_cam and cam_R / cam_t / cam_c / cam_fk must describe the same number of cameras")
        if not (len(a["obs_cam"]) == len(a["obs_feat"]) == no):
            raise ValueError("obs_point, obs_cam and obs_feat must hold one entry per observation")
        if not all(len(a[k]) == npt for k in ("pt_mse", "pt_views", "pt_bad", "pt_mutable")) or len(a.get("pt_new_added", a["pt_bad"])) != npt:
            raise ValueError("point_xyz, pt_bad, pt_mse, pt_views, pt_mutable and pt_new_added must hold one entry per point")
        mm = None if model_mutable is None else A.as_c(np.asarray(model_mutable, dtype=np.uint8).reshape(-1), np.uint8)
        if mm is not None and len(mm) != nm:
            raise ValueError("model_mutable must hold one entry per model")
        in_store = (a["cam_img"] >= 0) & (a["cam_img"] < len(store.n_features))     # (an image outside the store: the library reports it)
        if in_store.all() and len(a["feat_point"]) != int(store.n_features[a["cam_img"]].sum()):
            raise ValueError("feat_point must hold one entry per feature of every camera's image")
        kp = None if keypoints is None else A.as_c(np.asarray(keypoints, dtype=np.float32).reshape(-1, 2), np.float32)
        if kp is not None and len(kp) != int(store.n_features.sum()):
            raise ValueError("keypoints must hold one row per feature of every image")
        g = a.get
        P = A.ReconInit(nc, A.ptr(g("cam_img"), ip), A.ptr(g("feat_point"), ip), npt, A.ptr(kp, A.c_float_p), no, A.ptr(g("obs_point"), ip),
                        A.ptr(g("obs_cam"), ip), A.ptr(g("obs_feat"), ip), A.ptr(g("cam_pose"), dp), nm, A.ptr(g("cam_model"), dp),
                        A.ptr(g("cam_model_of_cam"), ip), A.ptr(mm, up), A.ptr(g("cam_R"), dp), A.ptr(g("cam_t"), dp), A.ptr(g("cam_c"), dp),
                        A.ptr(g("cam_fk"), dp), A.ptr(g("point_xyz"), dp), A.ptr(g("pt_bad"), up), A.ptr(g("pt_mse"), dp), A.ptr(g("pt_views"), ip),
                        A.ptr(g("pt_mutable"), up), A.ptr(g("pt_new_added"), up), int(reserve_points), int(reserve_obs))
        ctx.check(lib().msfm_recon_create(ctx._h, store._h, C.byref(P), C.byref(self._h)))

    @classmethod
    def from_seed(cls, ctx: Context, store, seed_set, cam_pose, cam_model, cam_model_of_cam, keypoints=None, model_mutable=None, reserve_points=0,
                  reserve_obs=0):
        """msfm_recon_create_from_seed: the two-camera model of `seed_set`'s winner (a `SeedSet` of `seed_hypotheses(keep=True)` on
        this store), made on the device from the points the set keeps there.  cam_pose [2][6], cam_model [n_models][3] (one or two
        models) and cam_model_of_cam [2] are the solver's blocks, as `seed.find_seed_pair` returns them."""
        pose = A.as_c(np.asarray(cam_pose, dtype=np.float64).reshape(2, 6), np.float64)
        model = A.as_c(np.asarray(cam_model, dtype=np.float64).reshape(-1, 3), np.float64)
        moc = A.as_c(np.asarray(cam_model_of_cam, dtype=np.int32).reshape(2), np.int32)
        mm = None if model_mutable is None else A.as_c(np.asarray(model_mutable, dtype=np.uint8).reshape(-1), np.uint8)
        if mm is not None and len(mm) != len(model):
            raise ValueError("model_mutable must hold one entry per model")
        kp = None if keypoints is None else A.as_c(np.asarray(keypoints, dtype=np.float32).reshape(-1, 2), np.float32)
        if kp is not None and len(kp) != int(store.n_features.sum()):
            raise ValueError("keypoints must hold one row per feature of every image")
        q = cls.__new__(cls)
        q.ctx, q.store, q._h, q._n_visible = ctx, store, C.c_void_p(), 0
        ctx.check(lib().msfm_recon_create_from_seed(ctx._h, store._h, seed_set._h, A.ptr(pose, A.c_double_p), len(model), A.ptr(model, A.c_double_p),
                                                    A.ptr(moc, A.c_int_p), A.ptr(mm, A.c_u8_p), A.ptr(kp, A.c_float_p), int(reserve_points),
                                                    int(reserve_obs), C.byref(q._h)))
        return q

    def normalize(self, noise=None, target_deviation=100.0, point_sigma=0.5):
        """msfm_recon_normalize: the point side of BundleAdjuster::Normalize and Perturb on the resident points.  noise [n_points][3]
        standard normal draws (None: no perturbation); the defaults are the reference's values.  Returns (mid [3], scale)."""
        nz = None
        if noise is not None:
            nz = A.as_c(np.asarray(noise, dtype=np.float64).reshape(-1, 3), np.float64)
            if len(nz) != self.size()["n_points"]:
                raise ValueError("noise must hold one row per point")
        mid, scale = np.zeros(3), C.c_double()
        self.ctx.check(lib().msfm_recon_normalize(self._h, A.ptr(nz, A.c_double_p), float(target_deviation), float(point_sigma),
                                                  A.ptr(mid, A.c_double_p), C.byref(scale)))
        return mid, scale.value

    def set_cameras(self, cam_pose=None, cam_R=None, cam_t=None, cam_c=None):
        """msfm_recon_set_cameras: replaces the object's host camera tables (None keeps one): cam_pose [n_cams][6], cam_R
        [n_cams][3][3], cam_t, cam_c [n_cams][3]."""
        nc = self.size()["n_cams"]
        a = [None if v is None else A.as_c(np.asarray(v, dtype=np.float64).reshape(nc, w), np.float64)
             for v, w in ((cam_pose, 6), (cam_R, 9), (cam_t, 3), (cam_c, 3))]
        self.ctx.check(lib().msfm_recon_set_cameras(self._h, *[A.ptr(v, A.c_double_p) for v in a]))

    def size(self):
        """msfm_recon_size: n_cams, n_models, n_points, n_obs, cap_points, cap_obs and h2d_bytes (sent since creation, creation included)."""
        n = [C.c_int32() for _ in range(4)]
        b = [C.c_int64() for _ in range(3)]
        self.ctx.check(lib().msfm_recon_size(self._h, *[C.byref(x) for x in n + b]))
        return dict(zip(("n_cams", "n_models", "n_points", "n_obs", "cap_points", "cap_obs", "h2d_bytes"), [x.value for x in n + b]))

    def fetch(self):
        """msfm_recon_fetch: the flat state as a dict in the dtypes and shapes of `newpoints.py`, plus cam_pose, cam_model and
        cam_model_of_cam."""
        ip, dp, up = A.c_int_p, A.c_double_p, A.c_u8_p
        z = self.size()
        nc, nm, npt, no = z["n_cams"], z["n_models"], z["n_points"], z["n_obs"]
        cam_img = np.zeros(max(1, nc), np.int32)
        self.ctx.check(lib().msfm_recon_fetch(self._h, A.ptr(cam_img, ip), *[None] * 17))
        nfp = int(self.store.n_features[cam_img[:nc]].sum())
        i32, f64, u8 = np.int32, np.float64, np.uint8
        # (key, rows, trailing shape, dtype) in the order of msfm_recon_fetch behind cam_img
        spec = [("feat_point", nfp, (), i32), ("obs_point", no, (), i32), ("obs_cam", no, (), i32), ("obs_feat", no, (), i32),
                ("point_xyz", npt, (3,), f64), ("pt_bad", npt, (), u8), ("pt_mse", npt, (), f64), ("pt_views", npt, (), i32),
                ("pt_mutable", npt, (), u8), ("pt_new_added", npt, (), u8), ("cam_pose", nc, (6,), f64), ("cam_model", nm, (3,), f64),
                ("cam_model_of_cam", nc, (), i32), ("cam_R", nc, (3, 3), f64), ("cam_t", nc, (3,), f64), ("cam_c", nc, (3,), f64), ("cam_fk", nc, (3,), f64)]
        bufs = [np.zeros((max(1, rows),) + shape, dt) for _, rows, shape, dt in spec]
        typ = {i32: ip, f64: dp, u8: up}
        self.ctx.check(lib().msfm_recon_fetch(self._h, None, *[A.ptr(b, typ[dt]) for b, (_, _, _, dt) in zip(bufs, spec)]))
        out = {"n_features": np.array(self.store.n_features), "cam_img": cam_img[:nc]}
        out.update({key: b[:rows] for b, (key, rows, _, _) in zip(bufs, spec)})
        return out

    def localize(self, cand_img, fail_times, cand_f, cand_f_init=None, **opts):
        """msfm_recon_localize: FindImageToLocalize and the try loop on the resident state.  cand_img ascending, fail_times, cand_f
        (0.0: the sweep around cand_f_init) per candidate; opts: fields of msfm_localize_pose_options.  Returns a dict in the keys of
        `localize.localize_next_image`: image (-1: none), row, image_ids, failed_images, n_calls and, with a winner, f, R, t,
        avg_error, n_inliers, n_outliers, visible.  The winner stays pending in the object for `commit_camera`."""
        ip, dp = A.c_int_p, A.c_double_p
        cand, fail = (A.as_c(np.asarray(x, dtype=np.int32).reshape(-1), np.int32) for x in (cand_img, fail_times))
        f = A.as_c(np.asarray(cand_f, dtype=np.float64).reshape(-1), np.float64)
        fi = None if cand_f_init is None else A.as_c(np.asarray(cand_f_init, dtype=np.float64).reshape(-1), np.float64)
        if not (len(fail) == len(f) == len(cand)) or (fi is not None and len(fi) != len(cand)):
            raise ValueError("cand_img, fail_times, cand_f and cand_f_init must hold one entry per candidate")
        o = localize_pose_options(**opts)
        w = A.ReconWinner()
        self.ctx.check(lib().msfm_recon_localize(self._h, len(cand), A.ptr(cand, ip), A.ptr(fail, ip), A.ptr(f, dp), A.ptr(fi, dp), C.byref(o), C.byref(w)))
        ranked, failed, vis = np.zeros(max(1, w.n_ranked), np.int32), np.zeros(max(1, w.n_failed), np.int32), np.zeros(max(1, w.n_visible), np.int32)
        self.ctx.check(lib().msfm_recon_localize_fetch(self._h, A.ptr(ranked, ip), A.ptr(failed, ip), A.ptr(vis, ip)))
        self._n_visible = int(w.n_visible)
        out = dict(image=int(w.image), row=int(w.row), image_ids=[int(x) for x in ranked[:w.n_ranked]],
                   failed_images=[int(x) for x in failed[:w.n_failed]], n_calls=int(w.n_chunks))
        if w.image >= 0:
            out.update(f=float(w.f), R=np.array(w.R, np.float64).reshape(3, 3), t=np.array(w.t, np.float64), avg_error=float(w.avg_error),
                       n_inliers=int(w.n_inliers), n_outliers=int(w.n_outliers), n_corr=int(w.n_corr), visible=vis[:w.n_visible].copy())
        return out

    def commit_camera(self, cam_pose6, model, cam_model3=None, model_mutable=True):
        """msfm_recon_commit_camera: `localize.apply_localized_image` for the pending winner, on the device.  cam_pose6: the new
        camera's angle-axis and translation; model: an existing model, or n_models with cam_model3 = (f, k1, k2) to append one.
        Returns the visible list, the new camera first."""
        pose = A.as_c(np.asarray(cam_pose6, dtype=np.float64).reshape(6), np.float64)
        m3 = None if cam_model3 is None else A.as_c(np.asarray(cam_model3, dtype=np.float64).reshape(3), np.float64)
        vis = np.zeros(1 + self._n_visible, np.int32)
        new_cam = C.c_int32()
        self.ctx.check(lib().msfm_recon_commit_camera(self._h, A.ptr(pose, A.c_double_p), int(model), A.ptr(m3, A.c_double_p), int(bool(model_mutable)),
                                                      C.byref(new_cam), A.ptr(vis, A.c_int_p)))
        return [int(x) for x in vis]

    def new_points(self, new_cam, visible, stats=False, **opts):
        """msfm_recon_new_points: `Context.new_points` for the camera `new_cam` and its visible list on the resident state, the new
        points appended on the device as `newpoints.apply_new_points` appends them to the flat state.  Returns their number;
        with stats=True the dict of `Context.new_points` (h2d_bytes: of this call) with n_new added.  opts: fields of
        msfm_new_points_options."""
        visible = A.as_c(np.asarray(visible, dtype=np.int32).reshape(-1), np.int32)
        o = new_points_options(**opts)
        n, h = C.c_int32(), C.c_void_p()
        self.ctx.check(lib().msfm_recon_new_points(self._h, int(new_cam), len(visible), A.ptr(visible, A.c_int_p), C.byref(o), C.byref(n),
                                                   C.byref(h) if stats else None))
        if not stats:
            return n.value
        with _Handle(h, "msfm_new_points_set_destroy"):
            return dict(_new_points_set_result(h, 1), n_new=n.value)

    def adjust(self, new_cam=-1, visible=(), partial=True, full=False, outliers=True, capacity=512, **opts):
        """msfm_recon_adjust: `Context.round_adjust` on the resident state, written in place.  Returns its dict without the point
        arrays (they stay on the device; `fetch()` reads them): cam_pose, cam_model, cam_R, cam_t, cam_c, cam_fk, the counts,
        adjust_cams / adjust_pts, solved, summary, h2d_bytes (of this call) and, with keep_problem=1, problem."""
        visible = A.as_c(np.asarray(visible, dtype=np.int32).reshape(-1), np.int32)
        opts = dict(opts)
        for k in ("partial", "full"):
            if k + "_options" in opts:
                opts[k] = opts.pop(k + "_options")
        o = round_options(**opts)
        z = self.size()
        h = C.c_void_p()
        self.ctx.check(lib().msfm_recon_adjust(self._h, int(new_cam), len(visible), A.ptr(visible, A.c_int_p), int(bool(partial)), int(bool(full)),
                                               int(bool(outliers)), C.byref(o), C.byref(h)))
        with _Handle(h, "msfm_round_set_destroy"):
            out = _round_set_result(self.ctx, h, z["n_cams"], z["n_models"], 0, partial, full, o.keep_problem, capacity)
        for k in ("point_xyz", "pt_mutable", "pt_bad", "pt_mse", "pt_new_added", "pt_views"):
            del out[k]
        return out


class LocalizeSet(_Handle):
    """msfm_localize_set: the ranked candidates of one round; made with point_xyz it keeps their correspondences on the device."""
    _destroy = "msfm_localize_set_destroy"

    def __init__(self, ctx: Context, h):
        self.ctx, self._h = ctx, h
        nk, nc, nv, hp, nb = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        lib().msfm_localize_set_size(h, C.byref(nk), C.byref(nc), C.byref(nv), C.byref(hp), C.byref(nb))
        self.n_kept, self.n_corr, self.n_visible, self.has_points, self.h2d_bytes = nk.value, nc.value, nv.value, bool(hp.value), nb.value

    def fetch(self):
        nk, nc, nv = self.n_kept, self.n_corr, self.n_visible
        rank, coff, voff = np.zeros(max(1, nk), np.int32), np.zeros(nk + 1, np.int32), np.zeros(nk + 1, np.int32)
        cf, cp, vc = np.zeros(max(1, nc), np.int32), np.zeros(max(1, nc), np.int32), np.zeros(max(1, nv), np.int32)
        pw = np.zeros((max(1, nc), 3)) if self.has_points else None
        p2 = np.zeros((max(1, nc), 2)) if self.has_points else None
        lib().msfm_localize_set_fetch(self._h, A.ptr(rank, A.c_int_p), A.ptr(coff, A.c_int_p), A.ptr(cf, A.c_int_p), A.ptr(cp, A.c_int_p),
                                      A.ptr(voff, A.c_int_p), A.ptr(vc, A.c_int_p), A.ptr(pw, A.c_double_p), A.ptr(p2, A.c_double_p))
        out = dict(rank=rank[:nk], corr_off=coff, corr_feat=cf[:nc], corr_point=cp[:nc], vis_off=voff, vis_cam=vc[:nv], h2d_bytes=self.h2d_bytes)
        if self.has_points:
            out["pts_w"], out["pts_2d"] = pw[:nc], p2[:nc]
        return out

    def poses(self, row_f, row_f_init=None, n_points=0, pt_new_added=None, **opts):
        """msfm_localize_poses (sfm_incremental.cc:143-164 around :565-753): the tries of the ranked rows in one call.  row_f [n_kept]
        (0.0 = unknown, then row_f_init is read); pt_new_added [n_points] or None; opts: fields of msfm_localize_pose_options.
        Returns a dict: tried, arm, pass, f, R [n][3][3], t [n][3], avg_error, best_step, best_iter, n_inliers, n_outliers per row;
        errors, corr_state per correspondence; n_tried, winner, next_row."""
        n = self.n_kept
        f = A.as_c(np.broadcast_to(np.asarray(row_f, dtype=np.float64), (n,)).copy(), np.float64)
        fi = None if row_f_init is None else A.as_c(np.broadcast_to(np.asarray(row_f_init, dtype=np.float64), (n,)).copy(), np.float64)
        added = None if pt_new_added is None else A.as_c(np.asarray(pt_new_added, dtype=np.uint8).reshape(-1), np.uint8)
        if added is not None:
            if n_points and n_points != len(added):
                raise ValueError("pt_new_added must hold n_points entries")
            n_points = len(added)
        o = localize_pose_options(**opts)
        h = C.c_void_p()
        self.ctx.check(lib().msfm_localize_poses(self.ctx._h, self._h, A.ptr(f, A.c_double_p), A.ptr(fi, A.c_double_p), int(n_points),
                                                 A.ptr(added, A.c_u8_p), C.byref(o), C.byref(h)))
        with _Handle(h, "msfm_localize_pose_set_destroy"):
            nr, nc, ntr, win, nxt = (C.c_int32() for _ in range(5))
            lib().msfm_localize_pose_set_size(h, C.byref(nr), C.byref(nc), C.byref(ntr), C.byref(win), C.byref(nxt))
            nc, m = nc.value, max(1, n)
            tried, arm, pas, state = np.zeros(m, np.uint8), np.zeros(m, np.uint8), np.zeros(m, np.uint8), np.zeros(max(1, nc), np.uint8)
            fo, R, t, avg, err = np.zeros(m), np.zeros((m, 3, 3)), np.zeros((m, 3)), np.zeros(m), np.zeros(max(1, nc))
            bs, bi, nin, nout = (np.zeros(m, np.int32) for _ in range(4))
            dp, ip, up = A.c_double_p, A.c_int_p, A.c_u8_p
            lib().msfm_localize_pose_set_fetch(h, A.ptr(tried, up), A.ptr(arm, up), A.ptr(pas, up), A.ptr(fo, dp), A.ptr(R, dp), A.ptr(t, dp),
                                               A.ptr(avg, dp), A.ptr(bs, ip), A.ptr(bi, ip), A.ptr(nin, ip), A.ptr(nout, ip), A.ptr(err, dp),
                                               A.ptr(state, up))
        return {"tried": tried[:n], "arm": arm[:n], "pass": pas[:n], "f": fo[:n], "R": R[:n], "t": t[:n], "avg_error": avg[:n],
                "best_step": bs[:n], "best_iter": bi[:n], "n_inliers": nin[:n], "n_outliers": nout[:n], "errors": err[:nc],
                "corr_state": state[:nc], "n_tried": ntr.value, "winner": win.value, "next_row": nxt.value}


class BaResident(_Handle):
    """msfm_ba_create / run / upload / download: a BA problem kept in HBM across solves."""
    _destroy = "msfm_ba_destroy"

    def __init__(self, ctx: Context, arrays: A.BaArrays):
        self.ctx, self.arrays = ctx, arrays
        self._h = C.c_void_p()
        ctx.check(lib().msfm_ba_create(ctx._h, C.byref(arrays.struct), C.byref(self._h)))

    def run(self, options=None, capacity=512):
        options = options or default_options()
        buf = A.SummaryBuf(capacity)
        self.ctx.check(lib().msfm_ba_run(self._h, C.byref(options), C.byref(buf.struct)))
        return buf.result()

    def layout(self):
        lay = A.BaLayout()
        self.ctx.check(lib().msfm_ba_get_layout(self._h, C.byref(lay)))
        return dict(reduced_order=lay.reduced_order, system_order=lay.system_order, n_domains=lay.n_domains,
                    domain_cols=list(lay.domain_cols)[:max(0, lay.n_domains if lay.n_domains > 1 else 0)],
                    separator_cols=lay.separator_cols, panel_launches=lay.panel_launches, n_levels=lay.n_levels,
                    level_nodes=list(lay.level_nodes)[:lay.n_levels], level_begin=list(lay.level_begin)[:lay.n_levels], root_cols=lay.root_cols,
                    fold=dict(cc_entries=lay.cc_entries, cc_entries_folded=lay.cc_entries_folded, slots=lay.fold_slots, passes=lay.fold_passes,
                              mc_entries=lay.mc_entries, mc_entries_folded=lay.mc_entries_folded, mc_slots=lay.fold_mc_slots,
                              parts=lay.fold_parts, crit_steps=lay.fold_crit_steps, crit_steps_unsplit=lay.fold_crit_steps_unsplit,
                              wave_steps=lay.fold_wave_steps),
                    solve_paths=lay.solve_paths, assemble_paths=lay.assemble_paths, rider_paths=lay.rider_paths, npb_S=lay.npb_S, npb_L=lay.npb_L, npb_X=lay.npb_X, npb_S4=lay.npb_S4)

    def upload(self, cam_pose=None, cam_model=None, point=None):
        cp, cm, pt = A.as_c(cam_pose, np.float64), A.as_c(cam_model, np.float64), A.as_c(point, np.float64)
        self.ctx.check(lib().msfm_ba_upload_params(self._h, A.ptr(cp, A.c_double_p), A.ptr(cm, A.c_double_p),
                                                   A.ptr(pt, A.c_double_p)))

    def download(self):
        a = self.arrays
        cp, cm, pt = np.zeros_like(a.cam_pose), np.zeros_like(a.cam_model), np.zeros_like(a.point)
        self.ctx.check(lib().msfm_ba_download_params(self._h, A.ptr(cp, A.c_double_p), A.ptr(cm, A.c_double_p),
                                                     A.ptr(pt, A.c_double_p)))
        return cp, cm, pt


class MultiContext(_Handle):
    """msfm_ctx_create_multi: one process, several GPUs - the library owns a context and a host thread per device and the
    communicator between them (ncclCommInitAll over xGMI; an in-process reduction when `devices` names one device several
    times, which is how the path runs on a one-GPU box).  The calls take the whole problem; the split is inside."""
    _destroy = "msfm_multi_destroy"

    def __init__(self, n_gpus, devices=None):
        self._h = C.c_void_p()
        dev = None if devices is None else A.as_c(np.asarray(devices, dtype=np.int32), np.int32)
        rc = lib().msfm_ctx_create_multi(n_gpus, None if dev is None else A.ptr(dev, A.c_int_p), C.byref(self._h))
        if rc != 0:
            raise MsfmError(rc, "msfm_ctx_create_multi failed")
        self.n = lib().msfm_multi_size(self._h)

    def check(self, rc):
        if rc != 0:
            raise MsfmError(rc, lib().msfm_multi_last_error(self._h).decode())

    def ba_solve(self, arrays: A.BaArrays, options=None, capacity=512):
        options = options or default_options()
        buf = A.SummaryBuf(capacity)
        self.check(lib().msfm_multi_ba_solve(self._h, C.byref(arrays.struct), C.byref(options), C.byref(buf.struct)))
        return buf.result()

    def _tri(self, fn, tracks, th_error, th_angle):
        n = tracks.struct.n_tracks
        X, mse, ok = np.zeros((n, 3)), np.zeros(n), np.zeros(n, dtype=np.uint8)
        self.check(fn(self._h, C.byref(tracks.struct), th_error, th_angle, A.ptr(X, A.c_double_p), A.ptr(mse, A.c_double_p), A.ptr(ok, A.c_u8_p)))
        return X, mse, ok

    def triangulate_midpoint(self, tracks, th_error, th_angle):
        return self._tri(lib().msfm_multi_triangulate_midpoint_batch, tracks, th_error, th_angle)

    def triangulate_dlt(self, tracks, th_error, th_angle):
        return self._tri(lib().msfm_multi_triangulate_dlt_batch, tracks, th_error, th_angle)

    def reproject_mse(self, tracks, X):
        X = A.as_c(X, np.float64)
        mse = np.zeros(tracks.struct.n_tracks)
        self.check(lib().msfm_multi_reproject_mse_batch(self._h, C.byref(tracks.struct), A.ptr(X, A.c_double_p), A.ptr(mse, A.c_double_p)))
        return mse

    def match_pairs(self, descs, pairs, ratio_good=0.6, ratio_all=0.85):
        """codes per pair, n_all, n_good - what DescSet.match_pairs + fetch give, with the pair list split over the contexts."""
        descs = [A.as_c(d, np.float32) for d in descs]
        pairs = A.as_c(np.asarray(pairs, dtype=np.int32).reshape(-1, 2), np.int32)
        count = np.array([len(d) for d in descs], dtype=np.int32)
        dp = (A.c_float_p * len(descs))(*[A.ptr(d, A.c_float_p) if len(d) else None for d in descs])
        codes = [np.zeros(max(1, int(count[j])), np.int32) for _, j in pairs]
        cp = (A.c_int_p * max(1, len(pairs)))(*[A.ptr(c, A.c_int_p) for c in codes])
        na, ng = np.zeros(max(1, len(pairs)), np.int32), np.zeros(max(1, len(pairs)), np.int32)
        self.check(lib().msfm_multi_match_pairs(self._h, len(descs), dp, A.ptr(count, A.c_int_p), 128, A.ptr(pairs, A.c_int_p), len(pairs),
                                                ratio_good, ratio_all, cp, A.ptr(na, A.c_int_p), A.ptr(ng, A.c_int_p)))
        return [c[:count[j]] for c, (_, j) in zip(codes, pairs)], na[:len(pairs)], ng[:len(pairs)]


def camera_graph_dissection(adjacency, tail_cols=4, force_depth=-1):
    """msfm_camera_graph_dissection (host only: works without a GPU): labels per camera (leaf id, or -(d + 1) for a separator cut
    at depth d), number of leaves (0: dense order kept) and the critical path in 64-column panel steps."""
    adj = np.ascontiguousarray(adjacency, dtype=np.uint8)
    n = adj.shape[0]
    assert adj.shape == (n, n)
    label = np.zeros(n, np.int32)
    nl, steps = C.c_int(0), C.c_int(0)
    rc = lib().msfm_camera_graph_dissection(n, A.ptr(adj, A.c_u8_p), int(tail_cols), int(force_depth), A.ptr(label, A.c_int_p), C.byref(nl),
                                            C.byref(steps))
    if rc != 0:
        raise MsfmError(rc, "msfm_camera_graph_dissection")
    return label, nl.value, steps.value
