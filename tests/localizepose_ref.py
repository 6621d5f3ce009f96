"""The try loop of IncrementalSfM::Run (sfm_incremental.cc:143-164) around IncrementalSfM::LocalizeImage (:565-729) restated as
the literal sequential walk, on the output of tests/localize_ref.localize_ref (or of `Context.localize_candidates`, the same
dict).  The yardstick of tests/test_gpu_localizepose.py; its own rules are pinned by tests/test_localizepose_ref.py.

The two pose solvers are arguments, so the rules can be pinned on hand-made error arrays; `oracle_solvers` gives the real ones:
oracle.epnp_ransac and tests/epnpf_ref.epnpf_sweep with the row handed in as problem r behind r empty problems, which is how
msfm_localize_poses numbers its samples.

Unlike the reference's loop the walk does not stop at the first success: every tried row is reported (a failed try changes
nothing but localize_fail_times_, :650 / :681, so later rows do not depend on earlier ones), and `winner` is where the
reference would have stopped."""
import numpy as np

from tests import epnpf_ref

DEFAULTS = dict(th_mse_localization=5.0, th_min_2d3d_corres=20, max_iter=200, seed=0x4D53464D50,
                sweep=dict(f_ratio_min=0.5, f_ratio_max=4.0, f_ratio_step=0.01, max_iter=200, seed=0x4D53464D50), first_row=0, max_tries=16)


def oracle_solvers(O, max_iter=200, seed=0x4D53464D50, sweep=None):
    """(known, swept): known(r, X, x, f) -> (R, t, errors, avg, best_iter); swept(r, X, x, f_init) -> (f, R, t, errors, avg,
    best_step, best_iter)."""
    sw = dict(DEFAULTS["sweep"], **(sweep or {}))

    def known(r, X, x, f):
        off = np.array([0] * (r + 1) + [len(X)], np.int32)
        R, t, e, avg, it = O.epnp_ransac(off, X, x, np.concatenate([np.ones(r), [f]]), max_iter=max_iter, seed=seed)
        return R[r], t[r], e, avg[r], it[r]

    def swept(r, X, x, f_init):
        off = np.array([0] * (r + 1) + [len(X)], np.int32)
        f, R, t, e, avg, bs, bi, _ = epnpf_ref.epnpf_sweep(O, off, X, x, np.concatenate([np.ones(r), [f_init]]), **sw)
        return f[r], R[r], t[r], e, avg[r], bs[r], bi[r]

    return known, swept


def localize_poses_ref(loc, row_f, row_f_init, n_points, pt_new_added, known, swept, th_mse_localization=5.0, th_min_2d3d_corres=20,
                       first_row=0, max_tries=16):
    """Returns the dict of `LocalizeSet.poses`."""
    off = np.asarray(loc["corr_off"])
    n, T = len(off) - 1, int(off[-1])
    out = dict(tried=np.zeros(n, np.uint8), arm=np.zeros(n, np.uint8), f=np.zeros(n), R=np.zeros((n, 3, 3)), t=np.zeros((n, 3)),
               avg_error=np.zeros(n), best_step=np.zeros(n, np.int32), best_iter=np.zeros(n, np.int32), n_inliers=np.zeros(n, np.int32),
               n_outliers=np.zeros(n, np.int32), errors=np.zeros(T), corr_state=np.zeros(T, np.uint8))
    out["pass"] = np.zeros(n, np.uint8)
    row_f = np.broadcast_to(np.asarray(row_f, np.float64), (n,))
    winner, next_row, n_tried = -1, -1, 0
    for r in range(n):                                                            # :146
        b, e = int(off[r]), int(off[r + 1])
        if e - b < th_min_2d3d_corres or e - b < 3:                               # :148, :567
            continue
        if r < first_row:
            continue
        if max_tries and n_tried == max_tries:
            next_row = r
            break
        n_tried += 1
        out["tried"][r] = 1
        X, x = loc["pts_w"][b:e], loc["pts_2d"][b:e]
        if row_f[r] != 0.0:                                                       # :644
            out["arm"][r] = 1
            R, t, err, avg, it = known(r, X, x, float(row_f[r]))
            f, step = float(row_f[r]), -1
        else:
            out["arm"][r] = 2
            f, R, t, err, avg, step, it = swept(r, X, x, float(np.broadcast_to(row_f_init, (n,))[r]))   # :675-677, :703
        out["f"][r], out["R"][r], out["t"][r], out["avg_error"][r], out["best_step"][r], out["best_iter"][r] = f, R, t, avg, step, it
        out["errors"][b:e] = err
        if avg > th_mse_localization:                                             # :648 / :679 (a NaN goes on)
            continue
        out["pass"][r] = 1
        if winner < 0:
            winner = r
        added = np.zeros(n_points, bool) if pt_new_added is None else np.array(pt_new_added, dtype=bool)   # is_new_added_, a copy per row
        for i in range(b, e):                                                     # :709
            p = int(loc["corr_point"][i])
            if err[i - b] > avg:                                                  # :713
                out["corr_state"][i] = 1                                          # is_bad_estimated_ = true
                out["n_outliers"][r] += 1
            elif not added[p]:                                                    # :721
                added[p] = True
                out["corr_state"][i] = 2
                out["n_inliers"][r] += 1                                          # :727
            else:
                out["corr_state"][i] = 3
    out.update(n_tried=n_tried, winner=winner, next_row=next_row)
    return out
