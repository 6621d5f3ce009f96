"""Dense stereo on the device: DenseReconstruction::SGMDense (SfM/src/dense_reconstruction.cc:113-190) on rectified pairs through
msfm_sgm_create / msfm_sgm_execute / msfm_sgm_depth (include/msfm.h, "Dense stereo", states the definitions), the pose file it
starts from, and the poses of the rectified images it ends with.

The rectification itself (EpipolarRectification: OpenCV's stereoRectify + remap) is not built: the caller supplies the
rectified pairs and the rotations the rectification applied."""
import numpy as np

from . import capi


def read_pose_file(path):
    """DenseReconstruction::ReadinPoseFile (dense_reconstruction.cc:70-111): eight header lines, then per image its name, w, h, K
    (3 x 3, row-major), five distortion values (k1 k2 k3 p1 p2), t (3) and R (3 x 3, row-major), separated by white space.
    -> dict(names, sizes [n][2] (w, h), Ks [n][3][3], dist [n][5], ts [n][3], Rs [n][3][3]).  Only complete records are
    returned (the reference's `while (!ff.eof())` appends one more, unread, record after trailing white space)."""
    with open(path) as fh:
        tok = "".join(fh.readlines()[8:]).split()
    per = 1 + 2 + 9 + 5 + 3 + 9
    n = len(tok) // per
    names, rows = [], np.zeros((n, per - 1), np.float64)
    for i in range(n):
        rec = tok[i * per:(i + 1) * per]
        names.append(rec[0])
        rows[i] = [float(v) for v in rec[1:]]
    return dict(names=names, sizes=rows[:, 0:2].astype(np.int32), Ks=rows[:, 2:11].reshape(n, 3, 3).copy(), dist=rows[:, 11:16].copy(),
                ts=rows[:, 16:19].copy(), Rs=rows[:, 19:28].reshape(n, 3, 3).copy())


def sgm_dense(ctx: capi.Context, pairs, Ks, ts, disp_size=128, p1=10, p2=120, uniqueness=0.96):
    """The loop of SGMDense over consecutive images: pairs[i] = (left, right), the rectified images i + 1 and i (uint8 [h][w], all
    of one size), on one `StereoSGM` that every pair reuses.  -> [(disparity uint8 [h][w], depth uint8 [h][w])] per pair, with
    baseline = |ts[i + 1] - ts[i]| and focal = Ks[i + 1][0, 0] (dense_reconstruction.cc:161-162)."""
    pairs = list(pairs)
    if not pairs:
        return []
    Ks, ts = np.asarray(Ks, np.float64), np.asarray(ts, np.float64).reshape(-1, 3)
    if len(Ks) < len(pairs) + 1 or len(ts) < len(pairs) + 1:
        raise ValueError("%d pairs need the K and t of %d images" % (len(pairs), len(pairs) + 1))
    h, w = np.asarray(pairs[0][0]).shape
    out = []
    with ctx.stereo_sgm(w, h, disp_size, p1, p2, uniqueness) as sgm:
        for i, (left, right) in enumerate(pairs):
            sgm.execute(left, right)
            baseline = float(np.sqrt(((ts[i + 1] - ts[i]) ** 2).sum()))
            out.append((sgm.disparity(), sgm.depth(baseline, float(Ks[i + 1][0, 0]))))
    return out


def epipolar_poses(Rs, ts, R_left):
    """The poses of the rectified left images (dense_reconstruction.cc:186-188): for pair i, whose left image is i + 1 and whose
    rectification rotated it by R_left[i]:  R_new = Rs[i + 1] R_left[i], c = -Rs[i + 1]^-1 ts[i + 1], t_new = -R_new c.
    -> (Rs_new [n][3][3], ts_new [n][3]); image 0 is never a left image and keeps zeros (the reference leaves an empty matrix there)."""
    Rs, ts = np.asarray(Rs, np.float64), np.asarray(ts, np.float64).reshape(-1, 3)
    Rn, tn = np.zeros_like(Rs), np.zeros_like(ts)
    for i, Rl in enumerate(R_left):
        Rn[i + 1] = Rs[i + 1] @ np.asarray(Rl, np.float64)
        c = -np.linalg.inv(Rs[i + 1]) @ ts[i + 1]
        tn[i + 1] = -Rn[i + 1] @ c
    return Rn, tn
