"""Dense stereo on the device: DenseReconstruction::SGMDense (SfM/src/dense_reconstruction.cc:113-190) from posed images - the
pose file it starts from, EpipolarRectification per pair (msfm_rectifier_rectify), the matching on the rectified planes where
the rectifier left them (msfm_sgm_execute_rectified), the depth image, and the poses of the rectified images it ends with, back
into a pose file.  include/msfm.h, "Stereo rectification" and "Dense stereo", states the definitions.

`sgm_dense_posed` is that loop with the reference's inputs.  `sgm_dense` remains for pairs that were rectified elsewhere.
The rectification is by this project's own definitions: parity with OpenCV's stereoRectify / remap is unpinned, there are no
distortion coefficients (the reference passes zeros) and the input is one grey plane; ELASDense and Depth2Points are not built."""
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


def write_pose_file(path, names, sizes, Ks, ts, Rs):
    """DenseReconstruction::SavePoseFile (dense_reconstruction.cc:333-362) as the file `read_pose_file` reads: the seven header
    lines and the empty one, then per image its name, w, h, K without skew, five zero distortion values, t and R at 8 decimals.
    The reference's fprintf hands a std::string to %s and integer zeros to %lf (:349-354), which prints garbage; this writes what
    it evidently meant.  It also starts at image 1 (image 0 is never a left image and has no new pose): pass the records to write."""
    Ks, ts, Rs = np.asarray(Ks, np.float64), np.asarray(ts, np.float64).reshape(-1, 3), np.asarray(Rs, np.float64)
    with open(path, "w") as fh:
        for line in ("fileName imageWidth imageHeight", "camera matrix K [3x3]", "radial distortion [3x1]", "tangential distortion [2x1]",
                     "camera position t [3x1]", "camera rotation R [3x3]", "camera model P = K [R|-Rt] X"):
            fh.write(line + "\n")
        fh.write("\n")
        for name, (w, h), K, t, R in zip(names, sizes, Ks, ts, Rs):
            fh.write("%s %d %d\n" % (name, w, h))
            fh.write("%.8f %.8f %.8f\n" % (K[0, 0], 0, K[0, 2]))
            fh.write("%.8f %.8f %.8f\n" % (0, K[1, 1], K[1, 2]))
            fh.write("0 0 1\n")
            fh.write("%.8f %.8f %.8f\n" % (0, 0, 0))
            fh.write("%.8f %.8f\n" % (0, 0))
            fh.write("%.8f %.8f %.8f\n" % tuple(t))
            for row in R:
                fh.write("%.8f %.8f %.8f\n" % tuple(row))


def epipolar_rectification(rect: capi.Rectifier, left, K1, R1, t1, right, K2, R2, t2, keep_maps=False):
    """DenseReconstruction::EpipolarRectification (dense_reconstruction.cc:299-331) on a resident rectifier, with the reference's
    argument order: camera 1 is `left`.  The rectified pair stays on the device (`rect.fetch(0)`, `rect.fetch(1)`,
    `StereoSGM.execute_rectified(rect)`).  -> (R_left, R_right, the whole dict of `Rectifier.rectify`)."""
    out = rect.rectify(left, right, K1, R1, t1, K2, R2, t2, keep_maps=keep_maps)
    return out["R_left"], out["R_right"], out


def sgm_dense_posed(ctx: capi.Context, images, Ks, Rs, ts, disp_size=128, p1=10, p2=120, uniqueness=0.96):
    """The loop of SGMDense (dense_reconstruction.cc:123-189) from unrectified images (uint8 [h][w], all of one size) and their
    poses: pair i has the left image i + 1 and the right image i.  Per pair: rectify, match on the rectified planes device to
    device, depth with baseline = |ts[i + 1] - ts[i]| and focal = Ks[i + 1][0, 0] (:161-162, as the reference has it), and the new
    pose of the left image (`epipolar_poses`).  One `Rectifier` and one `StereoSGM` serve every pair.
    -> dict(disparity, depth: per pair uint8 [h][w]; R_left, R_right: per pair [3][3]; P_right_sign: per pair the sign of
    P_right[0][3] - positive means camera i + 1 was not the left one and the matching saw only negative disparities, which the
    reference does not notice either; Rs_new [n][3][3], ts_new [n][3])."""
    images = list(images)
    Ks, Rs = np.asarray(Ks, np.float64), np.asarray(Rs, np.float64)
    ts = np.asarray(ts, np.float64).reshape(-1, 3)
    n = len(images)
    if len(Ks) < n or len(Rs) < n or len(ts) < n:
        raise ValueError("%d images need %d K, R and t" % (n, n))
    out = dict(disparity=[], depth=[], R_left=[], R_right=[], P_right_sign=[])
    if n >= 2:
        h, w = np.asarray(images[0]).shape
        with ctx.rectifier(w, h) as rect, ctx.stereo_sgm(w, h, disp_size, p1, p2, uniqueness) as sgm:
            for i in range(n - 1):
                Rl, Rr, g = epipolar_rectification(rect, images[i + 1], Ks[i + 1], Rs[i + 1], ts[i + 1], images[i], Ks[i], Rs[i], ts[i])
                sgm.execute_rectified(rect)
                baseline = float(np.sqrt(((ts[i + 1] - ts[i]) ** 2).sum()))
                out["disparity"].append(sgm.disparity())
                out["depth"].append(sgm.depth(baseline, float(Ks[i + 1][0, 0])))
                out["R_left"].append(Rl)
                out["R_right"].append(Rr)
                out["P_right_sign"].append(int(np.sign(g["P_right"][0, 3])))
    out["Rs_new"], out["ts_new"] = epipolar_poses(Rs[:n], ts[:n], out["R_left"])
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
