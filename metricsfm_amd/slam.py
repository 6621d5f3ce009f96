"""The SLAM + GPS path from descriptors to the adjusted, registered model on one resident chain: SLAMGPS::FeatureMatching
(SfM/src/slam_gps.cc:312-555) as a whole, and SLAMGPS::Run (:98-119) behind it."""
import os

import numpy as np

from . import capi, gpsreg, matchfiles

TH_FIRST_SECOND_RATIO = 0.80          # slam_gps.cc:320


def thresholds(resize_ratio):
    """`float th_epipolar = 2.0 / resize_ratio; float th_distance = 5.0 / resize_ratio;` (slam_gps.cc:316-317): the quotient in
    binary64, the local in binary32."""
    return float(np.float32(2.0 / float(resize_ratio))), float(np.float32(5.0 / float(resize_ratio)))


def match_graph(n_cams, pairs, n_matches):
    """match_graph[id1][id2] = matches[j].size() (slam_gps.cc:540), dense [n][n], zero where no pair was matched."""
    g = np.zeros((int(n_cams), int(n_cams)), dtype=np.int32)
    for (i, j), n in zip(np.asarray(pairs).reshape(-1, 2), n_matches):
        g[int(i), int(j)] = int(n)
    return g


def feature_matching(ctx, ds, n_cams, track_off, track_cam, track_xy, resize_ratio=0.5, fold=None, **opts):
    """SLAMGPS::FeatureMatching on a descriptor set that holds the keypoints of its images:

        step 1 (:323-423)   ctx.slam_priors on the SLAM points (CSR tracks track_off / track_cam / track_xy of n_cams cameras)
        step 2 (:455-503)   ds.match_pairs_slam with the kept pairs and their prior F / H, the same thresholds, ratio 0.80
               (:503-541)   Chain(res).verify_slam(**opts): GeoVerificationFundamental on all survivors of a pair, the pair
                            keeps the entries of the mask whatever the verdict (include/msfm.h has the three conventions)

    `opts` are the options of msfm_fundamental_ransac_batch (seed, threshold, ...).  Returns (chain, res, record); the record
    holds pairs, F_prior, H_prior, candidates (the rows of msfm_slam_priors), n_survivors (of the three checks), n_matches,
    ok, F and the dense match_graph [n_cams][n_cams] (:540).  The caller closes the chain and the result.

    With `fold` the files of the reference are written there through matchfiles: prior.txt (WriteOutPriorInfo), the
    <i>_match files (WriteOutMatches appends a record per pair with matches) and graph_matching.txt (WriteOutMatchGraph).
    This is the only place where matches are fetched from the device."""
    th_e, th_d = thresholds(resize_ratio)
    pairs, Fp, Hp, cand = ctx.slam_priors(n_cams, track_off, track_cam, track_xy, th_epipolar=th_e, th_distance=th_d)
    res = ds.match_pairs_slam(pairs, Fp, Hp, th_first_second_ratio=TH_FIRST_SECOND_RATIO, th_epipolar=th_e, th_distance=th_d)
    chain = None
    try:
        chain = capi.Chain(res)
        n_surv, _ = res.counts()
        n_m, ok, F = chain.verify_slam(**opts)
        rec = dict(pairs=pairs, F_prior=Fp, H_prior=Hp, candidates=cand, n_survivors=n_surv, n_matches=n_m, ok=ok, F=F,
                   match_graph=match_graph(n_cams, pairs, n_m))
        if fold is not None:
            os.makedirs(fold, exist_ok=True)
            matchfiles.write_prior_info(os.path.join(fold, "prior.txt"), n_cams, pairs, Fp, Hp)
            for p, (i, j) in enumerate(pairs):
                if n_m[p]:
                    matchfiles.write_out_matches(fold, int(i), int(j), chain.fetch_matches(p))
            matchfiles.write_out_match_graph(fold, rec["match_graph"])
    except Exception:
        if chain is not None:
            chain.close()
        res.close()
        raise
    return chain, res, rec


def slam_gps_run(ctx, ds, n_cams, track_off, track_cam, track_xy, cam_R, cam_c, cam_model, cam_model_of_cam, gps, resize_ratio=0.5, fold=None,
                 fransac=None, **register):
    """SLAMGPS::Run (slam_gps.cc:98-119) with the `if (0)` of :103 taken, which is how the input of Triangulation comes to
    exist: feature_matching, the data association of Triangulation (chain.build_tracks, pairs in (i, j) order as :566-583
    walks match_graph_ > 0), then gpsreg.slam_gps_register on the same chain.  `fransac`: options of the verification,
    `register`: keyword arguments of slam_gps_register.  Returns (chain, res, matching record, registration record)."""
    chain, res, rec = feature_matching(ctx, ds, n_cams, track_off, track_cam, track_xy, resize_ratio=resize_ratio, fold=fold, **(fransac or {}))
    try:
        rec["n_tracks"], rec["n_obs"] = chain.build_tracks()
        reg = gpsreg.slam_gps_register(chain, cam_R, cam_c, cam_model, cam_model_of_cam, gps, **register)
    except Exception:
        chain.close(); res.close()
        raise
    return chain, res, rec, reg
