/*
 * msfm.h — C ABI of the MI355X-native bundle-adjustment + feature-matching core.
 *
 * Every entry point replaces one inline third-party call (or one short loop) of the
 * reference's SfM/src hot path; the reference file:line each one stands in for is cited
 * on the declaration.  Plain pointers and sizes only: no C++ types, no torch types.
 *
 * Conventions
 *   - All buffers are caller-owned HOST memory unless the name ends in `_dev`.
 *     The library never retains a host pointer past return.
 *   - Return value: MSFM_OK (0) or a negative MSFM_E_* code; msfm_last_error(ctx)
 *     gives the text.  No C++ exception crosses this boundary.
 *   - One msfm_ctx per GPU (one process per GPU).  A ctx is not re-entrant; the
 *     reference's OpenMP-parallel kNN loop (fine_matching_graph.cc:87-100) is hoisted
 *     into the one batched call msfm_match_pairs().
 *   - Bundle adjustment arithmetic is IEEE binary64 throughout; matching takes
 *     binary32 descriptors as the reference does (database.cc:412-418).
 */
#ifndef MSFM_H_
#define MSFM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSFM_VERSION 100 /* 0.1.0 */

/* ---- error codes ------------------------------------------------------------------ */
#define MSFM_OK 0
#define MSFM_E_INVAL (-1)   /* bad argument / inconsistent sizes                         */
#define MSFM_E_NOMEM (-2)   /* host or device allocation failed                          */
#define MSFM_E_DEVICE (-3)  /* HIP runtime error (no GPU, launch failure, ...)           */
#define MSFM_E_NUMERIC (-4) /* unrecoverable numeric failure (Ceres: FAILURE)            */

typedef struct msfm_ctx msfm_ctx;

int msfm_version(void);
/* device < 0: use the current HIP device.  Fails with MSFM_E_DEVICE when no GPU is
 * visible — there is no CPU fallback behind this ABI. */
int msfm_ctx_create(int device, msfm_ctx** out);
/* Every object made from a ctx that keeps it is a child of that context: descriptor sets, match results, chains, resident BA
 * problems, word sets, vocabulary trees, word results, scale spaces, stereo objects, match stores, seed / localize / round
 * sets and resident states.  Children should be destroyed first; if some are still alive the context is kept until the last
 * of them is destroyed, then released.  A create that fails leaves no child behind.
 * The msfm_*_destroy of a child accepts NULL, sets the context's device itself and, where the object holds device memory,
 * waits for the context's stream before that memory is given back: always, except msfm_seed_set_destroy and
 * msfm_localize_set_destroy (only for a set that kept arrays on the device) and msfm_round_set_destroy (host memory only,
 * never).  The host-only results - track, pair, new-points and localize-pose sets - belong to no context. */
void msfm_ctx_destroy(msfm_ctx* ctx);
const char* msfm_last_error(const msfm_ctx* ctx);
/* The HIP stream (hipStream_t) every kernel of this ctx is launched on. */
void* msfm_ctx_stream(msfm_ctx* ctx);
int msfm_ctx_synchronize(msfm_ctx* ctx);

/* Per-kernel-class device time accumulated with HIP events on the ctx stream since the
 * last reset (used by bench.py for the live roofline figure).  Off by default. */
#define MSFM_MAX_KERNEL_STATS 32
typedef struct msfm_kernel_stat {
  char name[48];
  uint64_t launches;
  double total_ms;
} msfm_kernel_stat;
int msfm_ctx_profile_enable(msfm_ctx* ctx, int enable);
int msfm_ctx_profile_reset(msfm_ctx* ctx);
int msfm_ctx_profile_get(msfm_ctx* ctx, msfm_kernel_stat* stats, int cap, int* n_out);

/* ==================================================================================== *
 *  Matching  
 * ==================================================================================== */

/* Exact 2-nearest-neighbour search, squared L2, of every query descriptor among the
 * train descriptors.  Replaces the FLANN pair
 *     flann_build_index(...)                   SfM/src/graph/fine_matching_graph.cc:72-81
 *     flann_find_nearest_neighbors_index(...)  SfM/src/graph/fine_matching_graph.cc:99
 * (twin call site SfM/src/slam_gps.cc:438-447,463) and fills the same two arrays FLANN
 * fills (`knn_id[j]`, `knn_dis[j]`, fine_matching_graph.cc:96-99):
 *     ids     [n_query][2]  index into train, nearest first
 *     sqdists [n_query][2]  squared L2 distance, ascending
 * Unlike the kd-tree (8 trees, 64 checks — approximate) the result is the exact 2-NN;
 * equal distances are ordered by lower train index.  n_train >= 2 is required (the
 * reference divides dists[0]/dists[1]).  dim must be 128 (SIFT; database.cc:412-418 stores 128 columns): the
 * kernels are specialised for it and every other value is refused with MSFM_E_INVAL.
 */
int msfm_knn2_f32(msfm_ctx* ctx, const float* train, int n_train, const float* query, int n_query,
                  int dim, int* ids, float* sqdists);

/* Device-resident descriptor store: one entry per image, uploaded once and reused by
 * every pair that touches the image (the reference re-reads `<idx2>_feature` from disk
 * per pair, fine_matching_graph.cc:91). */
typedef struct msfm_descset msfm_descset;
int msfm_descset_create(msfm_ctx* ctx, int n_images, int dim /* 128 */, msfm_descset** out);
/* Replaces the image's descriptors.  Waits for work already enqueued on the ctx stream (a running match may still read
 * the old buffers).  Match results created before the upload become stale: msfm_match_pairs_rerun /
 * msfm_match_result_fetch on them return MSFM_E_INVAL; create a new result with msfm_match_pairs. */
int msfm_descset_upload(msfm_descset* set, int image, const float* desc, int count);
int msfm_descset_count(const msfm_descset* set, int image);
/* Ordering rule: a set may be destroyed before its match results.  The results then keep what they own - counts, codes
 * and (with keep_knn) the 2-NN arrays stay readable through msfm_match_result_counts / _fetch / _stats - while
 * msfm_match_pairs_rerun on them returns MSFM_E_INVAL; they are released by msfm_match_result_destroy as usual. */
void msfm_descset_destroy(msfm_descset* set);

/* Batched pair matching with the ratio tests fused in
 * (fine_matching_graph.cc:87-133; the SLAM variant slam_gps.cc:469-503 is msfm_match_pairs_slam below).
 * pairs[p] = {idx1 (train image), idx2 (query image)}.
 * For pair p and query feature m of image idx2 (in feature order, which is the order of
 * the reference loop fine_matching_graph.cc:116-133):
 *     ratio = sqdist0 / sqdist1
 *     good  = ratio < ratio_good,  all = ratio < ratio_all       (two independent tests, :118-130)
 *     code  = -1                                                  if neither
 *           = id0 | (good ? MSFM_MATCH_GOOD : 0) | (all ? 0 : MSFM_MATCH_NOT_ALL)   otherwise
 * With the reference's thresholds (0.6 < 0.85) a good match is always in the "all" set and MSFM_MATCH_NOT_ALL never
 * appears; id0 = code & MSFM_MATCH_ID_MASK.
 * The codes live in device memory inside the result object; fetch copies one pair to
 * the host.  n_all / n_good are the sizes of the reference's matches_all / matches_good.
 */
#define MSFM_MATCH_GOOD 0x40000000
#define MSFM_MATCH_NOT_ALL 0x20000000
#define MSFM_MATCH_ID_MASK 0x1FFFFFFF
typedef struct msfm_match_result msfm_match_result;
int msfm_match_pairs(msfm_descset* set, const int* pairs /*[n_pairs][2]*/, int n_pairs,
                     float ratio_good, float ratio_all, int keep_knn, msfm_match_result** out);
int msfm_match_result_counts(msfm_match_result* res, int* n_all /*[n_pairs]*/,
                             int* n_good /*[n_pairs]*/);
/* code[count(idx2)]; ids/sqdists may be NULL, and are only available with keep_knn. */
int msfm_match_result_fetch(msfm_match_result* res, int pair, int32_t* code, int* ids,
                            float* sqdists);
/* Non-integral descriptors go through an approximate shortlist + exact re-rank; queries whose
 * shortlist could not be certified are redone by exact brute force.  n_slow_path counts them
 * (0 for integer-valued data, which takes the exact int8 kernel). */
int msfm_match_result_stats(msfm_match_result* res, int* n_queries, int* n_slow_path);
void msfm_match_result_destroy(msfm_match_result* res);
/* Re-run the same pair list into an existing result object (steady-state bench loop:
 * no allocation, no host transfer). */
int msfm_match_pairs_rerun(msfm_descset* set, msfm_match_result* res);

/* Keypoint positions of an image's features, [count][2] float as cv::Point2f (`db_.keypoints_[id]->pts[k].pt`), resident
 * beside its descriptors; `count` must equal the image's descriptor count.  Needed by msfm_match_pairs_slam; uploading the
 * descriptors of the image again drops them. */
int msfm_descset_upload_keypoints(msfm_descset* set, int image, const float* xy, int count);

/* The matching loop of SLAMGPS::FeatureMatching step 2 (SfM/src/slam_gps.cc:455-503), batched over image pairs, in place of
 * flann_find_nearest_neighbors_index (:463) and the three checks behind it.  For pair p = {id1 (train), id2 (query)} with
 * its prior F = Fs[i][j] and H = Hs[i][j] (row-major [9], as cv::Mat_<double>(3,3)) and query feature m:
 *     check1 (:469-475)  ratio = sqdist0 / sqdist1;  rejected if ratio > th_first_second_ratio
 *                        (`>`: a ratio equal to the threshold, or 0/0 from duplicate descriptors, passes - unlike the
 *                        `ratio < th` tests of fine_matching_graph.cc:118-130 behind msfm_match_pairs)
 *     check2 (:478-488)  l = F [x1 y1 1]^T, rejected if |l . [x2 y2 1]| / sqrt(l0^2 + l1^2) > th_epipolar
 *     check3 (:490-499)  q = H [x1 y1 1]^T / q2, rejected if |[x2 y2] - q| > 40 * th_distance
 * with (x1, y1) the position of train feature id0 and (x2, y2) of query feature m, binary64 arithmetic as cv::Mat does it.
 *     code = id0 (no flag bits) for a match that passes all three, -1 otherwise   -> matches[j] = (code, m) in m order (:503)
 *     n_good[p] = survivors of check1,  n_all[p] = survivors of all three (= matches[j].size() before :509)
 * The survivors then go to msfm_fundamental_ransac_batch (GeoVerificationFundamental, :509). */
typedef struct msfm_slam_match_options {
  float th_first_second_ratio; /* 0.80               (slam_gps.cc:320) */
  float th_epipolar;           /* 2.0 / resize_ratio (slam_gps.cc:316) */
  float th_distance;           /* 5.0 / resize_ratio (slam_gps.cc:317) */
} msfm_slam_match_options;
void msfm_slam_match_default_options(msfm_slam_match_options* opt);
int msfm_match_pairs_slam(msfm_descset* set, const int* pairs /*[n_pairs][2]*/, int n_pairs,
                          const double* F /*[n_pairs][9]*/, const double* H /*[n_pairs][9]*/,
                          const msfm_slam_match_options* opt, int keep_knn, msfm_match_result** out);

/* ==================================================================================== *
 *  Bundle adjustment  
 * ==================================================================================== */

/* The problem BundleAdjuster::RunOptimizetion assembles (SfM/src/optimizer.cc:59-129)
 * gathered into flat arrays.  Gather order = point index ascending, then std::map key
 * order of the point's observations (optimizer.cc:62,80-82); bad points
 * (is_bad_estimated_, :64) are simply not gathered.
 *
 * Which reference functor an observation becomes follows optimizer.cc:86-125:
 *   pt_mutable & cam_mutable & model_mutable -> ReprojectionErrorPoseCamXYZ (2;6,3,3)
 *   pt_mutable & cam_mutable & !model_mutable-> ReprojectionErrorPoseXYZ    (2;6,3)
 *   pt_mutable & !cam_mutable                -> ReprojectionErrorXYZ        (2;3)
 *   !pt_mutable & cam_mutable & model_mutable-> ReprojectionErrorPoseCam    (2;6,3)
 *   !pt_mutable & cam_mutable & !model_mut.  -> ReprojectionErrorPose       (2;6)
 *   !pt_mutable & !cam_mutable               -> no residual
 */
typedef struct msfm_ba_problem {
  int n_cams, n_models, n_points, n_obs;
  double* cam_pose;            /* [n_cams][6] angle-axis, t (camera.cc:89-99)      in/out */
  double* cam_model;           /* [n_models][3] f, k1, k2 (basic_structs.h:83-90)  in/out */
  const int32_t* cam_model_of_cam; /* [n_cams]                                            */
  double* point;               /* [n_points][3] (structure.h:64)                   in/out */
  const int32_t* obs_cam;      /* [n_obs]                                                 */
  const int32_t* obs_pt;       /* [n_obs] non-decreasing                                  */
  const double* obs_xy;        /* [n_obs][2] centred pixels (database.cc:522-527)         */
  const double* pt_weight;     /* [n_points] residual weight (optimizer.cc:69-78)         */
  const uint8_t* cam_mutable;  /* [n_cams]   NULL = all mutable                           */
  const uint8_t* model_mutable;/* [n_models] NULL = all mutable (basic_structs.h:64)      */
  const uint8_t* pt_mutable;   /* [n_points] NULL = all mutable                           */
  /* Absolute GPS residual per camera (gps_error_pose_absolute.h:31-44, wiring
   * slam_gps.cc:818-830): r = [w|tx-x|, w|ty-y|, (w/5)|tz-z|] on pose[3:6], Huber(1).
   * NULL = none.  */
  const double* gps_xyz;       /* [n_cams][3] */
  double gps_weight;
} msfm_ba_problem;

/* Only the fields the reference sets (optimizer.cc:42-48; slam_gps.cc:681-684) plus the
 * Ceres 1.13 defaults it inherits, spelled out so that tests can vary them.
 * msfm_ba_options_default() fills the Ceres defaults. */
typedef struct msfm_ba_options {
  int max_num_iterations;        /* 200 (basic_structs.h:232); 100 in test_sfm.cc:35-36   */
  int num_threads;               /* passed through; the GPU path ignores it               */
  int progress_to_stdout;        /* minimizer_progress_to_stdout                          */
  double huber_delta;            /* 1.0 (optimizer.cc:84)                                 */
  double function_tolerance;     /* 1e-6                                                  */
  double gradient_tolerance;     /* 1e-10                                                 */
  double parameter_tolerance;    /* 1e-8                                                  */
  double initial_trust_region_radius; /* 1e4                                              */
  double max_trust_region_radius;     /* 1e16                                             */
  double min_trust_region_radius;     /* 1e-32                                            */
  double min_relative_decrease;       /* 1e-3                                             */
  double min_lm_diagonal;             /* 1e-6                                             */
  double max_lm_diagonal;             /* 1e32                                             */
  int max_num_consecutive_invalid_steps; /* 5                                             */
  int jacobi_scaling;                 /* 1                                                */
} msfm_ba_options;
void msfm_ba_options_default(msfm_ba_options* opt);

/* Termination (ceres::TerminationType + which test fired). */
#define MSFM_BA_CONVERGENCE_FUNCTION 1
#define MSFM_BA_CONVERGENCE_GRADIENT 2
#define MSFM_BA_CONVERGENCE_PARAMETER 3
#define MSFM_BA_NO_CONVERGENCE 4 /* iteration cap */
#define MSFM_BA_FAILURE 5        /* too many consecutive invalid steps */
#define MSFM_BA_MIN_RADIUS 6

/* One row of the Ceres progress table per iteration (row 0 = iteration 0). */
typedef struct msfm_ba_iteration {
  double cost;              /* after the iteration                                        */
  double cost_change;
  double gradient_max_norm;
  double step_norm;
  double relative_decrease; /* tr_ratio                                                   */
  double trust_region_radius;
  int32_t step_is_valid;
  int32_t step_is_successful;
} msfm_ba_iteration;

typedef struct msfm_ba_summary {
  int termination;
  int num_iterations;       /* rows written to `iterations` minus 1                       */
  int num_successful_steps;
  int num_unsuccessful_steps;
  double initial_cost, final_cost;
  int num_residuals;        /* scalar residual count                                      */
  int num_reduced_params;   /* order of the reduced camera system                         */
  msfm_ba_iteration* iterations; /* caller-provided, may be NULL                          */
  int iterations_capacity;
  double solve_ms;          /* device time of the LM loop, problem already resident       */
  double setup_ms;          /* upload + symbolic set-up (block-pair lists)                */
} msfm_ba_summary;

/* Replaces `ceres::Solve(options_, &problem_, &summary_)` at SfM/src/optimizer.cc:133 and
 * SfM/src/slam_gps.cc:841: trust-region Levenberg–Marquardt, Huber(1) loss, Jacobi
 * scaling, dense Schur complement on the points, dense Cholesky of the reduced camera
 * system, with the Ceres 1.13 control flow (step acceptance, radius update, stopping
 * rules).  Updates cam_pose / cam_model / point in place, like Ceres does through the
 * `data` blocks. */
int msfm_ba_solve(msfm_ctx* ctx, msfm_ba_problem* problem, const msfm_ba_options* options,
                  msfm_ba_summary* summary);

/* Split form, for callers that keep a problem resident across solves (bench loop,
 * windowed BA re-solves): create = upload + symbolic set-up, run = LM loop on the
 * resident state, download = copy parameters back, reset = re-upload parameters only. */
typedef struct msfm_ba msfm_ba;
int msfm_ba_create(msfm_ctx* ctx, const msfm_ba_problem* problem, msfm_ba** out);
int msfm_ba_run(msfm_ba* ba, const msfm_ba_options* options, msfm_ba_summary* summary);
int msfm_ba_upload_params(msfm_ba* ba, const double* cam_pose, const double* cam_model,
                          const double* point);
int msfm_ba_download_params(msfm_ba* ba, double* cam_pose, double* cam_model, double* point);
void msfm_ba_destroy(msfm_ba* ba);
/* How the reduced camera system of a resident problem is laid out and eliminated (no reference counterpart:
 * Ceres' DENSE_SCHUR factors S in the given camera order).  n_domains <= 1: dense order. */
typedef struct msfm_ba_layout {
  int reduced_order;      /* 6 * camera blocks + 3 * intrinsics blocks */
  int system_order;       /* order of the factored matrix: reduced_order + identity padding of the domains */
  int n_domains;          /* mutually uncoupled camera domains whose panel chains share launches */
  int domain_cols[8];     /* columns of each domain (multiples of 64) */
  int separator_cols;     /* every separator + intrinsics (everything behind the leaf domains) */
  int panel_launches;     /* panel launches per factorisation */
  /* the elimination tree behind it: level 0 = the leaf domains above, level 1.. = separators from the deepest cut to
   * the shallowest (nodes of one level are mutually uncoupled and share launches), then the root chain */
  int n_levels;
  int level_nodes[3];
  int level_begin[3];     /* first column of each level */
  int root_cols;          /* root separator + intrinsics: the final dense chain */
  /* Schur products formed inside the point kernel instead of by the gather kernels (0 everywhere: gather path only):
   * pair-list entries of the camera x camera list in all / folded; (workgroup, block) slots = 288-byte partial sums the
   * point kernel writes and the assembly reads; the same for the intrinsics x camera list (144-byte partials) */
  long long cc_entries, cc_entries_folded;
  int fold_slots, fold_passes;
  long long mc_entries, mc_entries_folded;
  int fold_mc_slots;
  /* how the last factorisation of msfm_ba_run ran (0 before the first one): MSFM_PATH_LEVEL_CHAIN(l) = tree level l as one
   * persistent k_chain launch, MSFM_PATH_ROOT_CHAIN = the root chain as one, MSFM_PATH_BACKSOLVE_CHAIN = the back
   * substitution as one k_backsolve_chain launch; a clear bit = one launch per 64-column panel / block pair */
  int solve_paths;
  /* eliminated points by track length class (msfm_ba_create orders them class-major): up to 8 rows, 9..16 rows, more.  The
   * point kernels give a point of up to 4 rows 4 lanes, of 5..8 rows 8 lanes, of 9..16 rows 16 - one row per lane - and take
   * the rows of longer tracks in rounds of 8; a workgroup never mixes lane widths.  npb_S counts every point of up to 8
   * rows; npb_S4 says how many of those have up to 4 rows (they come first and have the 4 lanes when the problem has more
   * than MSFM_LANES4_MIN eliminated points, default 24 576; in a smaller problem they are 8-lane points in the common order) */
  int npb_S, npb_L, npb_X;
  int npb_S4;
  /* how the last reduced system of msfm_ba_run was assembled (0 before the first one): MSFM_PATH_ASM_BESIDE = the fold partials
   * were summed into the system by workgroups of the per-camera sums' launch and the blocks finished by the launches that
   * form the per-camera and per-intrinsics sums; 0 = by a launch of its own behind them */
  int assemble_paths;
  /* what rode along with the launches of the last factor-and-solve of msfm_ba_run instead of being a launch of its own (0
   * before the first solve, and always with MSFM_SOLVE_RIDERS=0): MSFM_PATH_RIDER_MODELSUM = the per-intrinsics sums and the
   * intrinsics block of the system, by extra workgroups of the first corner update (only with MSFM_PATH_ASM_BESIDE and an
   * elimination tree); MSFM_PATH_RIDER_UPDATE = the camera / intrinsics part of the step, by the back substitution's launch
   * block by block behind the publication of each (only where that is one launch and the point part of the step has the
   * workgroups for its block sums).  The bits of this field are
   * distinct from those of the two fields above, so that a value read from the wrong field shows. */
  int rider_paths;
  /* how the point kernel's four waves share the products of a workgroup (0 everywhere: gather path only).  Four threads - a
   * quad - sum a slot; a slot of more than 8 entries is cut into up to four parts with a quad each, which are added up inside
   * the wave.  fold_parts = quads with work (= fold_slots where no slot is cut).  The other three count entry steps - one
   * trip of a quad's loop over its entries - by this model: the sixteen quads of a wave take as long as the longest of them,
   * and a pass of a workgroup as long as the wave with the most steps.  fold_crit_steps = that wave's steps summed over all
   * passes, fold_crit_steps_unsplit = the same figure had no slot been cut, fold_wave_steps = the steps of all waves. */
  long long fold_parts, fold_crit_steps, fold_crit_steps_unsplit, fold_wave_steps;
} msfm_ba_layout;
#define MSFM_PATH_ASM_BESIDE 1
#define MSFM_PATH_RIDER_MODELSUM (1 << 8)
#define MSFM_PATH_RIDER_UPDATE (1 << 9)
#define MSFM_PATH_LEVEL_CHAIN(l) (1 << (l))
#define MSFM_PATH_ROOT_CHAIN (1 << 3)
#define MSFM_PATH_BACKSOLVE_CHAIN (1 << 4)
int msfm_ba_get_layout(const msfm_ba* ba, msfm_ba_layout* out);

/* The elimination order of msfm_ba_create as a host-only function (no device, no context: a diagnostic for tests and for
 * sizing): the nested dissection of a camera graph given as an n x n 0/1 adjacency matrix (cameras that see a common
 * eliminated point; the reduced camera matrix of optimizer.cc:133's Schur complement has a block exactly there).
 * tail_cols = columns that follow the last camera (3 per intrinsics block + 1), force_depth = -1 (choose) or 1..3.
 * label[c] = leaf domain of camera c (0 .. n_leaves - 1), or -(d + 1) for a camera of a separator cut at depth d (-1 = the
 * root separator).  *chain_steps = 64-column panel steps on the critical path (longest leaf + longest separator of every
 * depth + root).  *n_leaves = 0 (and every label 0): the dense order is kept. */
int msfm_camera_graph_dissection(int n_cams, const uint8_t* adjacency, int tail_cols, int force_depth, int32_t* label,
                                 int* n_leaves, int* chain_steps);

/* Multi-GPU: points (with all their observations) are sharded over ranks, cameras and
 * intrinsics are replicated; a few times per LM iteration `count` doubles at `buf_dev` (the per-camera J^T J sums, the
 * partial reduced system [S | rhs], a handful of scalars) must be reduced over ranks in place
 * with `op` (sum or max).
 * The host supplies the collective (RCCL all-reduce through torch.distributed in the
 * Python host, ncclAllReduce in a C++ host); it is called on the host thread that runs
 * the solve, after the producing kernels have been enqueued on `stream`, and must leave
 * the reduced data visible to work enqueued on `stream` afterwards.
 * The reference has no counterpart (no collective anywhere in SfM/src). */
#define MSFM_REDUCE_SUM 0
#define MSFM_REDUCE_MAX 1
typedef int (*msfm_allreduce_fn)(void* user, double* buf_dev, size_t count, int op, void* stream);
int msfm_ctx_set_allreduce(msfm_ctx* ctx, msfm_allreduce_fn fn, void* user, int rank,
                           int world_size);

/* The same collective supplied by the library itself: RCCL all-reduce over xGMI, one process per GPU (the
 * multi-GPU context owns the communicator).  librccl is loaded at run time by these two calls only, so a single-GPU
 * host has no RCCL dependency.  Rank 0 obtains an id, the host hands the 128 bytes to the other ranks by whatever it has
 * (MPI_Bcast, a file, torch.distributed.broadcast_object_list), then EVERY rank calls msfm_ctx_init_rccl - a collective
 * call - which creates the communicator on the context's device and installs ncclAllReduce (ncclDouble, sum / max,
 * in place, on the context's stream) as the reduction hook.  msfm_ctx_destroy releases the communicator. */
#define MSFM_RCCL_ID_BYTES 128
int msfm_rccl_get_unique_id(msfm_ctx* ctx, unsigned char id[MSFM_RCCL_ID_BYTES]);
int msfm_ctx_init_rccl(msfm_ctx* ctx, const unsigned char id[MSFM_RCCL_ID_BYTES], int rank, int world_size);
/* Runs the installed collective (host hook or the native RCCL one) on `count` doubles at `buf_dev`, in place, ordered on
 * the context's stream - what the solver does internally; exposed so that a host can reduce its own per-rank results
 * (the N x N match-count matrix of fine_matching_graph.cc:275-292, timing maxima) through the same communicator. */
int msfm_ctx_allreduce(msfm_ctx* ctx, double* buf_dev, size_t count, int op);

/* ==================================================================================== *
 *  Triangulation / reprojection  
 * ==================================================================================== */

/* Tracks in CSR form; cameras as the reference keeps them (camera.h:60-75):
 *   cam_R [n_cams][9] row-major R, cam_t [n_cams][3], cam_c [n_cams][3] centre,
 *   cam_fk [n_cams][3] = f, k1, k2 of the camera's CameraModel. */
typedef struct msfm_tracks {
  int n_tracks, n_cams;
  const int32_t* track_off; /* [n_tracks+1] */
  const int32_t* track_cam; /* [track_off[n_tracks]] */
  const double* track_xy;   /* [..][2] centred pixels */
  const double* cam_R;
  const double* cam_t;
  const double* cam_c;
  const double* cam_fk;
} msfm_tracks;

/* Point3D::Trianglate2 (SfM/src/structure.cc:211-265): ray-midpoint normal equations
 * solved by 4x4 LLT, then Reprojection() (:267-300) and
 * SufficientTriangulationAngle() (:325-355).
 *   X [n][3]; mse [n] (1e5 on negative depth, :280-284); ok [n] = return value.
 * A failed LLT leaves X untouched and ok = 0 (:248-251); X must therefore be
 * initialised by the caller. th_angle in radians. */
int msfm_triangulate_midpoint_batch(msfm_ctx* ctx, const msfm_tracks* tracks, double th_error,
                                    double th_angle, double* X, double* mse, uint8_t* ok);
/* Point3D::Trianglate (SfM/src/structure.cc:163-209): DLT rows :179-182, last right
 * singular vector (:187), same acceptance test.  Tracks with < 2 views return ok = 0. */
int msfm_triangulate_dlt_batch(msfm_ctx* ctx, const msfm_tracks* tracks, double th_error,
                               double th_angle, double* X, double* mse, uint8_t* ok);
/* Point3D::Reprojection (SfM/src/structure.cc:267-300) for given X; this is what
 * IncrementalSfM::RemovePointOutliers recomputes per point (sfm_incremental.cc:1831-1863). */
int msfm_reproject_mse_batch(msfm_ctx* ctx, const msfm_tracks* tracks, const double* X,
                             double* mse);

/* Closed-form fundamental-matrix filter (SfM/src/utils/geo_verification.cc:60-79):
 * l = F*[x1,y1,1]; l /= hypot(l0,l1); inlier iff |l . [x2,y2,1]| < th (3.0).
 * pt1/pt2 are float pixel pairs as cv::Point2f; inlier[n] gets 0/1. */
int msfm_epipolar_filter(msfm_ctx* ctx, const float* pt1, const float* pt2, int n,
                         const double F[9], double th, uint8_t* inlier);

/* GeoVerification::GeoVerificationFundamental (SfM/src/utils/geo_verification.cc:30-58), batched over image
 * pairs: cv::findFundamentalMat(pt1, pt2, status, cv::FM_RANSAC, 3.0) followed by the >= 30 inliers gate
 * (:34-36, :54-56).  OpenCV 2.4's FM_RANSAC restated: 7-point minimal solver (up to 3 models per sample),
 * error = max of the two squared point-to-epipolar-line distances <= threshold^2, confidence 0.99, at most
 * 2000 samples with the adaptive stop of cvRANSACUpdateNumIters, best model returned without refit.  The
 * sampler is counter based: sample h of pair p (its index in this call) depends only on (seed, p, h).
 * Pair p owns matches [offsets[p], offsets[p+1]); pt1/pt2 are cv::Point2f pairs (centred pixels).
 * Out: F[p][9] row-major (x2^T F x1 = 0, F[8] = 1 when possible; zeros when no model), inlier[total] 0/1
 * against the returned F, n_inliers[p], ok[p] = the bool GeoVerificationFundamental returns. */
typedef struct msfm_fransac_options {
  double threshold;      /* 3.0  (th_epipolar1, geo_verification.cc:44) */
  double confidence;     /* 0.99 (findFundamentalMat default param2)    */
  int max_iterations;    /* 2000 (CvModelEstimator2::runRANSAC default) */
  int min_points;        /* 30   (geo_verification.cc:34)               */
  int min_inliers;       /* 30   (geo_verification.cc:54)               */
  uint64_t seed;
} msfm_fransac_options;
void msfm_fransac_default_options(msfm_fransac_options* opt);
int msfm_fundamental_ransac_batch(msfm_ctx* ctx, int n_pairs, const int* offsets, const float* pt1,
                                  const float* pt2, const msfm_fransac_options* opt, double* F,
                                  uint8_t* inlier, int* n_inliers, uint8_t* ok);
/* cv::findHomography(pts1, pts2, mask, RANSAC, th) of OpenCV 2.4 (cvFindHomography + CvHomographyEstimator), batched over
 * image pairs: the prior homography of SLAMGPS::FeatureMatching step 1 (SfM/src/slam_gps.cc:402).  4-point samples with
 * OpenCV's collinearity check (300 attempts), error = binary32 squared transfer distance into image 2 <= threshold^2, at most
 * max_iterations samples with the adaptive stop of cvRANSACUpdateNumIters (confidence 0.995, 4 model points), then (polish)
 * a refit on the inliers and 10 Levenberg-Marquardt iterations, as cvFindHomography does.  The sampler is counter based:
 * sample h of pair p (its index in this call) depends only on (seed, p, h).  Pair p owns correspondences
 * [offsets[p], offsets[p+1]); pt1 / pt2 are cv::Point2f pairs, H maps pt1 to pt2.
 * Out: H[p][9] row-major with H[8] = 1 (zeros when no model), inlier[total] = the RANSAC mask of the best sample's model
 * (not recomputed after the polish), n_inliers[p], ok[p] = cvFindHomography's result.  N == 4: the direct fit, mask all
 * ones; N < 4: ok = 0, mask 0; no model found: ok = 0, H = 0 and the mask all ONES (cvFindHomography's temporary mask starts
 * at ones and is written back only when a model was found), so n_inliers = N.
 * Departure at N == 4: the direct fit is the exact 8x9 null space, and a rank-deficient system (e.g. four collinear points)
 * or a non-finite H gives ok = 0; OpenCV's runKernel (LtL eigenvector) returns 1 for any set whose spreads are
 * >= DBL_EPSILON, with whatever H that eigenvector gives.
 * MSFM_E_INVAL: max_iterations outside [1, 65536], confidence outside (0, 1), offsets not starting at 0 or decreasing. */
typedef struct msfm_hransac_options {
  double threshold;   /* 3.0   ransacReprojThreshold (<= 0 -> 3.0, as OpenCV does)                               */
  double confidence;  /* 0.995 fixed inside cvFindHomography                                                     */
  int max_iterations; /* 2000  fixed inside cvFindHomography                                                     */
  int polish;         /* 1: refit on the inliers + 10-iteration LM refine, as cvFindHomography does;
                         0: the best sample's model as found                                                     */
  uint64_t seed;
} msfm_hransac_options;
void msfm_hransac_default_options(msfm_hransac_options* opt);
int msfm_homography_ransac_batch(msfm_ctx* ctx, int n_pairs, const int* offsets, const float* pt1, const float* pt2,
                                 const msfm_hransac_options* opt, double* H /*[n][9]*/, uint8_t* inlier /*[total]*/,
                                 int* n_inliers, uint8_t* ok);

/* SLAMGPS::FeatureMatching step 1 (SfM/src/slam_gps.cc:323-423) in one call: the matching graph of a SLAM run and the prior
 * F and H of every kept image pair, which msfm_match_pairs_slam (step 2) takes.  For camera i ascending and j ascending
 * over [max(i - win_size, 0), min(i + win_size, n_cams)), j != i (:348-357; offsets -win_size .. win_size - 1):
 *   shared   the SLAM points seen by both cameras, ascending point index (math::same_in_vectors, :330-340, :360-364);
 *            fewer than th_same_pts -> skipped (verdict 1)
 *   pts1/2   their observations in i / j as cv::Point2f (binary32, :365-382)
 *   F        msfm_fundamental_ransac_batch (cv::findFundamentalMat(FM_RANSAC, th_epipolar), :385-393) over the list of the
 *            candidates with enough shared points (sampler index = position in that list, confidence 0.99, 2000 samples,
 *            seed_f); rejected if (float)n_f < (float)n * th_ratio_f or n_f < 30 (:396, binary32; verdict 2)
 *   H        msfm_homography_ransac_batch (cv::findHomography(RANSAC, th_distance), :400-408) on the same list (seed_h,
 *            default options otherwise); rejected if (float)n_h > (float)n_f * th_h_f_ratio (:409, binary32; verdict 3)
 *   kept     (i, j, F, H) in (i, j) order (:411-415) - exactly the pairs / F / H of msfm_match_pairs_slam.
 * H is not run for candidates the F gate rejects (their candidate row says -1); kept results do not depend on it.
 * A candidate whose F RANSAC finds no model has n_f = 0 (msfm_fundamental_ransac_batch's mask is 0 then) and verdict 2;
 * cvFindFundamentalMat would leave its mask at all ones, so the reference counts n_f = N there - a rare departure that the
 * composition of the public calls defines.
 * The SLAM points come as msfm_tracks: n_tracks points, n_cams cameras, track_off / track_cam / track_xy (cam_* unused, may
 * be NULL).  MSFM_E_INVAL: two observations of one point in one camera (pts1 / pts2 would not line up), a camera outside
 * [0, n_cams), win_size < 1, th_same_pts < 15 (below 15 OpenCV 2.4's findFundamentalMat does not run RANSAC),
 * th_epipolar <= 0 or NaN and th_distance NaN (what the two public calls refuse; th_distance <= 0 means 3.0, as there).
 * The default thresholds are those of resize_ratio = 1; SLAMGPS::SLAMGPS sets resize_ratio = 0.5 (slam_gps.cc:55), so a
 * reference run uses th_epipolar = 4 and th_distance = 10 px on observations stored at full resolution (:199).
 * cap = n_cams * (2 * win_size - 1) bounds both outputs.  Out: n_pairs kept pairs [cap][2], F / H [cap][9]; candidates (may
 * be NULL) [cap][6] = i, j, n_shared, n_inliers_f, n_inliers_h (-1: not run), verdict (0 kept, 1 shared, 2 F gate, 3 H gate)
 * for every window slot in (i, j) order, *n_candidates rows. */
typedef struct msfm_slam_prior_options {
  int win_size;        /* 5    slam_gps.cc:314 */
  int th_same_pts;     /* 20   :315            */
  float th_epipolar;   /* 2.0 / resize_ratio  :316 */
  float th_distance;   /* 5.0 / resize_ratio  :317 */
  float th_ratio_f;    /* 0.5  :318 */
  float th_h_f_ratio;  /* 0.90 :319 */
  uint64_t seed_f, seed_h;
} msfm_slam_prior_options;
void msfm_slam_prior_default_options(msfm_slam_prior_options* opt);
int msfm_slam_priors(msfm_ctx* ctx, const msfm_tracks* points, const msfm_slam_prior_options* opt, int* n_pairs,
                     int* pairs, double* F, double* H, int* n_candidates, int* candidates);

/* The closed-form filter above for many pairs at once (fine_matching_graph.cc:148-150: applied to the
 * "all" match set only when the pair's RANSAC succeeded): pairs with ok[p] == 0 get all-zero masks
 * (ok may be NULL = every pair). */
int msfm_epipolar_filter_batch(msfm_ctx* ctx, int n_pairs, const int* offsets, const float* pt1,
                               const float* pt2, const double* F, const uint8_t* ok, double th,
                               uint8_t* inlier);

/* ======================================================================================
 *  Track building between matching and triangulation  
 * ====================================================================================== */
/* The data association of SLAMGPS::Triangulation (SfM/src/slam_gps.cc:565-635): walk the image pairs in the
 * caller's order (the reference: idx1 ascending, idx2 ascending over match_graph_[idx1][idx2] > 0) and their matches
 * (feature in idx1, feature in idx2): a match whose first feature already belongs to a point adds the second
 * feature to it (:597-606), else one whose second feature belongs to a point adds the first (:607-616), else a new
 * point is created (:617-633).  std::map::insert semantics are kept: a point holds at most one observation per
 * image (the first), a feature stays with the first point it was mapped to, two existing points are never merged.
 * msfm_tracks_build is that walk on the host; msfm_tracks_build_device gives the identical result from the GPU (first
 * appearances by atomicMin, the "joins" forest, a stable sort of the observations by (point, image)) - the form for the
 * match lists of a whole image set (config 3: 6 M matches).  The tracks then go to msfm_triangulate_midpoint_batch (th_tri_angle = 3 degrees, points with fewer
 * than 3 views or a failed triangulation are marked bad, :638-648).
 * Out: CSR tracks, observations of a track in ascending image order (std::map iteration order). */
typedef struct msfm_track_set msfm_track_set;
int msfm_tracks_build(int n_images, const int* n_features, int n_pairs, const int* pair_img /*[n_pairs][2]*/,
                      const int* match_off /*[n_pairs+1]*/, const int* matches /*[match_off[n_pairs]][2]*/,
                      msfm_track_set** out);
int msfm_tracks_build_device(msfm_ctx* ctx, int n_images, const int* n_features, int n_pairs, const int* pair_img,
                             const int* match_off, const int* matches, msfm_track_set** out);
int msfm_track_set_size(const msfm_track_set* set, int* n_tracks, int* n_observations);
int msfm_track_set_fetch(const msfm_track_set* set, int* track_off /*[n_tracks+1]*/, int* obs_image, int* obs_feature);
void msfm_track_set_destroy(msfm_track_set* set);

/* ======================================================================================
 *  The same chain with every intermediate result resident on the GPU
 * ====================================================================================== */
/* match codes -> geometric verification -> track building -> triangulation -> bundle adjustment without a host round trip
 * in between: the hand-over the reference makes through std::vector / std::map objects per pair and per point
 * (fine_matching_graph.cc:116-186 -> slam_gps.cc:557-648 -> optimizer.cc:59-133; incremental form
 * sfm_incremental.cc:755-915).  Each step runs the kernels of its host-array counterpart on device buffers and gives
 * the same result bit for bit; between the descriptor / keypoint upload and msfm_ba_download_params only a few integers
 * per image pair and the cameras cross PCIe.  Image index = camera index.
 *   msfm_chain_create       takes the codes of a msfm_match_pairs or msfm_match_pairs_slam result whose descriptor set holds
 *                           the keypoints of every image involved (msfm_descset_upload_keypoints); the chain records the form
 *   msfm_chain_verify       per pair: GeoVerificationFundamental on matches_good (msfm_fundamental_ransac_batch, pair p of the
 *                           list = pair p of the sampler), then, if it succeeded, the closed-form filter with th_filter (3.0)
 *                           on matches_all; a pair keeps the surviving matches_all entries, a failed pair none
 *                           (fine_matching_graph.cc:138-153, :182-186)
 *   msfm_chain_verify_slam  the verification of a SLAM-form chain, the tail of SLAMGPS::FeatureMatching step 2
 *                           (slam_gps.cc:503-541): GeoVerificationFundamental on ALL survivors of the pair's three checks in
 *                           query order (pair p of the list = pair p of the sampler), no good / all split and no filter
 *                           behind it; the pair keeps the entries of the RANSAC mask WHATEVER the verdict:
 *                             < min_points survivors              -> no RANSAC, no match, ok = 0
 *                             >= min_points, < min_inliers inliers -> ok = 0 and those 1..29 matches are kept
 *                             no model found                       -> mask of msfm_fundamental_ransac_batch is 0: no match
 *                           matches are (train feature in id1, query feature m in id2) in ascending m.  Each verify call
 *                           refuses a chain of the other form, a second call and a result the chain was not made from
 *                           (MSFM_E_INVAL; the chain stays usable)
 *   msfm_chain_build_tracks msfm_tracks_build_device on those matches, pairs in the order of the match result
 *   msfm_chain_triangulate  msfm_triangulate_midpoint_batch on every track (X starts at 0), observations from the keypoints
 *   msfm_chain_ba_create    msfm_ba_create on the tracks with ok = 1 and >= min_views observations (slam_gps.cc:638-648:
 *                           3), gather order and weights of optimizer.cc:59-129 (2 views -> 1.0, more -> weight_ge3);
 *                           cameras / intrinsics from the caller (host), every block mutable.  The msfm_ba is the caller's.
 * The fetch functions copy a stage's result to the host (tests, file writers); none is needed to go on. */
typedef struct msfm_chain msfm_chain;
int msfm_chain_create(msfm_match_result* res, msfm_chain** out);
int msfm_chain_verify(msfm_chain* chain, msfm_match_result* res, const msfm_fransac_options* opt, double th_filter);
int msfm_chain_verify_slam(msfm_chain* chain, msfm_match_result* res, const msfm_fransac_options* opt);
int msfm_chain_matches(msfm_chain* chain, int* n_matches /*[n_pairs]*/, uint8_t* ok /*[n_pairs]*/, double* F /*[n_pairs][9]*/);
int msfm_chain_fetch_matches(msfm_chain* chain, int pair, int* matches /*[n_matches[pair]][2]*/);
int msfm_chain_build_tracks(msfm_chain* chain, int* n_tracks, int* n_observations);
int msfm_chain_fetch_tracks(msfm_chain* chain, int* track_off, int* obs_image, int* obs_feature);
int msfm_chain_triangulate(msfm_chain* chain, int n_cams, const double* cam_R, const double* cam_t, const double* cam_c,
                           const double* cam_fk, double th_error, double th_angle, int* n_accepted);
int msfm_chain_fetch_points(msfm_chain* chain, double* X /*[n_tracks][3]*/, double* mse, uint8_t* ok);
int msfm_chain_ba_create(msfm_chain* chain, int n_cams, int n_models, double* cam_pose, double* cam_model,
                         const int32_t* cam_model_of_cam, int min_views, double weight_ge3, msfm_ba** out, int* n_points,
                         int* n_observations);
/* track index of every point of the bundle adjustment (to put the adjusted points back) */
int msfm_chain_fetch_point_tracks(msfm_chain* chain, int* track_of_point /*[n_points]*/);
void msfm_chain_destroy(msfm_chain* chain);

/* ======================================================================================
 *  SLAM + GPS registration
 * ====================================================================================== */
/* What SLAMGPS::Run (SfM/src/slam_gps.cc:63-137) does between Triangulation (:98) and the end of FullBundleAdjustment
 * (:119) beside the adjustment itself: AbsoluteOrientationWithGPSGlobal, GetAccuracy, GPSRegistration2, and the GPS rows of
 * the bundle adjustment.  metricsfm_amd/gpsreg.py drives them in the reference's order on a msfm_chain.
 * The device code uses + - * / sqrt only and no fused multiply-adds, so a CPU restatement built with -ffp-contract=off
 * agrees bit for bit (tests/gpsreg_ref.cpp). */
typedef struct msfm_gpsreg_options {
  int32_t window;     /* 20: the weight of camera i looks at cameras i - window and i + window, clamped (slam_gps.cc:1607-1614) */
  int32_t min_views;  /* 3: tracks with fewer rows are bad before GetAccuracy sees them (slam_gps.cc:638-648) */
  double clip_deg;    /* 80: upper bound of the turning angle whose tangent is the weight (slam_gps.cc:1621-1623) */
  double th_outlier;  /* 3.0: th_outlier of GetAccuracy (slam_gps.cc:1587) */
} msfm_gpsreg_options;
void msfm_gpsreg_default_options(msfm_gpsreg_options* opt);

/* SLAMGPS::AbsoluteOrientationWithGPSGlobal (slam_gps.cc:1596-1674).  Host only (acos, tan and sqrt of the C library).
 *   weight[i] = tan(min(|acos(ds . de / sqrt(|ds|^2 + 0.1) / sqrt(|de|^2 + 0.1)) - pi|, clip)), ds / de the x, y steps from
 *               GPS position i to positions max(0, i - window) and min(n - 1, i + window)                       (:1606-1624)
 *   SimilarityTransformation (SfM/src/utils/transformation.cpp:142-216) of the camera centres onto the GPS positions as
 *               written: unweighted centroids, weighted covariance and source variance divided by n, the SVD of the
 *               covariance, Z(2,2) = det(V U^T), Rg = V Z U^T, scale = sum S_i Z_ii / s_mv, tg = -scale Rg s_center +
 *               d_center, err = the mean distance.  The 3x3 SVD restates Eigen 3's two-sided JacobiSVD from its published
 *               algorithm; agreement with Eigen itself is not pinned.
 *   Camera::Transformation (SfM/src/camera.cc:79-87) on every camera: R' = R Rg^-1 (inverse by cofactors), c' = scale Rg c +
 *               tg, t' = -R' c', the angle-axis vector by RotationMatrixToAngleAxis                             (:1639-1641)
 *   offset = mean of the new centres (gps_offset_), subtracted from the cameras - a second Camera::Transformation with
 *               (I, -offset, 1) - and from the GPS positions                                                    (:1651-1673)
 * In : cam_R [n][9] row-major, cam_c [n][3], gps [n][3]; opt may be NULL (defaults; window and clip_deg are read).
 * Out: the caller's arrays cam_R [n][9], cam_t / cam_c / cam_aa / gps [n][3], weight [n], and the scalars.
 * n_cams < 3 is MSFM_E_INVAL (the reference ignores SimilarityTransformation's failed return and goes on with
 * uninitialised values), as is a null pointer. */
typedef struct msfm_gps_orient_result {
  double* cam_R;
  double* cam_t;
  double* cam_c;
  double* cam_aa;
  double* gps;
  double* weight;
  double Rg[9], tg[3], scale, err, offset[3];
} msfm_gps_orient_result;
int msfm_gps_orient_global(int n_cams, const double* cam_R, const double* cam_c, const double* gps, const msfm_gpsreg_options* opt,
                           msfm_gps_orient_result* out);

/* SLAMGPS::GetAccuracy (slam_gps.cc:1573-1594) = AccuracyAssessment::ErrorReprojectionPts / ErrorReprojectionPti
 * (SfM/src/accuracy_accessment.cc:38-113) and the flags of :1584-1593, on CSR tracks (cam_c of `tracks` is not read).
 * Per track, rows in order: pt_c = [R|t] (X, 1); a row with pt_c.z > 0 gives e = (u - x)^2 + (v - y)^2 with
 * u = f (1 + r2 (k1 + k2 r2)) x + dcx (std::pow(d, 2) stated as d * d).  With m such rows: e_avg their sequential mean,
 * e_mse = sqrt(sum (e - e_avg)^2 / (m - 1)), n_used = m.  m < 2, ok_in == 0 or fewer than min_views rows: e_avg = 1000.0
 * (:94), e_mse = 0, n_used = 0.  ok_out = ok_in && rows >= min_views && !(e_avg > th_outlier) - the negation of
 * is_bad_estimated_ after :1587-1590; n_outliers = tracks with e_avg > th_outlier, n_inliers = the others (:1584-1593).
 * cam_dc [n_cams][2] = dcx, dcy of the camera's model, NULL = 0.  The aggregates :110-112 print are not formed.
 * n_outliers / n_inliers may be NULL.  A track_cam outside n_cams, a NaN threshold or a null array is MSFM_E_INVAL. */
int msfm_point_accuracy_batch(msfm_ctx* ctx, const msfm_tracks* tracks, const double* cam_dc, const double* X, const uint8_t* ok_in,
                              int min_views, double th_outlier, double* e_avg /*[n]*/, double* e_mse /*[n]*/, int32_t* n_used /*[n]*/,
                              uint8_t* ok_out /*[n]*/, int* n_outliers, int* n_inliers);
/* The point loop of SLAMGPS::GPSRegistration2 (slam_gps.cc:933-978): cam_offset[c] = gps[c] - cam_c[c] once per camera
 * (:920-924); per track with ok != 0, rows in order: dis = |X - cam_c[c]|, w = 1 / (sqrt(dis) + 5), weight_i += w,
 * offset_i += w * cam_offset[c]; then offset_i /= weight_i and X += offset_i.  Tracks with ok == 0 are untouched.  (:980-982,
 * every camera onto its GPS position, is SetACPose on the host's cameras.) */
int msfm_gps_register_points(msfm_ctx* ctx, int n_tracks, const int32_t* track_off, const int32_t* track_cam, const uint8_t* ok, int n_cams,
                             const double* cam_c, const double* gps, double* X /*[n_tracks][3], in / out*/);

/* The same on the resident tracks / observations / X / ok of a triangulated msfm_chain; bit for bit what the two calls above
 * give on the fetched arrays.
 *   msfm_chain_accuracy       writes ok_out into the chain's ok (GetAccuracy's effect: msfm_chain_fetch_points shows it,
 *                             msfm_chain_ba_create leaves the removed points out); msfm_chain_fetch_accuracy copies e_avg /
 *                             e_mse / n_used [n_tracks] of the last call to the host (any may be NULL)
 *   msfm_chain_gps_register   shifts the resident X in place
 *   msfm_chain_ba_create_gps  msfm_chain_ba_create with the GPS rows of FullBundleAdjustment (slam_gps.cc:818-830):
 *                             gps_xyz [n_cams][3]; gps_weight <= 0: the rule of :824, (double)(n_observations / n_cams) in
 *                             integer division; gps_weight_used (may be NULL) reports the weight of the problem
 *   msfm_chain_store_points   the adjusted points of the msfm_ba this chain made last back into X[track_of_point[p]],
 *                             device to device (the second GetAccuracy, :119, and the final cloud then come from the chain);
 *                             any other msfm_ba is MSFM_E_INVAL */
int msfm_chain_accuracy(msfm_chain* chain, int n_cams, const double* cam_R, const double* cam_t, const double* cam_fk, const double* cam_dc,
                        int min_views, double th_outlier, int* n_outliers, int* n_inliers);
int msfm_chain_fetch_accuracy(msfm_chain* chain, double* e_avg, double* e_mse, int32_t* n_used);
int msfm_chain_gps_register(msfm_chain* chain, int n_cams, const double* cam_c, const double* gps);
int msfm_chain_ba_create_gps(msfm_chain* chain, int n_cams, int n_models, double* cam_pose, double* cam_model,
                             const int32_t* cam_model_of_cam, int min_views, double weight_ge3, const double* gps_xyz, double gps_weight,
                             double* gps_weight_used, msfm_ba** out, int* n_points, int* n_observations);
int msfm_chain_store_points(msfm_chain* chain, msfm_ba* ba);

/* ======================================================================================
 *  Which image pairs to match: hypotheses from visual words, verified in batches
 * ====================================================================================== */
/* InitialMatchingGraph::match_graph_feature (SfM/src/graph/initial_matching_graph.cc:164-294) with the inverted-file
 * similarity of SimilarityGraph::SimilarityGraphInvFile (similarity_graph.cc:47-117).  Input is what the reference reads from
 * its `<i>_words` and `<i>_feature` files: per image the word id of every feature (Database::words_id_[i]) and the keypoints.
 * Sort an image's word ids; the runs of equal ids are its groups g0 < g1 < ... < gm.  The reference's quirks are kept:
 *   inverted file  the image enters word w's bin iff w's group is a single feature and is neither g0 (keep_unique_vector,
 *                  basic_funcs.h:127-152, compares the first element with itself) nor gm (the last group is never pushed, so
 *                  id num_words never reaches the num_words-sized table).  A bin with more than num_words / 100 images
 *                  (integer division) is emptied (:109-116).
 *   similarity     S[a][b] = bins that hold both images (:68-81): symmetric, zero diagonal; int32 here, the same integers in
 *                  float there.
 *   hypotheses     image i: all j != i by S[i][j] descending, the first K (:216-231).  Equal similarity goes to the lower
 *                  image id (the reference leaves ties to std::sort).  Images without words take part with similarity 0.
 *   word table     keep_unique_idx_vector (basic_funcs.cc:380-408): group g_k, k >= 2, gives the entry (its word, its lowest
 *                  feature index) iff g_(k-1) is a single feature, whatever its own size; g0 and g1 never do.  (Lowest feature:
 *                  the reference's std::sort leaves it open.)  No stop-word rule here; an image without words has no entries.
 *   join           hypothesis (i, j): the entries of i's table in ascending word order whose word is in j's table, as
 *                  (feature of i, feature of j) (:242-253); n_init = their number.
 *   verification   problem r * K + s of ONE msfm_fundamental_ransac_batch call holds the joined keypoints of row r, slot s of a
 *                  msfm_pair_select call, all of them (min_points rejects the short ones): F, inlier, n_inliers, ok of the
 *                  chunk are that call's, bit for bit.  The sampler index is the position in the call, so how a host cuts the
 *                  images into chunks decides which samples a pair sees (as for the seed search).
 *   verdict        0 kept: n_init >= th_init_matches (:254), ok (:270), n_inliers > th_inliers (:274); 1: too few joined
 *                  matches; 2: GeoVerificationFundamental false; 3: verified, but not more than th_inliers inliers.
 *   pairs          the kept hypotheses as (idx1, idx2) in (row, slot) order = match_graph_init; the `pairs` of msfm_match_pairs.
 * msfm_wordset_create does everything that does not depend on the options once - word tables, similarity matrix, ranked
 * hypotheses, keypoints - and keeps it on the device; a set counts as a child of its context.  max_hypotheses = 0: the rule
 * of :168-169, min(max(200, n / 10), n - 1) capped at 500; > 0: that many (<= n - 1).  word_id and keypoints are flat over
 * all images back to back; the word rows of an image with has_words = 0 are ignored.
 * msfm_wordset_size: n_inverted = images entered into bins before the stop rule, n_mapped = word-table entries.
 * msfm_wordset_fetch (every pointer may be NULL): similarity [n][n], hyp_img / hyp_sim [n][K], map_off [n + 1],
 * map_word / map_feat [n_mapped] (image i's table is map_off[i] .. map_off[i + 1], ascending word).
 * msfm_pair_select answers rows [first_image, first_image + n_rows) with one host wait for the offsets and one for the
 * answer (plus those of the RANSAC); options.max_hypotheses = 0: the set's K, else the first that many slots (<= K).
 * msfm_pair_set_fetch (every pointer may be NULL): n_init / n_inliers / verdict [rows][K], pairs [n_kept][2], F [rows][K][9],
 * init_off [rows * K + 1], init_matches [n_init_total][2], init_inlier [n_init_total].  A pair set is host memory only.
 * MSFM_E_INVAL, the objects stay usable: a NULL pointer, n_images < 2 (or above 46340), a word id outside [0, num_words],
 * max_hypotheses out of range, first_image / n_rows out of range, a chunk whose joined matches do not fit int32. */
typedef struct msfm_wordset msfm_wordset;
typedef struct msfm_pair_set msfm_pair_set;
typedef struct msfm_pair_select_options {   /* msfm_pair_select_default_options fills the reference's values */
  int32_t th_init_matches;       /* 30 (:254) */
  int32_t th_inliers;            /* 20 (:274) */
  int32_t max_hypotheses;        /* 0 */
  msfm_fransac_options fransac;  /* msfm_fransac_default_options */
} msfm_pair_select_options;
void msfm_pair_select_default_options(msfm_pair_select_options* opt);
int msfm_wordset_create(msfm_ctx* ctx, int n_images, const int* n_features /*[n]*/, const uint8_t* has_words /*[n]*/,
                        const int32_t* word_id, int num_words /* Database::max_words_id_ */, const float* keypoints /*[..][2]*/,
                        int max_hypotheses, msfm_wordset** out);
int msfm_wordset_size(const msfm_wordset* set, int* n_images, int* n_hypotheses, int64_t* n_inverted, int64_t* n_mapped,
                      int64_t* h2d_bytes);
int msfm_wordset_fetch(const msfm_wordset* set, int32_t* similarity, int32_t* hyp_img, int32_t* hyp_sim, int32_t* map_off,
                       int32_t* map_word, int32_t* map_feat);
void msfm_wordset_destroy(msfm_wordset* set);
int msfm_pair_select(msfm_wordset* set, int first_image, int n_rows, const msfm_pair_select_options* opt, msfm_pair_set** out);
int msfm_pair_set_size(const msfm_pair_set* set, int* n_rows, int* n_hypotheses, int* n_kept, int64_t* n_init_total);
int msfm_pair_set_fetch(const msfm_pair_set* set, int32_t* n_init, int32_t* n_inliers, uint8_t* verdict, int32_t* pairs, double* F,
                        int32_t* init_off, int32_t* init_matches, uint8_t* init_inlier);
void msfm_pair_set_destroy(msfm_pair_set* set);

/* ======================================================================================
 *  The visual word of every feature: the vocabulary-tree descent
 * ====================================================================================== */
/* Database::BuildWords / GenerateWordsForImage (SfM/src/database.cc:745-867): one voc_.transform(descriptors, words_id) per
 * image, the `fBow _transform(features, word_ids)` overload of fbow::Vocabulary (SfM/thirdparty/fbow/include/fbow/fbow.h:417-452),
 * here for all images of a descriptor set at once, on the float32 rows the set holds.  The tree is the reference's: blocks of
 * up to k nodes (fbow.h:155-187), a node a 128-float descriptor, id_or_childblock (msb set: a leaf and its word id; else the
 * block of its children, fbow.h:129-137) and a weight.  Per feature:
 *   descent     start at block 0.  In the current block the nodes 0 .. N-1 are tried in order with best = 4294967296.0f
 *               (numeric_limits<uint32_t>::max() as a float); a node wins on d < best: strict, so a tie stays with the lower
 *               node and a NaN distance never wins.  A winning leaf gives word_id = its id and adds its weight to the image's
 *               bag; a winning inner node continues in its block, except that a link to block 0 ends the walk
 *               (`while (!leaf && id != 0)`, :449): such a feature keeps word id -1 and adds nothing.
 *   distance    L2_avx_generic (fbow.h:247-261): eight binary32 partial sums, element i into partial i % 8 in ascending i, as
 *               a separate subtract, multiply and add (no fused multiply-add), then ((s0+s1)+(s2+s3))+((s4+s5)+(s6+s7)).
 *               UNPINNED: which computeDist a reference build picks is decided in fbow's .cpp, which this project has never
 *               seen, and so is that build's floating-point mode; this is the form an x64 AVX build takes for 512-byte float
 *               descriptors.  The SSE and generic forms are not built.
 *   bag         fBow is a std::map<uint32_t, float>: per image the distinct words ascending, each with the binary32 sum of its
 *               features' leaf weights in feature order, from 0.0f.
 *   images      only an image with count > min_features gets words (database.cc:798: 300, strict); the others have
 *               has_words = 0, word id -1 on every feature, an empty bag - what msfm_wordset_create understands.
 *   maxima      image_max_id[i] = max(0, largest word id of image i) (:864-866); Database::max_words_id_ after image i is the
 *               running maximum of these in image order (what the `<i>_words` file records), and the last one is num_words,
 *               the num_words of msfm_wordset_create.
 *   DEPARTURE   when no node of a block wins (every distance >= 2^32 or NaN) the reference goes on with whatever index the
 *               block before, or the feature before, left in best_dist_idx.second.  Here such a feature gets word id -1, adds
 *               nothing to the bag and is counted in n_unassigned, as are the features the `id != 0` rule stops (counted for
 *               images with words only).  For finite descriptors with |value| < 2896 the case cannot arise.
 * msfm_voctree_create uploads the tree once (node_desc [n_blocks][k][128], node_link and node_weight [n_blocks][k], rows past
 * block_n[b] ignored) and stores the descriptors in the order the kernel reads them.  The tree is walked from block 0 on the
 * host first.  MSFM_E_INVAL, the context stays usable: a NULL pointer, k outside [2, 64], block_n[b] > k, a reached block with
 * no node, a child block >= n_blocks, a block reached twice or more than 32 blocks deep (the reference would not come back
 * from a cycle).  msfm_voctree_size: depth = blocks on the longest path, n_leaves = leaf nodes of the reached blocks.
 * msfm_descset_words: word ids, per-feature leaf weights, bags and maxima stay on the device inside the result; the host
 * waits once, for the bag sizes.  The result is a copy - it stays readable when the set changes - and remembers the set's
 * generation.  msfm_word_result_fetch (every pointer may be NULL): feat_off [n + 1], has_words [n], word_id [n_features],
 * image_max_id [n], bow_off [n + 1], bow_word / bow_weight [n_bow] (image i's bag is bow_off[i] .. bow_off[i + 1]).
 * msfm_wordset_create_from_words builds the set of msfm_wordset_create device to device: word ids and num_words from the result,
 * keypoints from the set's msfm_descset_upload_keypoints; array for array the set msfm_wordset_create makes of the fetched ids
 * and the same keypoints; msfm_wordset_size reports the few bytes it sends.  MSFM_E_INVAL: an image with words but no
 * keypoints, a result older than the set's last descriptor upload, n_unassigned > 0 (the reference would index its inverted
 * file at -1), n_images < 2, max_hypotheses out of range.  Trees, results and sets count as children of their context. */
typedef struct msfm_voctree msfm_voctree;
int msfm_voctree_create(msfm_ctx* ctx, int k, int n_blocks, const uint16_t* block_n /*[n_blocks]*/,
                        const float* node_desc /*[n_blocks][k][128]*/, const uint32_t* node_link /*[n_blocks][k]*/,
                        const float* node_weight /*[n_blocks][k]*/, msfm_voctree** out);
int msfm_voctree_size(const msfm_voctree* tree, int* k, int* n_blocks, int* depth, int64_t* n_leaves, int64_t* h2d_bytes);
void msfm_voctree_destroy(msfm_voctree* tree);
typedef struct msfm_word_result msfm_word_result;
int msfm_descset_words(msfm_descset* set, const msfm_voctree* tree, int min_features /* 300 */, msfm_word_result** out);
int msfm_word_result_size(const msfm_word_result* res, int* n_images, int64_t* n_features, int64_t* n_bow, int* num_words,
                          int64_t* n_unassigned);
int msfm_word_result_fetch(const msfm_word_result* res, int32_t* feat_off, uint8_t* has_words, int32_t* word_id, int32_t* image_max_id,
                           int32_t* bow_off, int32_t* bow_word, float* bow_weight);
void msfm_word_result_destroy(msfm_word_result* res);
int msfm_wordset_create_from_words(msfm_descset* set, const msfm_word_result* res, int max_hypotheses, msfm_wordset** out);

/* ======================================================================================
 *  Building the vocabulary tree: level-wide hierarchical k-means on a descriptor set
 * ====================================================================================== */
/* Database::BuildVocabularyTree (SfM/src/database.cc:655-677): fbow::VocabularyCreator::create over the descriptors of every
 * image_step-th image, here on the float32 rows a descriptor set already holds.  The result is an ordinary msfm_voctree, made on
 * the device in the layout the descent reads: no tree byte crosses PCIe, and msfm_voctree_size reports h2d_bytes = 0 for it.
 * PARITY IS UNPINNED.  fbow's vocabulary_creator.cpp is not in the reference tree; its header names Params{k, L, nthreads,
 * maxIters = 11}, getInitialClusterCenters, assignToClusters, recomputeCenters, a stop on an unchanged assignment hash and
 * feat_idx leaves for nodes too small to split, and the reference seeds from the C library's generator on three racing
 * threads, so a reference run does not reproduce itself.  What is restated is the published algorithm those names stand for -
 * k-means++ seeding, Lloyd iterations, recursion to L levels - with the definitions below, which are this project's and are
 * chosen so that the result does not depend on how the device schedules the work.  tests/voctrain_ref.py and
 * tests/voctrain_ref.cpp restate them; the device reproduces them bit for bit.
 *   sample      the images 0, image_step, 2 image_step, ... (database.cc:658-668) with all their features, whatever their count
 *               (the 300-feature rule belongs to BuildWords); the features are numbered s = 0, 1, ... in that order.
 *   distance    the descent's, exactly (above): eight unfused partial sums, ((s0+s1)+(s2+s3))+((s4+s5)+(s6+s7)); a member goes
 *               to the centre that wins with a strict < in centre order, so a tie stays with the lower cluster.  Sampled values
 *               are finite with |value| < 2896, the bound under which the descent's best = 2^32 start can never matter:
 *               training and descent agree on every distance.
 *   scales      maxabs = the largest |value| of the sample (an integer maximum over the bit patterns), e = the smallest
 *               integer with maxabs < 2^e taken from its exponent field (biased exponent - 126; -126 for zero and subnormals).
 *               E = 9 + 2 e, so 512 maxabs^2 < 2^E and every distance is below 2^E; weight_shift = 40 - E.  sum_shift S =
 *               39 - e, so maxabs 2^S < 2^39.  Both are per call, and are reported in the stats.
 *   nodes       a node is a set of sampled features in ascending s; the root holds all.  Level l = 0 .. levels - 1 processes
 *               every open node of the level together; the nodes of a level are numbered by their ordinal o = 0, 1, ...
 *               A node of m <= k members becomes a block of m leaves, node i carrying member i's descriptor.  A larger node is
 *               seeded and iterated; its non-empty clusters, in cluster order, become its block (emptied clusters are dropped,
 *               so block_n may be below k).  A cluster is a leaf when l = levels - 1 or when it has one member; every other
 *               cluster is an open node of level l + 1, in (node, cluster) order.  A node whose seeding ends with one centre
 *               becomes a block of one leaf that carries that centre (the descriptor of the drawn member).
 *   seeding     k-means++ with integer weights.  Centre 0 is member draw(0) mod m.  For centre j >= 1 every member has the
 *               weight w = (uint64) trunc(d * 2^weight_shift), d its smallest distance to the centres chosen so far (in binary64:
 *               scaling by a power of two and truncating are exact); W = the sum of w over the node.  W = 0 ends the seeding
 *               with j centres; otherwise centre j is the first member, in ascending s, whose inclusive prefix sum of w exceeds
 *               draw(j) mod W.  All sums are 64-bit integers, so any scan order gives the same draw.
 *   draw        splitmix64 (z = (x += 0x9E3779B97F4A7C15), two xor-shift-multiplies, as everywhere in this library):
 *               x = seed ^ 0x766F637472616E31; h = next(x); x = h ^ ((uint64) level << 40 | ordinal); h = next(x);
 *               x = h ^ j; draw(j) = next(x).
 *   iterations  one iteration assigns every member to its nearest centre and then recomputes the centres: a coordinate is
 *               (float)(((double) sum of q(x) / (double) count) * 2^-S) with q(x) = (int64) trunc(x * 2^S), the sum a 64-bit
 *               integer - exact for integer-valued descriptors, for others a truncation of the bits below 2^-S.  An emptied
 *               cluster keeps its centre.  A node stops after the iteration whose assignment equals the previous one's (the first
 *               never counts as equal), otherwise after max_iters iterations; either way its centres are the means of its final
 *               assignment.
 *   numbering   blocks breadth first: block 0 is the root's, the blocks of level l + 1 follow those of level l in (parent
 *               block, node) order, so no link points to block 0, which the descent treats as a stop.  Word ids run from 0 over
 *               the leaves in (block, node) order.  node_weight is 1.0f for a leaf and 0.0f for an inner node (fbow's weights are
 *               in the unseen .cpp; nothing here reads them but the bag sums).
 *   DEPARTURES  from what the creator's header implies: the stop compares the assignments themselves, not a hash of them; the
 *               seeding weights are truncated to integers; a small node's leaves carry the members' descriptors (the header's
 *               feat_idx leaves) and a node of one distinct descriptor becomes one leaf; one generator per (level, node, centre)
 *               instead of one shared by the threads.
 * msfm_descset_voctree_train: MSFM_E_INVAL, context and set stay usable: a NULL pointer, k outside [2, 64], levels outside
 * [1, 32] (the descent's depth limit), max_iters < 1, image_step < 1, no sampled feature, more than 2^23 sampled features, a
 * sampled value that is not finite or has |value| >= 2896 (values of images outside the sample are not looked at).
 * The options are plain arguments - the reference's values are k = 10, levels = 6, max_iters = 11 (fbow's Params), image_step = 1,
 * seed = 0 - and the statistics come from a getter, as the sizes of the other objects do: the header gains no struct.
 * msfm_voctree_train_stats (every pointer may be NULL; MSFM_E_INVAL for a tree that was uploaded, not trained): the sample
 * (n_images, n_features), the tree's size (n_blocks, n_leaves, depth = levels that hold a block), and per level l < depth, in
 * arrays of 32 entries, the open nodes (= blocks of the level), how many of them were iterated (level_split), the largest
 * iteration count of one of them and how many stopped at max_iters and not by an unchanged assignment (level_capped); the two
 * shifts; host_waits = the times the host waited for the stream: one for the value scan, two per level for the sizes of this and
 * of the next level, one per iteration for "is a node of this level still open" (asked at least once in a level that has a node
 * of more than k members), one at the end.
 * msfm_voctree_fetch (every pointer may be NULL) works on trained and uploaded trees alike and undoes the relay: block_n
 * [n_blocks], node_desc [n_blocks][k][128], node_link / node_weight [n_blocks][k] as msfm_voctree_create takes them, and the two
 * block fields featurefiles.write_voctree takes besides, derived from the links: block_leaf[b] = 1 where every node of block b
 * is a leaf, block_parent[b] = the block that links b (0 for block 0 and for a block nothing links). */
int msfm_descset_voctree_train(msfm_descset* set, int k /* 10 */, int levels /* 6 */, int max_iters /* 11 */, int image_step /* 1 */,
                               uint64_t seed, msfm_voctree** out);
int msfm_voctree_train_stats(const msfm_voctree* tree, int* n_images, int64_t* n_features, int* n_blocks, int64_t* n_leaves, int* depth,
                             int* weight_shift, int* sum_shift, int* host_waits, int32_t* level_nodes /*[32]*/,
                             int32_t* level_split /*[32]*/, int32_t* level_max_iters /*[32]*/, int32_t* level_capped /*[32]*/);
int msfm_voctree_fetch(const msfm_voctree* tree, uint16_t* block_n, float* node_desc, uint32_t* node_link, float* node_weight,
                       uint16_t* block_leaf, uint32_t* block_parent);

/* ======================================================================================
 *  Describing given SIFT frames: image to resident descriptor rows
 * ====================================================================================== */
/* The given-frames arm of Database::ExtractImageFeatures (SfM/src/database.cc:289-349), that is VLSiftExtractor::initialize
 * (SfM/src/feature/feature_extractor_vl_sift.h:41-71, the stretch) and VLSiftExtractor::run_sift with nikeys >= 0
 * (feature_extractor_vl_sift.cpp:75-216; :150-169 vl_sift_keypoint_init on a supplied (x, y, sigma, angle), :182
 * vl_sift_calc_keypoint_descriptor, :183 transpose_descriptor, :202 the factor 512): the Gaussian scale space of a uint8 image,
 * its gradients, and the 4 x 4 x 8 descriptor of every given frame, written straight into a descriptor set.  The DoG detector
 * and the orientation histogram follow in the next section; o_min = -1 upsampling and the CUDA-SIFT arm are not built.
 * PARITY IS UNPINNED.  VLFeat's sift.c / imopv.c are not in the reference tree (only vl/sift.h and import libraries).  The
 * definitions below are this project's; where they differ from VLFeat's, these hold.  They are chosen so that the result depends
 * neither on the device's scheduling nor on a library's transcendental functions: tests/sift_ref.cpp and tests/sift_ref.py
 * restate them and the device reproduces them bit for bit.
 *   arithmetic  binary32 on the device, every + - * / sqrtf rounded on its own (never contracted), / and sqrtf correctly
 *               rounded.  EPS = 1.19209290e-07f (2^-23), PI2 = 6.28318548f.  S = n_levels, O = n_octaves, levels s = -1 .. S + 1.
 *   host data   what needs exp, pow, log2, fmod, sin or cos is computed once on the host in binary64 with the C library, rounded
 *               to binary32, and used as data: the taps of every blur, the table T[i] = exp(-i * 25.0 / 256.0), i = 0 .. 256, and
 *               per frame (o, is, thr, st, ct).  k = pow(2, 1.0 / S), sigma0 = 1.6 * k, dsigma0 = sigma0 * sqrt(1 - 1 / (k * k)).
 *               The blur of level -1 is sd(-1) = sqrt(sa * sa - 0.25) with sa = sigma0 * pow(k, -1.0); of level s >= 0 it is
 *               sd(s) = dsigma0 * pow(k, (double) s): the same in every octave.
 *   stretch     (feature_extractor_vl_sift.h:51-62) p = (float(v) - fmin) / frange * 255.0f in that order, fmin and frange = max - min from an
 *               integer reduction over the width x height pixels (the bytes between width and stride are not looked at).
 *   blur by sd  W = max((int) ceil(4 sd), 1); g[i] = exp(-0.5 * (i - W)^2 / (sd * sd)), i = 0 .. 2W, divided by their sum (added
 *               in ascending i) in binary64, then rounded.  out(x) = ((0 + g[0] a_0) + g[1] a_1) + ... in ascending i with
 *               a_i = src[clamp(x + i - W, 0, w - 1)]: rows first, then the columns of that result with the same rule on y.
 *   octaves     octave o is (width >> o) x (height >> o).  Level (0, -1) is the stretched image blurred by sd(-1); level s is
 *               level s - 1 blurred by sd(s); level (o + 1, -1) is the pixels (2x, 2y) of level (o, S - 1).
 *   gradient    on the levels 0 .. S - 1: gx = 0.5f * (I[x + 1] - I[x - 1]) inside, I[1] - I[0] and I[w - 1] - I[w - 2] at the
 *               borders, gy likewise; mod = sqrtf(gx * gx + gy * gy).  angle in [0, PI2): ax = |gx|, ay = |gy|,
 *               mx = max(ax, ay), mn = min(ax, ay); mx = 0 gives 0; otherwise t = mn / mx, q = t * t,
 *               r = t * (c1 + q * (c3 + q * (c5 + q * (c7 + q * (c9 + q * c11))))) with c1 = 0.99997726f, c3 = -0.33262347f,
 *               c5 = 0.19354346f, c7 = -0.11643287f, c9 = 0.05265332f, c11 = -0.01172120f (the published degree-11 odd
 *               polynomial for atan on [0, 1], error below 2e-5 rad); if ay > ax: r = 1.57079637f - r; if gx < 0:
 *               r = 3.14159274f - r; if gy < 0: r = PI2 - r; if r >= PI2: r = r - PI2.
 *   frame       (x, y, sigma, theta) as binary32, widened to binary64: phi = log2((sigma + 2^-23) / sigma0),
 *               o = clamp(floor(phi - (-1 + 0.5) / S), 0, O - 1), is = clamp(floor(S * (phi - o) + 0.5), 0, S - 1);
 *               thr = fmod(theta, 6.283185307179586), plus that constant when negative; st = sin(theta), ct = cos(theta); thr, st
 *               and ct rounded to binary32.
 *   descriptor  on level (o, is) of w x h pixels: x' = x / 2^o, y' = y / 2^o, sigma' = sigma / 2^o; xf = x' + 0.5f,
 *               yf = y' + 0.5f.  The row is zero unless -1 < xf < w and -1 < yf < h - 1 (that is, unless xi = (int) xf, yi = (int) yf
 *               have 0 <= xi < w and 0 <= yi < h - 1).  SBP = 3.0f * sigma' + EPS, Wf = floorf(1.41421356f * SBP * 2.5f + 0.5f),
 *               W = Wf < 32768 ? (int) Wf : 32768.  The pixels (xi + dxi, yi + dyi), dyi = max(-W, 1 - yi) .. min(W, h - yi - 2)
 *               and inside it dxi = max(-W, 1 - xi) .. min(W, w - xi - 2), are visited in that (raster) order.  At pixel (px, py):
 *                 dx = float(px) - x', dy = float(py) - y';  nx = (ct * dx + st * dy) / SBP,  ny = ((-st) * dx + ct * dy) / SBP
 *                 th = angle - thr; if th < 0: th = th + PI2; if th >= PI2: th = th - PI2;  nt = (8.0f * th) / PI2
 *                 u = ((nx * nx + ny * ny) * 0.125f) * 10.24f; the pixel is skipped unless u < 256; i = (int) u, f = u - float(i),
 *                 win = T[i] + f * (T[i + 1] - T[i])
 *                 bx = floorf(nx - 0.5f), by = floorf(ny - 0.5f), bt = floorf(nt); the pixel is skipped unless -3 <= bx <= 1 and
 *                 -3 <= by <= 1;  rx = nx - (bx + 0.5f), ry = ny - (by + 0.5f), rt = nt - bt
 *                 wx[0] = |1.0f - rx|, wx[1] = |rx|, wy and wt likewise; for dbx, dby, dbt in {0, 1} with -2 <= bx + dbx <= 1 and
 *                 -2 <= by + dby <= 1 the value (((win * mod) * wx[dbx]) * wy[dby]) * wt[dbt] is added to
 *                 bin ((bt + dbt) mod 8) + 8 (bx + dbx + 2) + 32 (by + dby + 2).
 *               Each bin is the sum, from 0, of its contributions in the order of the pixels (two contributions of one pixel never
 *               share a bin).  Then n = sqrtf(sum of h[b] * h[b], b ascending from 0) + EPS, h = h / n, h = min(h, 0.2f), n again
 *               the same way, h = h / n; the value of bin t + 8 i + 32 j goes to column ((8 - t) mod 8) + 8 i + 32 (3 - j)
 *               (transpose_descriptor, :37-53) as 512.0f * h, or with quantize as min(float((int) (512.0f * h)), 255.0f).
 * A scale space is a child of its context and keeps the GSS levels and the gradient levels of every octave, nothing else.
 * msfm_scalespace_create: MSFM_E_INVAL for a NULL pointer, width or height < 2 or > 16384, stride < width, n_octaves or n_levels
 * outside [1, 8], min(width, height) >> (n_octaves - 1) < 2, a constant image; MSFM_E_NOMEM when the levels do not fit.
 * msfm_scalespace_fetch: kind 0 a GSS level, level in [-1, S + 1]; kind 1 / 2 the gradient modulus / angle, level in [0, S - 1];
 * out [h_o][w_o] float.  msfm_scalespace_size: the octave's size and the bytes create sent (image, taps, table).
 * msfm_descset_describe replaces the image's descriptors AND keypoints (xy = the frames' x, y) by the route
 * msfm_descset_upload takes - integrality flag, largest |value|, int8 forms, generation, stale match results - device to
 * device: no descriptor byte crosses PCIe, h2d_bytes (optional) counts the frames and the per-frame host values.
 * MSFM_E_INVAL, found before the first write, set and scale space stay usable: a NULL pointer, n < 0 or n > 65535, a non-finite
 * frame value, sigma <= 0, an image outside the set, set and scale space of different contexts (a set of dim != 128 does not
 * exist: msfm_descset_create refuses it).
 * msfm_descset_fetch: the image's rows [count][128] and keypoints [count][2]; either may be NULL. */
typedef struct msfm_scalespace msfm_scalespace;
int msfm_scalespace_create(msfm_ctx* ctx, const uint8_t* gray, int width, int height, int stride, int n_octaves /* 4 */,
                           int n_levels /* 5 */, msfm_scalespace** out);
int msfm_scalespace_fetch(const msfm_scalespace* ss, int octave, int level, int kind, float* out);
int msfm_scalespace_size(const msfm_scalespace* ss, int octave, int* w, int* h, int64_t* h2d_bytes);
void msfm_scalespace_destroy(msfm_scalespace* ss);
int msfm_descset_describe(msfm_descset* set, int image, const msfm_scalespace* ss, const float* frames /*[n][4]: x, y, sigma, angle*/,
                          int n, int quantize, int64_t* h2d_bytes);
int msfm_descset_fetch(const msfm_descset* set, int image, float* desc /*[count][128]*/, float* xy /*[count][2]*/);

/* ======================================================================================
 *  Detecting SIFT keypoints: DoG extrema and orientations to frames
 * ====================================================================================== */
/* The detecting arm of VLSiftExtractor::run_sift, nikeys < 0 (feature_extractor_vl_sift.cpp:130-136 vl_sift_detect, :171-173
 * vl_sift_calc_keypoint_orientations), on a scale space made above, with the reference's parameters as defaults
 * (feature_extractor_vl_sift.cpp:80-86): peak_thresh 0, edge_thresh 10, 36 orientation bins, at most 4 angles per keypoint,
 * o_min = 0.  PARITY IS UNPINNED as above, and the same principles hold: binary32 on the device with every operation rounded on
 * its own, no library transcendental on the device, nothing depends on the device's scheduling, what needs pow is computed on the
 * host in binary64 with the C library and used as data.  tests/siftdetect_ref.cpp restates what follows.
 *   DoG         D(o, s) = G(o, s + 1) - G(o, s), s = -1 .. S, one subtraction per value.  No plane of D is kept: the kernels form
 *               it from the resident levels where they need it, and the scale space object holds what it held before.
 *   extrema     on the levels s = 0 .. S - 1 and the pixels x = 1 .. w - 2, y = 1 .. h - 2 of every octave.  With v = D(x, y, s),
 *               t = 0.8f * peak_thresh and the 26 neighbours n = D(x + i, y + j, s + k), (i, j, k) in {-1, 0, 1}^3 \ {0}: a maximum
 *               has v > n for all of them and v >= t, a minimum v < n for all of them and v <= -t.  Ties are not extrema.
 *   refinement  of a candidate (x, y, s), at most 5 passes.  A pass, with d(i, j, k) = D(x + i, y + j, s + k):
 *                 Dx = 0.5f * (d(1,0,0) - d(-1,0,0)), Dy and Ds likewise;  Dxx = (d(1,0,0) + d(-1,0,0)) - 2.0f * d(0,0,0), Dyy and
 *                 Dss likewise;  Dxy = 0.25f * (((d(1,1,0) + d(-1,-1,0)) - d(-1,1,0)) - d(1,-1,0)), Dxs and Dys likewise (Dxs from
 *                 (1,0,1), (-1,0,-1), (-1,0,1), (1,0,-1); Dys from (0,1,1), (0,-1,-1), (0,-1,1), (0,1,-1)).
 *                 A = [Dxx Dxy Dxs; Dxy Dyy Dys; Dxs Dys Dss], b = (-Dx, -Dy, -Ds).  Gaussian elimination, for j = 0, 1, 2: the
 *                 pivot row is the first i >= j with the largest |A(i, j)| (a later row replaces it only when strictly larger); a
 *                 largest |A(i, j)| of 0 sets b = (0, 0, 0) and ends the elimination; else rows i and j are exchanged from column j
 *                 on, A(j, jj) = A(j, jj) / p for jj = j .. 2 and b(j) = b(j) / p with p the pivot's value, and for ii > j, with
 *                 f = A(ii, j): A(ii, jj) = A(ii, jj) - f * A(j, jj), jj = j .. 2, b(ii) = b(ii) - f * b(j).  Back substitution:
 *                 for i = 2, 1 and ii = i - 1 .. 0: b(ii) = b(ii) - b(i) * A(ii, i).
 *                 mx = +1 if b(0) > 0.6f and x < w - 2, -1 if b(0) < -0.6f and x > 1, else 0; my likewise from b(1), y and h.  If both
 *                 are 0 the loop ends; after the fifth pass it ends anyway (the keypoint is then `unconverged`); otherwise
 *                 x = x + mx, y = y + my (never s) and the next pass follows.  A keypoint whose (x, y) has changed has `moved`.
 *               With the last pass's values: val = d(0,0,0) + 0.5f * ((Dx * b(0) + Dy * b(1)) + Ds * b(2)),
 *               score = ((Dxx + Dyy) * (Dxx + Dyy)) / (Dxx * Dyy - Dxy * Dxy), xn = float(x) + b(0), yn = float(y) + b(1),
 *               sn = float(s) + b(2), bound = (float) ((e + 1) * (e + 1) / e) with e = (double) edge_thresh.  The candidate is
 *               rejected by the first of these that does not hold, each written so that a NaN fails it:
 *                 peak    |val| > peak_thresh                     edge    score < bound                  negative  score >= 0
 *                 offset  |b(0)|, |b(1)|, |b(2)| all < 1.5f        bounds  0 <= xn <= w - 1, 0 <= yn <= h - 1, -1 <= sn <= S + 1
 *               and is otherwise the raw keypoint (o, ix, iy, is, xn, yn, sn) with (ix, iy) the last pass's (x, y) and is = s.
 *   orientation of a raw keypoint, on the gradient planes of its (o, is).  Host: sigmaw = (float) (1.5 * sigma0 * pow(2, sn / S))
 *               in binary64 with sn widened.  The device makes the raw keypoints, the host this number, the device the angles: two
 *               device passes around one host step.  xi = (int) (xn + 0.5f), yi = (int) (yn + 0.5f), W = (int) floorf(3.0f * sigmaw).
 *               The pixels (xi + dxi, yi + dyi) with the descriptor's clipping, dyi = max(-W, 1 - yi) .. min(W, h - yi - 2) and
 *               inside it dxi = max(-W, 1 - xi) .. min(W, w - xi - 2), in that (raster) order.  At pixel (px, py):
 *                 dx = float(px) - xn, dy = float(py) - yn, r2 = dx * dx + dy * dy; skipped unless r2 < float(W * W) + 0.6f
 *                 u = (r2 / ((2.0f * sigmaw) * sigmaw)) * 10.24f; skipped unless u < 256; i = (int) u, f = u - float(i),
 *                 win = T[i] + f * (T[i + 1] - T[i]), v = win * mod
 *                 fb = (36.0f * angle) / PI2, bf = floorf(fb - 0.5f), rb = fb - (bf + 0.5f), ib = ((int) bf + 36) mod 36
 *                 (1.0f - rb) * v is added to bin ib and rb * v to bin (ib + 1) mod 36.
 *               Each bin is the sum, from 0, of its contributions in the order of the pixels.  Then six times, from the old values:
 *               h[i] = ((h[(i + 35) mod 36] + h[i]) + h[(i + 1) mod 36]) / 3.0f.  m = the largest h.  Bin i is a peak when
 *               h[i] > 0.8f * m, h[i] > hm and h[i] > hp, with hm = h[(i + 35) mod 36], hp = h[(i + 1) mod 36]; then
 *               di = (-0.5f * (hp - hm)) / ((hp + hm) - 2.0f * h[i]), theta = (PI2 * ((float(i) + di) + 0.5f)) / 36.0f.  The first
 *               four peaks in ascending i are the keypoint's angles (it may have none).
 *   frames      on the host, per raw keypoint and angle: x = xn * 2^o, y = yn * 2^o (binary32, exact),
 *               sigma = (float) (1.6 * pow(2, 1.0 / S) * pow(2, o + (double) sn / S)), angle = theta: the [n][4] frames
 *               msfm_descset_describe takes.  ONE DEPARTURE from the reference: the descriptor of such a frame is the one of the
 *               section above, with (o, is) derived from sigma by its frame rule, not the detection's (o, is); so extract equals
 *               detect followed by describe bit for bit and there is one descriptor definition.
 *   order       frames are ordered by ascending (o, is, iy, ix) of the cell the extremum was DETECTED in, then by ascending
 *               bin; two extrema that refine to the same place both stay.  Positions come from a scan over the extremum masks
 *               and ordered compaction, never from the arrival order of an atomic.
 *   capacity    max_frames in [0, 65535] (what one describe call takes).  n_found counts every frame; when it exceeds max_frames
 *               the first max_frames in the order above are returned.  The candidate buffers are sized from a count pass with
 *               one host wait; no buffer is sized by a guess.
 * msfm_scalespace_detect: frames_out [max_frames][4] receives *n_out = min(n_found, max_frames) frames.  It waits three times: for
 * the candidate count, for the raw keypoints (the host step above, which also compacts the accepted ones in order and counts the
 * rejections), for the angles.  stats (optional) [MSFM_SIFT_DETECT_STATS]: 0 candidates; rejected by 1 peak, 2 edge, 3 negative
 * score, 4 offset, 5 bounds; 6 keypoints; 7 n_found; 8 .. 12 keypoints with 0 .. 4 angles; 13 keypoints that moved; 14 keypoints
 * unconverged; 15 host waits; 16 bytes to the device; 17 bytes from the device.
 * msfm_descset_extract: that detection, then its frames through msfm_descset_describe's own route into the image of the set; stats
 * as above with describe's waits and bytes added.
 * MSFM_E_INVAL, found before the first write, set and scale space stay usable: a NULL pointer (stats may be NULL), a non-finite or
 * negative threshold, max_frames outside [0, 65535], an image outside the set, set and scale space of different contexts. */
#define MSFM_SIFT_DETECT_STATS 18
int msfm_scalespace_detect(const msfm_scalespace* ss, float peak_thresh /* 0 */, float edge_thresh /* 10 */, int max_frames,
                           float* frames_out /*[max_frames][4]*/, int* n_out, int64_t* stats /*[MSFM_SIFT_DETECT_STATS]*/);
int msfm_descset_extract(msfm_descset* set, int image, const msfm_scalespace* ss, float peak_thresh, float edge_thresh, int max_frames,
                         int quantize, int64_t* stats /*[MSFM_SIFT_DETECT_STATS]*/);

/* ======================================================================================
 *  Stereo rectification: geometry on the host, maps and bilinear warp on the device
 * ====================================================================================== */
/* DenseReconstruction::EpipolarRectification (SfM/src/dense_reconstruction.cc:299-331): cv::stereoRectify, two
 * cv::initUndistortRectifyMap and two cv::remap(INTER_LINEAR), the first step per pair of SGMDense (:134) and of ELASDense (:226).
 * PARITY WITH OPENCV IS UNPINNED: the calib3d and imgproc sources are not in the reference tree and no build of them has been run
 * against this.  THE DEFINITIONS BELOW ARE THIS PROJECT'S OWN; where they differ from OpenCV, they hold.  Everything past the map
 * is integer arithmetic and the map is unfused binary64 without a library function on the device, so tests/rectify_ref.cpp restates
 * geometry, maps and warp sequentially and the device equals it bit for bit in every plane msfm_rectifier_fetch returns.
 * Camera 1 is the reference's left image i + 1, camera 2 its right image i.  All host arithmetic is binary64, every product and
 * sum rounded on its own, a three-term sum as (a + b) + c; acos, sin, cos and sqrt are the host C library's, and their results are
 * used as data.  Matrices are row-major.
 *
 * msfm_stereo_rectify: host only, no context (like msfm_camera_graph_dissection).  cv::stereoRectify with zero distortion,
 * CALIB_ZERO_DISPARITY, alpha = -1 and newImageSize = imageSize (dense_reconstruction.cc:308-314).
 *   relative    R21 = R2 inv(R1), the 3 x 3 inverse by the adjugate (every cofactor divided by the determinant);
 *               t21 = -(R21 t1) + t2.  The pose file's header calls t a camera position (:342), the reference passes it as a
 *               translation (:309): KEPT.
 *   halves      om = the rotation vector of R21: c = clamp((trace - 1) / 2, -1, 1), theta = acos(c), r = the skew part
 *               ((R21[2][1] - R21[1][2]) / 2, ...), om = r * (theta / |r|), 0 when |r| = 0.  DEPARTURE 1: no SVD clean-up of R21
 *               is done, and theta has acos's resolution (1e-8 rad beside theta = 0).  rodrigues(v), theta = |v|, k = v / theta:
 *               cos(theta) I + (1 - cos(theta)) k k^T + sin(theta) [k]x, the identity for v = 0.  r_r = rodrigues(-0.5 om);
 *               t = r_r t21.
 *   axis        idx = |t[0]| > |t[1]| ? 0 : 1 (0: a horizontal pair, 1: a vertical one); c = t[idx]; nt = |t|; uu = 0 but for
 *               uu[idx] = c > 0 ? 1 : -1; ww = t x uu; nw = |ww|; if nw > 0, ww *= acos(|c| / nt) / nw; wR = rodrigues(ww).
 *   rotations   R1_ = wR r_r^T, R2_ = wR r_r, t_rect = R2_ t21 (only its idx component is not roundoff).
 *   focal       fc = min(K1[idx^1][idx^1], K2[idx^1][idx^1]).
 *   centre      per camera k the corners (0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1): n = ((x - cx) / fx, (y - cy) / fy, 1),
 *               p = Rk_ n, (p.x / p.z) * fc and (p.y / p.z) * fc, summed in that order and times 0.25: avg.
 *               cc_k = ((w - 1) / 2 - avg.x, (h - 1) / 2 - avg.y); zero disparity: cc = (cc_1 + cc_2) * 0.5 for both cameras.
 *   outputs     P1_ = [fc 0 cc.x 0; 0 fc cc.y 0; 0 0 1 0]; P2_ the same with P2_[idx][3] = t_rect[idx] * fc;
 *               Q = [1 0 0 -cc.x; 0 1 0 -cc.y; 0 0 0 fc; 0 0 -1 / t_rect[idx] 0].  Every output pointer is optional.
 *   KEPT        when camera 1 is not the left one, P2_[0][3] > 0 and every true disparity is negative, so the matching behind it
 *               finds nothing.  The reference does not look either; dense.sgm_dense_posed returns the sign per pair.
 * MSFM_E_INVAL before any write: a NULL input; a non-finite value; K[0][0] or K[1][1] of either camera not positive; nt == 0
 * (no baseline); a relative rotation within 1e-6 of pi (the skew part has lost the axis); width or height outside [1, 16384];
 * an R1 without an inverse, or poses that give a non-finite output.
 *
 * maps         cv::initUndistortRectifyMap with zero distortion and CV_32FC1, per camera k and output pixel, column j, row i.
 *               On the host iR = inv(Pk_[:, :3] Rk_) by the adjugate.  On the device in unfused binary64:
 *               X = (iR[0][0] * j + iR[0][1] * i) + iR[0][2], Y and W likewise from rows 1 and 2; wi = 1.0 / W;
 *               mapx = (float)(fx * (X * wi) + cx), mapy = (float)(fy * (Y * wi) + cy) with the camera's own K, whose skew entry
 *               is ignored.  DEPARTURE 2: OpenCV accumulates X, Y and W along the row by repeated addition; here every pixel is
 *               evaluated directly, so no pixel depends on its neighbour.
 * warp         cv::remap(INTER_LINEAR) on uint8 with BORDER_CONSTANT 0, as its 5-bit fixed-point arithmetic, in integers.
 *               px = mapx * 32.0f, py = mapy * 32.0f (binary32, exact).  If either is not finite or of magnitude >= 2^30 the
 *               pixel is 0.  Otherwise sx = rint(px) (half to even), ix = sx >> 5 (arithmetic), ax = sx & 31; sy, iy, ay likewise.
 *               S = (32 - ax)(32 - ay) p00 + ax (32 - ay) p01 + (32 - ax) ay p10 + ax ay p11, p00 = src(ix, iy), p01 = src(ix + 1,
 *               iy), p10 = src(ix, iy + 1), p11 = src(ix + 1, iy + 1); a tap outside the source counts 0, each tap on its own.
 *               out = (S + 512) >> 10.  This equals OpenCV's table of 15-bit weights: a product of two 5-bit fractions times
 *               2^15 is an integer, so the table rounds nothing.
 * NOT BUILT: distortion coefficients (the reference passes zeros); alpha >= 0; a new image size; colour input for the ELASDense
 * arm; ELASDense itself; Depth2Points; a C++ host mirror.
 *
 * msfm_rectifier is a child of its context like msfm_sgm, made for one image size.  It owns the parameter block of a call
 * (2 cameras x (iR, fx, fy, cx, cy) = 208 bytes) with the two source planes behind it, the two rectified planes [2][h][w], and
 * four float map planes; msfm_rectifier_size reports them (208 + 20 w h bytes), the SGM object does not.
 * msfm_rectifier_rectify does the geometry on the host (MSFM_E_INVAL as above, before anything is staged), copies block and pair
 * into pinned staging of the object, uploads them in one copy and enqueues ONE launch for both images on the context's stream; it
 * does NOT wait, and the caller's buffers are free on return.  keep_maps != 0 also writes the four map planes.  R1_out, R2_out
 * [9], P1_out, P2_out [12] (each optional) receive the geometry.  stats (optional) [MSFM_RECTIFY_STATS], as MSFM_SGM_STATS:
 * 0 host waits, 1 bytes to the device (208 + 2 w h), 2 kernel launches (1).
 * msfm_rectifier_fetch waits and copies one plane [h][w]: kind 0 / 1 rectified left / right (uint8); 2 / 3 mapx / mapy of the
 * left image, 4 / 5 of the right (float).
 * MSFM_E_INVAL before any write, with the object still usable: a NULL pointer (stats and the geometry outputs may be NULL); a
 * side outside [1, 16384]; stride < width; a kind out of range; a fetch before the first rectify; a map fetch when the last
 * rectify kept none. */
#define MSFM_RECTIFY_STATS 3
typedef struct msfm_rectifier msfm_rectifier;
int msfm_stereo_rectify(const double K1[9], const double R1[9], const double t1[3], const double K2[9], const double R2[9],
                        const double t2[3], int width, int height, double* R1_out /*[9]*/, double* R2_out /*[9]*/,
                        double* P1_out /*[12]*/, double* P2_out /*[12]*/, double* Q_out /*[16]*/, int* idx_out);
int msfm_rectifier_create(msfm_ctx* ctx, int width, int height, msfm_rectifier** out);
int msfm_rectifier_rectify(msfm_rectifier* rect, const uint8_t* left, int left_stride, const uint8_t* right, int right_stride,
                           const double K1[9], const double R1[9], const double t1[3], const double K2[9], const double R2[9],
                           const double t2[3], int keep_maps, double* R1_out /*[9]*/, double* R2_out /*[9]*/,
                           double* P1_out /*[12]*/, double* P2_out /*[12]*/, int64_t* stats /*[MSFM_RECTIFY_STATS]*/);
int msfm_rectifier_fetch(const msfm_rectifier* rect, int kind, void* out);
int msfm_rectifier_size(const msfm_rectifier* rect, int* width, int* height, int64_t* device_bytes);
void msfm_rectifier_destroy(msfm_rectifier* rect);

/* ======================================================================================
 *  Dense stereo: census, eight-path semi-global matching, disparity to depth
 * ====================================================================================== */
/* DenseReconstruction::SGMDense (SfM/src/dense_reconstruction.cc:113-190): sgm::StereoSGM::execute of libSGM
 * (SfM/src/dense/cudasgm) on a rectified pair of uint8 images, width x height, each with its own stride, and the disparity turned
 * into a depth image.  D = disp_size is 64 or 128; the reference's call (dense_reconstruction.cc:154-155, basic_structs.h:240-241)
 * is P1 = 10, P2 = 120, uniqueness 0.96, D = 128, 8-bit input, 8-bit output, no subpixel.  THE DEFINITIONS BELOW ARE RESTATED FROM
 * READING libSGM's sources; every kept behaviour cites its file and line; no build of those sources has been run against them.
 * The arithmetic is integer but for one binary32 product, nothing depends on the device's scheduling, and tests/sgm_ref.cpp
 * restates what follows sequentially: the device equals it byte for byte in every plane msfm_sgm_fetch returns.
 *   census      uint32, for the left and the right image (census_transform.cu:31-119, the 9 x 7 symmetric form).  For a pixel with
 *               4 <= x < width - 4 and 3 <= y < height - 3 the value has 31 bits: from f = 0, first for dy = -3, -2, -1 and inside
 *               it dx = -4 .. 4, then for dy = 0 and dx = -4 .. -1:  f = (f << 1) | (I(x + dx, y + dy) > I(x - dx, y - dy)).
 *               Every other pixel has census 0.  DEPARTURE 1: the reference never writes these border features and leaves the
 *               buffer as it came from the allocator.
 *   cost        C(x, y, d) = popcount(census_L(x, y) ^ census_R(x - d, y)), d = 0 .. D - 1; census_R is 0 where x - d < 0.
 *   paths       eight, r = 0 (+1, 0), 1 (-1, 0), 2 (0, +1), 3 (0, -1), 4 (+1, +1), 5 (-1, +1), 6 (-1, -1), 7 (+1, -1)
 *               (path_aggregation.cu).  With q = p - r: if q is outside the image, L_r(p, d) = C(p, d); otherwise, with
 *               m = min_e L_r(q, e):  L_r(p, d) = C(p, d) + min(L_r(q, d) - m, L_r(q, d - 1) - m + P1, L_r(q, d + 1) - m + P1, P2),
 *               the d - 1 and d + 1 terms only inside [0, D) (path_aggregation_common.hpp:47-89).  Unsigned 32-bit inside the
 *               recurrence, stored as one byte: L <= 31 + P2.  DEPARTURE 2: P2 > 224, P1 > P2 or a negative value is
 *               MSFM_E_INVAL; the reference would silently truncate to 8 bits.
 *   sum         S(x, y, d) = the sum of L_r over the eight paths, uint16.
 *   left        among key(d) = (S(x, y, d) << 16) | d the two smallest keys k0 < k1, so equal costs go to the lower disparity
 *               (winner_takes_all.cu:100-113, :139-227).  c0 = k0 >> 16, d0 = k0 & 0xffff, c1, d1 likewise.  float(c1) * uniqueness
 *               is one binary32 multiplication.  dispL = d0 if that product is >= float(c0); otherwise d0 if |d1 - d0| <= 1;
 *               otherwise 0.
 *   right       for the right pixel p the same rule on the keys (S(p + d, y, d) << 16) | d over d = 0 .. min(D - 1, width - 1 - p);
 *               with a single candidate the second key is 0xffffffff (winner_takes_all.cu:228-261).  DEPARTURE 3: width < D is
 *               MSFM_E_INVAL; the reference's final flush writes in front of the row there.
 *   median      of both disparity planes, uint16: for 1 <= x <= width - 2 and 1 <= y <= height - 2 the median of the 3 x 3
 *               neighbourhood; every other pixel is 0 (median_filter.cu:111-125: the output buffer is zeroed once and never written there).
 *   consistency on the median-filtered left plane, only for x < 16 * (width / 16) and y < 16 * (height / 16) (integer division:
 *               the reference's launch grid, check_consistency.cu:61, KEPT AS A QUIRK; pixels outside it keep the median's value).
 *               With d the left value and k = x - d the value becomes 0 when I_L(x, y) == 0, or d <= 0, or 0 <= k < width and
 *               |R_med(k, y) - d| > 1 (check_consistency.cu:22-35).  A k < 0 does not invalidate.
 *   output      the final left plane cast to uint8 (values < D <= 128).
 *   depth       dense_reconstruction.cc:160-181.  Per pixel with disp != 0: t = ((200.0 * baseline) * focal) / double(disp) in
 *               binary64; depth = t > 255 || t < 0 ? 0 : (uint8) t by truncation; disp == 0 gives 0.  The 128 values are made
 *               on the host (the division is the host's) and applied to the final plane as a table.
 * NOT BUILT: 16-bit input; the subpixel arm (its 16-bit median in the reference truncates columns to 8 bits, which would need a
 * ruling of its own); ELASDense; Depth2Points; a C++ host mirror; a multi-GPU form.  (EpipolarRectification is the section
 * above, by this project's own definitions.)
 * msfm_sgm is a child of its context like msfm_scalespace.  It owns all its device planes for its lifetime - two images, two
 * census planes, eight cost volumes [h][w][D] of uint8, four uint16 planes, the uint8 result - and is reused pair after pair, as the
 * reference reuses a StereoSGM.  MSFM_E_NOMEM when the planes do not fit (4 000 x 3 000 at D = 128: 11.5 GB of cost volumes).
 * msfm_sgm_execute copies the pair into pinned staging of the object, uploads it and enqueues everything on the context's stream;
 * it does NOT wait, and the caller's buffers are free on return.  A second execute replaces the first's result.
 * stats (optional) [MSFM_SGM_STATS]: 0 host waits (0, unless the caller is two executes ahead of the device and the staging
 * slot's copy has not run), 1 bytes to the device, 2 kernel launches.
 * msfm_sgm_execute_rectified runs the same chain on the rectified planes of a msfm_rectifier where its last rectify put them:
 * same stream, no wait, no copy; stats reports 0 waits, 0 bytes and the 7 launches.  The two executes may follow each other on
 * one object in any order.  MSFM_E_INVAL: a NULL rectifier, one of another context or another size, one that has not rectified yet.
 * msfm_sgm_fetch waits and copies one plane, [h][w] of: kind 0 / 1 census L / R (uint32); 2 the cost volume of path `index`
 * (uint8 [h][w][D]); 3 / 4 raw left / right disparity (uint16); 5 / 6 median-filtered left / right (uint16); 7 final left (uint8).
 * index is 0 for every kind but 2.  msfm_sgm_depth waits and writes the depth of the final plane.
 * MSFM_E_INVAL before any write, with the object still usable: a NULL pointer (stats may be NULL); disp_size not 64 or 128;
 * width < disp_size or > 16384; height < 1 or > 16384; stride < width; the parameter rules above; uniqueness non-finite or outside
 * [0, 1]; a fetch kind or index out of range; a non-finite baseline or focal; a fetch or depth before the first execute. */
#define MSFM_SGM_STATS 3
typedef struct msfm_sgm msfm_sgm;
int msfm_sgm_create(msfm_ctx* ctx, int width, int height, int disp_size /* 128 */, int p1 /* 10 */, int p2 /* 120 */,
                    float uniqueness /* 0.96 */, msfm_sgm** out);
int msfm_sgm_execute(msfm_sgm* sgm, const uint8_t* left, int left_stride, const uint8_t* right, int right_stride,
                     int64_t* stats /*[MSFM_SGM_STATS]*/);
int msfm_sgm_execute_rectified(msfm_sgm* sgm, const msfm_rectifier* rect, int64_t* stats /*[MSFM_SGM_STATS]*/);
int msfm_sgm_fetch(const msfm_sgm* sgm, int kind, int index, void* out);
int msfm_sgm_depth(const msfm_sgm* sgm, double baseline, double focal, uint8_t* depth_out /*[h][w]*/);
int msfm_sgm_size(const msfm_sgm* sgm, int* width, int* height, int* disp_size, int64_t* device_bytes);
void msfm_sgm_destroy(msfm_sgm* sgm);

/* ======================================================================================
 *  Which image to localise next: the batched 2D-3D correspondence search
 * ====================================================================================== */
/* A resident copy of the verified matches, so that the search below moves no match over PCIe per round (the reference
 * re-reads and parses `<i>_match` in Graph::QueryMatch, SfM/src/graph/graph.cc:92-137, per candidate x registered image).
 * pair_img[p] = (idx1, idx2) as WriteOutMatches(idx1, idx2, ...) stores it (fine_matching_graph.cc:184), matches[m] =
 * (feature in idx1, feature in idx2): the layout of msfm_tracks_build.  A feature of idx1 may occur in several matches of a
 * pair (ptr_id[0] is not unique over the queries, graph.cc:116-129): kept.  Pairs must be strictly ascending in
 * (idx1, idx2) - the reference's visiting order - and every feature index inside its image (checked on the device), else
 * MSFM_E_INVAL.  The store keeps a row index by idx1: QueryMatch(i, j) is "row i, entry j".
 * msfm_match_store_from_chain copies the matches of a verified chain (and the keypoints it holds) device to device; the
 * chain may be destroyed afterwards.  A store counts as a child of its context. */
typedef struct msfm_match_store msfm_match_store;
int msfm_match_store_create(msfm_ctx* ctx, int n_images, const int* n_features, int n_pairs,
                            const int* pair_img /*[n_pairs][2]*/, const int* match_off /*[n_pairs+1]*/,
                            const int* matches /*[match_off[n_pairs]][2]*/, msfm_match_store** out);
int msfm_match_store_from_chain(msfm_chain* chain, msfm_match_store** out);
void msfm_match_store_destroy(msfm_match_store* store);

/* The search of IncrementalSfM::FindImageToLocalize (SfM/src/sfm_incremental.cc:440-562) for a whole candidate list.
 * (Which images are candidates, :423-438, is a loop over the match graph: metricsfm_amd/localize.py::candidate_images.)
 * Per candidate image i, registered images j in ascending image id that have a store pair (i, j) with matches (:452-474),
 * that pair's matches in stored order (:480):
 *   - (f_i, f_j) qualifies when p = feat_point[cam(j)][f_j] >= 0 and !pt_bad[p] (:486-487);
 *   - it inserts f_i -> p and f_i -> pt_mse[p] + (pt_views[p] <= 2 ? 3.0 : 0.0) with std::map::insert semantics: the first
 *     qualifying match that names f_i wins, over all j (:489-496);
 *   - count_2d3d_ij counts every qualifying match, also those whose insert did not take (:497); cam(j) is visible when
 *     the count is > 5 (:503), visible cameras in the order of the walk;
 *   - correspondences ordered by that mse ascending (:517-531); std::sort leaves ties open - here they go to the lower
 *     f_i, NaN last (-0.0 = +0.0);
 *   - score = n_corr / (5 + fail_times), integer division (:543); candidates by score descending, ties to the lower
 *     image id; score 0 dropped (:552).
 * In : n_cams, cam_img[n_cams] (img_cam_map_ inverted; is_img_processed_ is true exactly for these);
 *      feat_point: for camera c, local feature f -> point id held by cams_[c]->pts_ or -1, cameras in order, camera c
 *      starting at the sum of n_features[cam_img[c']] over c' < c;  n_points, pt_bad (is_bad_estimated_), pt_mse (mse_),
 *      pt_views (cams_.size());  n_cand, cand_img (strictly ascending, none registered), fail_times (>= 0).
 *      Optional: point_xyz [n_points][3] asks for pts_w / pts_2d; the keypoints then come from the store (made from a
 *      chain) or from `keypoints`, float [sum of n_features][2] in image order (only the kept candidates' rows are read).
 * Out: a msfm_localize_set.  rank[n_kept] = indices into cand_img in output order; row r of the CSR arrays belongs to
 *      candidate rank[r]: corr_off[n_kept+1], corr_feat / corr_point [n_corr] in sorted order; vis_off[n_kept+1], vis_cam
 *      [n_visible] (camera indices).  With point_xyz: pts_w [n_corr][3], pts_2d [n_corr][2] (keypoints float -> double,
 *      :592-600) - with offsets = corr_off exactly what msfm_epnp_ransac_batch / msfm_epnpf_sweep_batch take.
 *      A candidate's rows do not depend on which other candidates are in the call.
 * feat_point >= n_points is MSFM_E_INVAL (checked on the device before anything is indexed by it).  Per call the host
 * sends feat_point, the point arrays and four integers per walked pair; h2d_bytes of msfm_localize_set_size reports it.
 * A set made with point_xyz keeps corr_point / pts_w / pts_2d on the device as well, for msfm_localize_poses below, until
 * msfm_localize_set_destroy.  A set counts as a child of its context, like a store: destroy it before the context (a
 * context destroyed first is kept alive until its last child has gone). */
typedef struct msfm_localize_problem {
  int32_t n_cams;
  const int32_t* cam_img;
  const int32_t* feat_point;
  int32_t n_points;
  const uint8_t* pt_bad;
  const double* pt_mse;
  const int32_t* pt_views;
  int32_t n_cand;
  const int32_t* cand_img;
  const int32_t* fail_times;
  const double* point_xyz;   /* optional */
  const float* keypoints;    /* optional */
} msfm_localize_problem;
typedef struct msfm_localize_set msfm_localize_set;
int msfm_localize_candidates(msfm_ctx* ctx, const msfm_match_store* store, const msfm_localize_problem* problem,
                             msfm_localize_set** out);
int msfm_localize_set_size(const msfm_localize_set* set, int* n_kept, int* n_corr, int* n_visible, int* has_points,
                           int64_t* h2d_bytes);
int msfm_localize_set_fetch(const msfm_localize_set* set, int* rank, int* corr_off, int* corr_feat, int* corr_point,
                            int* vis_off, int* vis_cam, double* pts_w, double* pts_2d);
void msfm_localize_set_destroy(msfm_localize_set* set);

/* ======================================================================================
 *  Pose initialisers ahead of each bundle adjustment  
 * ====================================================================================== */
/* AbsolutePoseEstimation::AbsolutePoseWithFocalLength (SfM/src/orientation/absolute_pose_estimation.cc:42-58, called
 * when an image is localised against the model, sfm_incremental.cc:646) for a batch of images.  Per image:
 * AbsolutePoseEPNP::EPNPRansac (absolute_pose_via_epnp.cc:103-139) - `max_iter` (reference: 200) samples of 4
 * correspondences, EPnP on each (:142-185; compute_pose :472-519 with OpenCV's Jacobi SVD restated), the sample
 * whose error over its own four points is smallest is kept - then AbsolutePoseEstimation::Error over all
 * correspondences (:67-103).  The reference samples with std::random_shuffle; here sample `it` of image `p` is a
 * pure function of (seed, p, it), so results do not depend on the batch split.
 * In : offsets[n+1] delimits each image's correspondences; pts_w [total][3] world points, pts_2d [total][2] centred
 *      pixels, f[n] focal lengths.
 * Out: R [n][9] row-major and t [n][3] with Xc = R Xw + t (zeros when no sample qualified or fewer than 4 points);
 *      errors [total] = reprojection error, 1000.0 where it is >= 10 px; avg_error [n] = rms of the errors < 10 px
 *      (10000.0 when there is none) - the value compared with th_mse_localization (sfm_incremental.cc:648);
 *      best_iter [n] (may be NULL) = index of the kept sample, -1 if none. */
int msfm_epnp_ransac_batch(msfm_ctx* ctx, int n_problems, const int* offsets, const double* pts_w,
                           const double* pts_2d, const double* f, int max_iter, uint64_t seed, double* R,
                           double* t, double* errors, double* avg_error, int* best_iter);
/* AbsolutePoseEstimation::AbsolutePoseWithoutFocalLength (absolute_pose_estimation.cc:28-40, the arm of
 * IncrementalSfM::LocalizeImage an image without a known focal length takes, sfm_incremental.cc:673-704) for a batch of
 * images.  Per image AbsolutePoseEPNPF::EPNPF (absolute_pose_via_epnpf.cc:34-63): n_steps = (int)((f_ratio_max -
 * f_ratio_min) / f_ratio_step) candidate focal lengths f_i = (f_ratio_min + i * f_ratio_step) * f_init (:44, :49), one
 * complete EPNPRansac of `max_iter` samples at each, the first step whose kept sample has the smallest error below
 * 1000000.0 wins (:46, :56) - then AbsolutePoseEstimation::Error over all correspondences at the winning focal length (:35).
 * Step i of image p IS problem p * n_steps + i of msfm_epnp_ransac_batch with focal length f_i and the same seed and
 * max_iter, bit for bit (the reference likewise continues one std::rand stream through the sweep, so its steps draw
 * different samples); the whole sweep runs on the device, the correspondences are uploaded once and only one record per
 * step exists there.  The reference's quirk is kept: the minimal solver's "no fit" value 100000.0 is below the 1000000.0
 * start, so a sweep whose every step failed keeps step 0; only an image with fewer than 4 points keeps none. */
typedef struct msfm_epnpf_options {
  double f_ratio_min;  /* 0.5   absolute_pose_estimation.cc:31 */
  double f_ratio_max;  /* 4.00  absolute_pose_estimation.cc:32 */
  double f_ratio_step; /* 0.01  absolute_pose_via_epnpf.cc:41 */
  int32_t max_iter;    /* 200   absolute_pose_via_epnpf.cc:39; 1..65536 */
  uint64_t seed;
} msfm_epnpf_options;
void msfm_epnpf_default_options(msfm_epnpf_options* opt);
/* (int)((f_ratio_max - f_ratio_min) / f_ratio_step) in binary64 (350 for the defaults); MSFM_E_INVAL (< 0) unless
 * f_ratio_step > 0, f_ratio_max > f_ratio_min and the count is in 1..65535. */
int msfm_epnpf_num_steps(const msfm_epnpf_options* opt);
/* In : as msfm_epnp_ransac_batch, with f_init[n] = the guess the candidates scale (the reference: 1.2 * max(w, h),
 *      sfm_incremental.cc:675); n_problems <= 65535 and n_problems * n_steps must fit an int.
 * Out: f_out [n] = the kept candidate (the reference's SetFocalLength argument, sfm_incremental.cc:704); R, t, errors,
 *      avg_error = what msfm_epnp_ransac_batch returns for problem p * n_steps + best_step; best_step [n] and
 *      best_iter [n] (each may be NULL) = the kept step and its kept sample; step_error [n][n_steps] (may be NULL) = each
 *      step's error over its kept sample's own four points (absolute_pose_via_epnp.cc:129-133; 1e9 when no sample ran).
 *      No step kept (fewer than 4 points): f_out = f_init, best_step = best_iter = -1, the rest as
 *      msfm_epnp_ransac_batch returns it for such an image. */
int msfm_epnpf_sweep_batch(msfm_ctx* ctx, int n_problems, const int* offsets, const double* pts_w,
                           const double* pts_2d, const double* f_init, const msfm_epnpf_options* opt, double* f_out,
                           double* R, double* t, double* errors, double* avg_error, int* best_step, int* best_iter,
                           double* step_error);

/* ---- the localisation tries of one round, on the resident correspondence set (msfm_localize_candidates above) ---- */
/* The try loop of IncrementalSfM::Run (SfM/src/sfm_incremental.cc:143-164) around IncrementalSfM::LocalizeImage (:565-753)
 * for the ranked rows of a msfm_localize_set in one call, on the correspondences the set keeps on the device.  A failed
 * try returns at :670 / :701 before any state but localize_fail_times_ is touched, so the rows are independent and the
 * batch gives the answer of the one-at-a-time loop.
 *   - row r is eligible when its correspondence count is >= th_min_2d3d_corres (:148) and >= 3 (:567); tried rows are the
 *     first max_tries eligible rows with index >= first_row (max_tries = 0: all of them); next_row = the first eligible row
 *     behind the last tried one, or -1 - a host that found no winner calls again with first_row = next_row;
 *   - row_f[r] != 0 (:644-672): row r IS problem r of msfm_epnp_ransac_batch(n_kept, corr_off, pts_w, pts_2d, row_f,
 *     max_iter, seed), bit for bit; row_f[r] == 0 (:673-704): row r IS problem r of msfm_epnpf_sweep_batch(n_kept, corr_off,
 *     pts_w, pts_2d, row_f_init, &sweep), f[r] = the kept focal length (:703).  The samples of a row depend on (seed, r,
 *     sample) only, so first_row / max_tries change no row's result.  An arm without a tried row is not launched;
 *   - pass[r] = !(avg_error[r] > th_mse_localization), the negation of :648 / :679 (a NaN passes, as there); winner = the
 *     first tried row that passes, or -1;
 *   - corr_state, for passing rows, walks the row's correspondences in order as :709-729 does: 1 = errors[i] > avg_error
 *     (the point becomes is_bad_estimated_, :713-717); 2 = an inlier whose point is not pt_new_added and which is the first
 *     such inlier of the row naming that point (AddObservation / Camera::AddPoints take it, :721-728); 3 = an inlier whose
 *     point has is_new_added_ already, from pt_new_added or from an earlier correspondence of this row.  n_inliers counts
 *     state 2 (count_inliers, :727), n_outliers state 1.  A point may be taken through one feature and marked bad through
 *     another: both are reported.
 * In : row_f [n_kept] (>= 0; 0.0 = unknown), row_f_init [n_kept] (read where row_f == 0; may be NULL when no row needs it),
 *      n_points (> every point id of the set), pt_new_added [n_points] or NULL = all 0.
 * Out: a msfm_localize_pose_set (host memory only).  Per row: tried, arm (0 untried, 1 known focal length, 2 sweep),
 *      pass, f (row_f on arm 1), R [3][3], t [3], avg_error, best_step (-1 on arm 1), best_iter, n_inliers, n_outliers; per
 *      correspondence, in the layout of corr_off: errors, corr_state.  Untried rows hold zeros.  Every fetch pointer may be NULL.
 * No correspondence crosses PCIe on the way in and the host waits once.  Scratch: tried rows x n_points integers.
 * MSFM_E_INVAL: a set made without point_xyz, n_points not above a point id of the set, max_iter or the sweep options outside
 * what the two pose calls take, first_row < 0, max_tries < 0, a negative or NaN row_f. */
typedef struct msfm_localize_pose_options {
  double th_mse_localization; /* 5.0  basic_structs.h:186 */
  int32_t th_min_2d3d_corres; /* 20   basic_structs.h:177 */
  int32_t max_iter;           /* 200  EPnP samples, known-focal arm; 1..65536 */
  uint64_t seed;              /* 0x4D53464D50, the hosts' default for msfm_epnp_ransac_batch */
  msfm_epnpf_options sweep;   /* msfm_epnpf_default_options */
  int32_t first_row;          /* 0 */
  int32_t max_tries;          /* 16; 0 = every eligible row */
} msfm_localize_pose_options;
typedef struct msfm_localize_pose_set msfm_localize_pose_set;
void msfm_localize_pose_default_options(msfm_localize_pose_options* opt);
int msfm_localize_poses(msfm_ctx* ctx, const msfm_localize_set* set, const double* row_f, const double* row_f_init,
                        int n_points, const uint8_t* pt_new_added, const msfm_localize_pose_options* opt,
                        msfm_localize_pose_set** out);
int msfm_localize_pose_set_size(const msfm_localize_pose_set* set, int* n_rows, int* n_corr, int* n_tried, int* winner,
                                int* next_row);
int msfm_localize_pose_set_fetch(const msfm_localize_pose_set* set, uint8_t* tried, uint8_t* arm, uint8_t* pass, double* f,
                                 double* R, double* t, double* avg_error, int* best_step, int* best_iter, int* n_inliers,
                                 int* n_outliers, double* errors /*[n_corr]*/, uint8_t* corr_state /*[n_corr]*/);
void msfm_localize_pose_set_destroy(msfm_localize_pose_set* set);
/* RelativePoseEstimation::RelativePoseWithFocalLength (SfM/src/orientation/relative_pose_estimation.cc:91-120,
 * called for the seed pair, sfm_incremental.cc:309) for a batch of image pairs.  Per pair, on points divided by the
 * focal lengths: EssentialMatrixFivePoints::FivePointEssentialMatrixRANSAC (essential_matrix_five_point.cc:30-92) -
 * `ransac_times` (reference: 100) samples of 5 matches (all matches at once when there are 5..9), Nister's solver
 * through the 10x10 action matrix (:97-178; Eigen's FullPivLU / EigenSolver restated), every real solution scored
 * by the Sampson sum over all matches (:333-349), fewer than 4 solutions in total = failure - then
 * RelativePoseFromEssentialMatrix::ReltivePoseFromEMatrix (relative_pose_from_essential_matrix.cc:33-104): SVD of
 * E, four (R, t) hypotheses, each match votes for the first hypothesis that puts it in front of both cameras.
 * Out: E [n][9] row-major with x_cur^T E x_ref = 0 on (pixel / f, 1); R [n][9], t [n][3] exactly as the reference
 *      returns them in RTPoseRelative; ok [n]; n_candidates [n] (may be NULL) = number of essential matrices scored. */
int msfm_relpose_5pt_batch(msfm_ctx* ctx, int n_pairs, const int* offsets, const double* pts_ref,
                           const double* pts_cur, const double* f_ref, const double* f_cur, int ransac_times,
                           uint64_t seed, double* E, double* R, double* t, uint8_t* ok, int* n_candidates);
/* RelativePoseEstimation::RelativePoseWithoutFocalLength (relative_pose_estimation.cc:29-83, the arm of
 * IncrementalSfM::FindSeedPairThenReconstruct a seed pair takes when a focal length is missing,
 * sfm_incremental.cc:306-333) for a batch of image pairs.  Per pair, on centred pixels NOT divided by a focal length:
 * FundamentalMatrixEightPoint::NormalizedEightPointFundamentalMatrixRANSAC (fundamental_matrix_eight_point.cc:30-97) -
 * `ransac_times` (reference: 200) samples of 8 matches (all matches at once when there are 8..15), each through the
 * normalised eight-point fit (:105-168: centroid / RMS-to-sqrt(2) normalisation :175-203, the kernel of the constraint
 * matrix by full-pivot LU for 8 rows - a kernel of another dimension drops the sample - or its last right singular
 * vector for more, rank 2 enforced, T2^T F T1), every fit scored by the Sampson sum over all matches (:205-221), the
 * first smallest sum below 1000000.0 kept and the FIRST fit when none is (:82-96) - then
 * RelativePoseFromFundamentalMatrix::ReltivePoseFromFMatrix (relative_pose_from_fundamental_matrix.cc:25-51): Hartley's
 * focal lengths from F (:56-123; the rotation of each epipole onto the x-z plane is formed as c = e0 / |(e0, e1)|,
 * s = -e1 / |(e0, e1)| - the cosine and sine of the reference's atan2(-e1, e0) without a libm call), E = diag(f2, f2, 1)
 * F diag(f1, f1, 1) (:125-136), and the decomposition and cheirality vote of msfm_relpose_5pt_batch on pixel / f, whose
 * verdict the reference ignores.  Sample `it` of pair `p` is a pure function of (seed, p, it, number of matches).
 * Out: F [n][9] row-major with x_cur^T F x_ref = 0 on centred pixels; f_ref, f_cur [n]; E [n][9] row-major with
 *      x_cur^T E x_ref = 0 on (pixel / f, 1); R [n][9], t [n][3] as the reference returns them in RTPoseRelative; ok [n];
 *      best_iter [n] = the kept sample (0 in the all-matches case), best_error [n] = its Sampson sum (1000000.0 when the
 *      first fit was kept by default), n_candidates [n] = fits scored; each of the three may be NULL.
 *      Fewer than 8 matches or no fit: ok = 0, every output zero, best_iter = -1, best_error = 1000000.0.
 *      Focal lengths not extractable (an epipole with x == 0, or an f^2 < 0; a NaN passes, as in the reference): ok = 0,
 *      F, best_iter, best_error and n_candidates stand, the rest is zero. */
int msfm_relpose_8pt_batch(msfm_ctx* ctx, int n_pairs, const int* offsets, const double* pts_ref,
                           const double* pts_cur, int ransac_times, uint64_t seed, double* F, double* f_ref,
                           double* f_cur, double* E, double* R, double* t, uint8_t* ok, int* best_iter,
                           double* best_error, int* n_candidates);

/* ======================================================================================
 *  Which seed pair reconstructs, and with which points: the hypotheses of a model's first pair in one call
 * ====================================================================================== */
/* The loop body of IncrementalSfM::FindSeedPairThenReconstruct (SfM/src/sfm_incremental.cc:235-390) up to and including its
 * two gates, for a list of hypotheses at once, on the resident match store.  (The order of the list, SortImagePairs
 * :1790-1829, uses the C library's log and stays on the host: metricsfm_amd/seed.py::sort_image_pairs,
 * IncrementalSfM::SortImagePairs of host/objectsfm.cc.)  Per hypothesis h = (id_img1, id_img2) of hyp_img, in that order:
 *   matches  QueryMatch(id_img1, id_img2) = store row id_img1, entry id_img2, in stored order (:249); a pair the store does
 *            not hold has 0 matches; a feature that occurs in several matches stays in all of them; keypoints go float ->
 *            double (:298-303)
 *   arm      both f != 0: RelativePoseWithFocalLength with the given f (:307-315); otherwise RelativePoseWithoutFocalLength on
 *            centred pixels, and BOTH focal lengths are replaced (:316-333): with same_model[h] both become (f1 + f2) / 2
 *            (:324-327), else f1 and f2 (:330-331).  The pose was formed with the unaveraged values; that quirk is kept.
 *   pose     hypothesis h IS problem h of an n_hyp-problem call of msfm_relpose_5pt_batch (ransac_times_5pt, seed_5pt) or
 *            msfm_relpose_8pt_batch (ransac_times_8pt, seed_8pt) in which the problems of the other arm are empty, bit for
 *            bit: the sample key (seed, p, it[, n]) is the hypothesis index, and splitting a list over calls is the
 *            caller's business.  !ok (:313, :321): pose_ok = 0, no points, pass = 0; f = the given values, R = t = c = 0.
 *   cameras  camera 0 is [I|0] with centre 0 (:290); camera 1 has R = R21, t = t21 as returned and c = -(R^T t), each
 *            component summed left to right as Camera::SetRTPose of host/objectsfm.cc does (:334)
 *   points   every match is one two-view Point3D::Trianglate2(th_mse_reprojection, th_angle_small) with camera 0's
 *            observation first (:344-374); the points are the accepted ones in match order: pt_match (index into the
 *            pair's matches), X, mse.  Operation order of msfm_triangulate_midpoint_batch, but compiled without fused
 *            multiply-adds and with + - * / sqrt only, so a CPU restatement built with -ffp-contract=off agrees bit for bit;
 *            msfm_triangulate_midpoint_batch itself is contracted and agrees with this (and with its oracle) to 1e-9.
 *   gates    pass = pose_ok && n_points >= th_seedpair_structures && n_points >= n_matches / 5, integer division (:380-381)
 *   winner   the first h with pass, or -1; every hypothesis is answered (the reference stops at the winner).
 * keypoints (optional): float [sum of n_features][2] in image order, as in msfm_localize_problem; only the rows of the
 * hypotheses' images are uploaded.  Without it the store must hold the keypoints of those images (made from a chain).
 * Nothing that scales with the store's matches crosses PCIe: h2d_bytes of msfm_seed_set_size reports what was sent.
 * MSFM_E_INVAL: n_hyp outside [0, 65535], an image id outside the store, id_img1 == id_img2, no keypoints for an image,
 * a negative or NaN f, th_mse_reprojection or th_angle_small NaN, th_seedpair_structures < 0, ransac_times outside
 * [1, 65536].  The context stays usable.
 * msfm_seed_set_fetch (every pointer may be NULL): arm [n] (5 or 8), pose_ok [n], pass [n], n_matches [n], f [n][2],
 * R [n][9] row-major, t [n][3], c [n][3] of camera 1, pt_off [n+1], pt_match / X [..][3] / mse over pt_off[n] points.
 * The set also keeps the winner's pt_match / X / mse on the device, with its place in the store, for
 * msfm_recon_create_from_seed - of the winner only, in blocks sized by the longest hypothesis of the call.  It is a child of
 * its context, like a store: destroy it before the context; msfm_seed_set_destroy waits for the context's stream. */
typedef struct msfm_seed_options {      /* msfm_seed_default_options fills the reference's values */
  double th_mse_reprojection;           /* 3.0                  basic_structs.h:187 */
  double th_angle_small;                /* 3.0 / 180.0 * 3.1415 basic_structs.h:190, radians */
  int32_t th_seedpair_structures;       /* 20                   basic_structs.h:174 */
  int32_t ransac_times_5pt, ransac_times_8pt;   /* 100, 200 */
  uint64_t seed_5pt, seed_8pt;          /* 0x4D53464D45, 0x4D53464D38: the defaults of the two relpose calls' Python binding */
} msfm_seed_options;
void msfm_seed_default_options(msfm_seed_options* opt);
typedef struct msfm_seed_problem {
  int32_t n_hyp;                        /* <= 65535 */
  const int32_t* hyp_img;               /* [n_hyp][2] (id_img1, id_img2), tried in this order */
  const double* cam_fk;                 /* [n_hyp][2][3]: f (0.0 = unknown), k1, k2 of each camera's model */
  const uint8_t* same_model;            /* [n_hyp] both cameras share one CameraModel (:324) */
  const float* keypoints;               /* optional */
} msfm_seed_problem;
typedef struct msfm_seed_set msfm_seed_set;
int msfm_seed_hypotheses(msfm_ctx* ctx, const msfm_match_store* store, const msfm_seed_problem* problem,
                         const msfm_seed_options* opt, msfm_seed_set** out);
int msfm_seed_set_size(const msfm_seed_set* set, int* n_hyp, int* n_points, int* winner, int64_t* h2d_bytes);
int msfm_seed_set_fetch(const msfm_seed_set* set, uint8_t* arm, uint8_t* pose_ok, uint8_t* pass, int* n_matches, double* f /*[n][2]*/,
                        double* R /*[n][9]*/, double* t, double* c, int* pt_off /*[n+1]*/, int* pt_match, double* X, double* mse);
void msfm_seed_set_destroy(msfm_seed_set* set);

/* ======================================================================================
 *  The new 3D points of a localised image: every match with a visible camera in one call
 * ====================================================================================== */
/* IncrementalSfM::GenerateNew3DPoints (SfM/src/sfm_incremental.cc:755-915) on the resident match store, for a list of new
 * cameras at once.  The reference's case is n_new = 1 (the camera just localised); each new camera c1 (image i1) is answered
 * independently against the handed state - its rows do not depend on which other new cameras are in the call - and the host
 * decides how to apply several.  Per new camera:
 *   walk       its visible cameras in listed order, duplicates included (:766-894); c2 == c1 is skipped (:769); the matches
 *              are QueryMatch(i1, i2) = store row i1, entry i2, in stored order (:777); a pair the store does not hold has 0
 *              matches.  A skipped or empty entry keeps its place in the per-entry outputs.
 *   angle      th_angle_large when the pair's match count (all matches, before any filter) is > th_matches_large, else
 *              th_angle_small (:780-784); the cosine of both is formed once on the host with the C library
 *   candidate  match (f1, f2) is one when feat_point[c1][f1] < 0 and feat_point[c2][f2] < 0 (:804-808): only `>= 0` is read of
 *              feat_point, which stands for cams_[c]->pts_.find(..) != end() and does not depend on is_bad_estimated_.  The
 *              state does not change during the walk: a feature that occurs in several matches, within a pair or across
 *              visible cameras, yields a candidate in each.  Kept as the reference has it.
 *   point      a two-view Point3D::Trianglate2(th_mse_reprojection, th_angle) with c1's observation first, keypoints float ->
 *              double (:810-821): the arithmetic of msfm_seed_hypotheses' points - no fused multiply-adds, + - * / sqrt only,
 *              so a CPU restatement built with -ffp-contract=off agrees bit for bit and msfm_triangulate_midpoint_batch to
 *              1e-9.  A failed LLT, sqrt(mse) > th_mse_reprojection or an insufficient angle: not accepted.  The 100000.0 of
 *              a point behind a camera (structure.cc:280-284) is an mse like any other.  Poses and models must be finite:
 *              an accepted point whose mse is NaN has no key in the reference ((int)NaN is undefined); here it sorts first.
 *   order      ascending by mse TRUNCATED to int - the reference stores it through std::pair<Point3DNew*, int> (:829, :897).
 *              std::sort leaves ties open; here ties keep the order of the walk (a stable sort).
 *   claims     in that order every point is appended to pts_ (its id is n_points + its position), and Camera::AddPoints is
 *              std::map::insert (:908-909): the first point that names (c1, f1) takes that slot of camera c1, later ones do
 *              not; the same for (c2, f2).  takes1 / takes2 say which inserts took: what a host that rebuilds feat_point needs.
 * In : n_cams, cam_img, feat_point, n_points as in msfm_localize_problem (feat_point: camera c starts at the sum of
 *      n_features[cam_img[c']] over c' < c; n_points = pts_.size(), the id base); cam_R [n_cams][9], cam_t, cam_c, cam_fk
 *      [n_cams][3] as in msfm_tracks; new_cam [n_new] camera indices; vis_off [n_new+1], vis_cam: each new camera's
 *      visible_cams_ as listed.  keypoints (optional): float [sum of n_features][2] in image order; without it the store
 *      must hold the keypoints of the involved images (made from a chain).
 * Per call the host sends the feat_point and pose rows of the involved cameras (the new ones and their visible ones), for a
 * host-made store those images' keypoint rows, and a few integers per visible entry: nothing that scales with the store's
 * matches.  h2d_bytes of msfm_new_points_set_size reports it.  One stream synchronisation, at the end; the set is host memory.
 * MSFM_E_INVAL: n_new outside [0, 65535], a camera index outside n_cams, a cam_img outside the store or listed twice, no
 * keypoints for an involved image, a NaN threshold, th_mse_reprojection negative or >= 46340 (the key is an int of a value
 * up to its square), th_matches_large < 0, vis_off not ascending from 0.  The context stays usable.
 * msfm_new_points_set_fetch (every pointer may be NULL): pt_off [n_new+1]; per point e of new camera k (pt_off[k] <= e <
 * pt_off[k+1], id n_points + e - pt_off[k]) in sorted order: cam2 (camera index), feat1, feat2 (local features), vis_entry
 * (index into that camera's visible list), pt_match (index into the pair's matches), X [..][3], mse, takes1, takes2; per
 * visible entry (vis_off's indexing): n_matches, large (1: th_angle_large applied), n_candidates, n_accepted. */
typedef struct msfm_new_points_options {   /* msfm_new_points_default_options fills the reference's values */
  double th_mse_reprojection;              /* 3.0                  basic_structs.h:187 */
  double th_angle_small;                   /* 3.0 / 180.0 * 3.1415 basic_structs.h:190, radians */
  double th_angle_large;                   /* 5.0 / 180.0 * 3.1415 basic_structs.h:191 */
  int32_t th_matches_large;                /* 500                  sfm_incremental.cc:781 */
} msfm_new_points_options;
void msfm_new_points_default_options(msfm_new_points_options* opt);
typedef struct msfm_new_points_problem {
  int32_t n_cams;
  const int32_t* cam_img;
  const int32_t* feat_point;
  int32_t n_points;
  const double* cam_R;
  const double* cam_t;
  const double* cam_c;
  const double* cam_fk;
  int32_t n_new;                           /* <= 65535 */
  const int32_t* new_cam;
  const int32_t* vis_off;
  const int32_t* vis_cam;
  const float* keypoints;                  /* optional */
} msfm_new_points_problem;
typedef struct msfm_new_points_set msfm_new_points_set;
int msfm_new_points(msfm_ctx* ctx, const msfm_match_store* store, const msfm_new_points_problem* problem,
                    const msfm_new_points_options* opt, msfm_new_points_set** out);
int msfm_new_points_set_size(const msfm_new_points_set* set, int* n_new, int* n_points, int* n_entries, int64_t* h2d_bytes);
int msfm_new_points_set_fetch(const msfm_new_points_set* set, int* pt_off /*[n_new+1]*/, int* cam2, int* feat1, int* feat2, int* vis_entry,
                              int* pt_match, double* X, double* mse, uint8_t* takes1, uint8_t* takes2, int* n_matches /*[n_entries]*/,
                              uint8_t* large, int* n_candidates, int* n_accepted);
void msfm_new_points_set_destroy(msfm_new_points_set* set);

/* ======================================================================================
 *  Adjusting a round: partial / full bundle adjustment and the outlier removal in one call
 * ====================================================================================== */
/* The second half of a round of IncrementalSfM::Run (SfM/src/sfm_incremental.cc:172-186) on the flat state, behind
 * msfm_localize_candidates / msfm_localize_poses / msfm_new_points: PartialBundleAdjustment(new_cam) (:917-1014), every fifth
 * image FullBundleAdjustment (:1016-1026), RemovePointOutliers (:1831-1863).  The three switches do_partial / do_full /
 * do_outliers pick the stages; they always run in that order (:174-186), each on what the one before left.  No GPS rows (the
 * SLAM path has its own driver) and no Normalize / Perturb: found_seed_ is true before any round's adjustment (:141), so
 * RunOptimizetion's is_initial_run is false.
 * The state has both sides of the object graph.  feat_point is Camera::pts_ (as in msfm_new_points_problem); the rows
 * obs_point / obs_cam / obs_feat [n_obs] are Point3D::cams_ / pts2d_, one row per Point3D::AddObservation (camera index, local
 * feature), in any order.  The two differ wherever a Camera::AddPoints insert did not take (msfm_new_points' takes1 / takes2).
 *   point side the observations of a point are ordered by the key of cams_ (structure.cc:134), feature + image * idx_max_per_image:
 *              (image id, local feature) ascending - neither camera index order nor row order.  std::map::insert keeps the
 *              first of several rows with one key; they carry the same keypoint, so which one cannot show.  pt_views[p] is
 *              the number of distinct keys.  An observation's xy is the keypoint of (image, feature), float -> double
 *              (:592-600, :810-821).
 *   frozen     ImmutableCamsPoints (:1865-1878): every camera, and every point that occurs in some feat_point row, bad ones
 *              included.  A point no camera holds keeps its incoming pt_mutable (Point3D::is_mutable_, 1 for a new point,
 *              structure.cc:34): that is why the flag is state.
 *   partial    (:919-945) frees every camera of new_cam's model and every camera of `visible` (new_cam's visible_cams_ as
 *              listed, itself first), and for each freed camera the points of its own feat_point row that are not bad.
 *   full       MutableCamsPoints (:1880-1893): every camera is free, every point held by some camera is free, bad ones
 *              included; other points keep their flag.
 *   gather     optimizer.cc:59-129: bad points are skipped, the others go in ascending id, rows in key order; weight 1.0 at
 *              two views, weight_partial / weight_full at three or more, 1.0 otherwise.  What is handed to the solver is the
 *              compact problem: only rows whose camera or point is free (the others get no residual block, :86-125), only
 *              points with such a row, renumbered in ascending id; the masks pass through.  A stage whose problem has no
 *              row is skipped: solved[stage] = 0, no error.
 *   solve      msfm_ba_create + msfm_ba_run on device arrays (the route of msfm_chain_ba_create): parameters, summary and
 *              iteration rows are those of msfm_ba_solve on the same arrays, bit for bit.  UpdateParameters: the points
 *              return to their state ids on the device; cam_R / cam_t / cam_c = -R^T t / cam_fk are formed per camera as
 *              Camera::UpdatePoseFromData (camera.cc:113-137) and UpdataModelFromData do, the angle-axis conversion on the
 *              host inside the library with the C library's sin / cos.  "adjust cams" / "adjust pts" (:947-963) are the free
 *              cameras and the free points of all pts_ at each solve.
 *   outliers   bad points are skipped, their pt_mse and pt_new_added left as they are.  For every other point
 *              Point3D::Reprojection (structure.cc:267-300) over its rows in key order: pt_c = M (X, 1); pt_c.z < 0 sets mse
 *              100000.0 and returns at that row (strict: a NaN walks on); otherwise (u - x)^2 + (v - y)^2 is accumulated in
 *              that order and divided by the row count (no row: 0 / 0).  sqrt(mse) > th_mse_outliers marks the point bad (a
 *              NaN does not); pt_new_added is cleared for every visited point.  + - * / sqrt only, no fused multiply-add: a
 *              sequential restatement in doubles agrees bit for bit.  counts = count_outliers, count_new_add,
 *              count_outliers_new_add (:1833-1862).
 * In : n_cams, cam_img, feat_point, n_points, keypoints as in msfm_new_points_problem (the store supplies n_features and,
 *      made from a chain, the keypoints; otherwise `keypoints`); the rows; cam_pose [n_cams][6], cam_model [n_models][3],
 *      cam_model_of_cam, model_mutable (optional) as in msfm_ba_problem; point_xyz [n_points][3], pt_bad, pt_mse, pt_mutable
 *      [n_points]; pt_new_added (optional, NULL = all 0); new_cam (-1: none), visible [n_visible].
 * Per call the host sends feat_point, the rows, the point arrays and flags and the cameras; h2d_bytes of
 * msfm_round_set_size reports it (what msfm_ba_create sends of its own - cameras, masks - is not counted).  The host waits
 * for the sizes of each stage's problem, where msfm_ba_create / msfm_ba_run wait themselves, for the cameras after a solve,
 * and at the end (with keep_problem also for the assembled arrays).
 * MSFM_E_INVAL: an index outside its array (feat_point and the rows are checked on the device before anything is indexed by
 * them), new_cam or a visible camera outside n_cams, a cam_img outside the store or listed twice, no keypoints for an image
 * that has an observation, do_partial without new_cam, a NaN or negative threshold or weight, and a key that does not fit
 * the sort: the bit width of n_cams - 1 plus the bit width of the largest feature count - 1 must not exceed 32.  The
 * context stays usable.  A set counts as a child of its context.
 * msfm_round_set_fetch (every pointer may be NULL): cam_pose, cam_model, cam_R [n_cams][9], cam_t, cam_c, cam_fk [n_cams][3];
 * point_xyz, pt_mutable (as the last solve set it), pt_bad, pt_mse, pt_new_added, pt_views [n_points]; counts [3]; adjust
 * [2][2] = cams, pts of the partial and of the full solve; solved [2]; summary [2] (the caller's `iterations` /
 * `iterations_capacity` are kept and filled).  msfm_round_set_fetch_problem (sets made with keep_problem): the assembled
 * problem of stage 0 (partial) or 1 (full) - n_points, n_obs, kept [n_points] (the state id of every problem point), obs_cam,
 * obs_pt [n_obs], obs_xy [n_obs][2], pt_weight [n_points], cam_mutable [n_cams], pt_mutable [n_points]. */
typedef struct msfm_round_options {        /* msfm_round_default_options fills the reference's values */
  msfm_ba_options partial;                 /* msfm_ba_options_default with 100 iterations  basic_structs.h:181-182 */
  msfm_ba_options full;
  double weight_partial;                   /* 2.0                  sfm_incremental.cc:1012 */
  double weight_full;                      /* 1.0                  sfm_incremental.cc:1024 */
  double th_mse_outliers;                  /* 1.0                  basic_structs.h:188 */
  int32_t keep_problem;                    /* 1: keep each solve's assembled arrays for msfm_round_set_fetch_problem */
} msfm_round_options;
void msfm_round_default_options(msfm_round_options* opt);
typedef struct msfm_round_problem {
  int32_t n_cams;
  const int32_t* cam_img;
  const int32_t* feat_point;
  int32_t n_points;
  const float* keypoints;                  /* optional */
  int32_t n_obs;
  const int32_t* obs_point;
  const int32_t* obs_cam;
  const int32_t* obs_feat;
  const double* cam_pose;
  int32_t n_models;
  const double* cam_model;
  const int32_t* cam_model_of_cam;
  const uint8_t* model_mutable;            /* optional */
  const double* point_xyz;
  const uint8_t* pt_bad;
  const double* pt_mse;
  const uint8_t* pt_mutable;
  const uint8_t* pt_new_added;             /* optional */
  int32_t new_cam;                         /* -1: none */
  int32_t n_visible;
  const int32_t* visible;
  int32_t do_partial, do_full, do_outliers;
} msfm_round_problem;
typedef struct msfm_round_set msfm_round_set;
int msfm_round_adjust(msfm_ctx* ctx, const msfm_match_store* store, const msfm_round_problem* problem,
                      const msfm_round_options* opt, msfm_round_set** out);
int msfm_round_set_size(const msfm_round_set* set, int* n_cams, int* n_models, int* n_points, int64_t* h2d_bytes);
int msfm_round_set_fetch(const msfm_round_set* set, double* cam_pose, double* cam_model, double* cam_R, double* cam_t, double* cam_c,
                         double* cam_fk, double* point_xyz, uint8_t* pt_mutable, uint8_t* pt_bad, double* pt_mse, uint8_t* pt_new_added,
                         int32_t* pt_views, int32_t* counts /*[3]*/, int32_t* adjust /*[2][2]*/, int32_t* solved /*[2]*/,
                         msfm_ba_summary* summary /*[2]*/);
int msfm_round_set_fetch_problem(const msfm_round_set* set, int stage, int* n_points, int* n_obs, int32_t* kept, int32_t* obs_cam,
                                 int32_t* obs_pt, double* obs_xy, double* pt_weight, uint8_t* cam_mutable, uint8_t* pt_mutable);
void msfm_round_set_destroy(msfm_round_set* set);

/* ======================================================================================
 *  The resident state: a model's flat state kept on the device across its rounds
 * ====================================================================================== */
/* msfm_round_adjust sends the whole flat state with every call and reads every point array back.  A msfm_recon keeps that
 * state on the device: it is uploaded once, when the object is made, and msfm_recon_adjust runs the round's adjustment on it
 * in place.  The object is a child of its context and is bound to one match store, which must outlive it.
 *   device  feat_point (room for every feature of the store: an image has at most one camera), obs_point / obs_cam /
 *           obs_feat, point_xyz, pt_bad, pt_mse, pt_views, pt_mutable, pt_new_added, and the keypoints of a store that was
 *           not made from a chain (all images' rows, in the store's order).  Capacity and length are kept apart:
 *           reserve_points / reserve_obs ask for room beyond the initial lengths.
 *   host    inside the object, O(cameras): cam_img, cam_pose, cam_model, cam_model_of_cam, model_mutable, cam_R, cam_t,
 *           cam_c, cam_fk. */
/* msfm_recon_create: the fields of msfm_recon_init are those of msfm_round_problem plus pt_views and the cameras as the
 * flat state keeps them (cam_R [n_cams][9], cam_t, cam_c, cam_fk [n_cams][3]).  It is the only call that sends anything that
 * scales with points, observations or features.  The host waits once, for the answer of the index check.  MSFM_E_INVAL is what
 * msfm_round_adjust refuses of a state: a feat_point entry >= n_points or a row with an index outside its array (checked on
 * the device; nothing is kept of a refused state), a cam_img outside the store or listed twice, a cam_model_of_cam outside
 * n_models, no keypoints for an image that has an observation, a key that does not fit the sort. */
typedef struct msfm_recon_init {
  int32_t n_cams;
  const int32_t* cam_img;
  const int32_t* feat_point;
  int32_t n_points;
  const float* keypoints;                  /* optional: [sum of the store's n_features][2] */
  int32_t n_obs;
  const int32_t* obs_point;
  const int32_t* obs_cam;
  const int32_t* obs_feat;
  const double* cam_pose;
  int32_t n_models;
  const double* cam_model;
  const int32_t* cam_model_of_cam;
  const uint8_t* model_mutable;            /* optional */
  const double* cam_R;
  const double* cam_t;
  const double* cam_c;
  const double* cam_fk;
  const double* point_xyz;
  const uint8_t* pt_bad;
  const double* pt_mse;
  const int32_t* pt_views;
  const uint8_t* pt_mutable;
  const uint8_t* pt_new_added;             /* optional */
  int32_t reserve_points, reserve_obs;     /* capacities to start with, where larger than n_points / n_obs */
} msfm_recon_init;
typedef struct msfm_recon msfm_recon;
int msfm_recon_create(msfm_ctx* ctx, const msfm_match_store* store, const msfm_recon_init* init, msfm_recon** out);
/* msfm_recon_size: the lengths, the capacities in elements, and the bytes sent to the device since (and including) creation.
 * msfm_recon_fetch downloads the state (every pointer may be NULL; the host waits once): cam_img [n_cams], feat_point [the
 * cameras' features, camera after camera], the rows [n_obs], the point arrays [n_points], the camera tables. */
int msfm_recon_size(const msfm_recon* recon, int* n_cams, int* n_models, int* n_points, int* n_obs, int64_t* cap_points,
                    int64_t* cap_obs, int64_t* h2d_bytes);
int msfm_recon_fetch(msfm_recon* recon, int32_t* cam_img, int32_t* feat_point, int32_t* obs_point, int32_t* obs_cam, int32_t* obs_feat,
                     double* point_xyz, uint8_t* pt_bad, double* pt_mse, int32_t* pt_views, uint8_t* pt_mutable, uint8_t* pt_new_added,
                     double* cam_pose, double* cam_model, int32_t* cam_model_of_cam, double* cam_R, double* cam_t, double* cam_c,
                     double* cam_fk);
/* msfm_recon_localize is FindImageToLocalize (msfm_localize_candidates) plus the try loop of Run :143-164 (msfm_localize_poses)
 * on the resident arrays; the library walks the ranked rows in chunks of opt->max_tries itself (first_row / next_row) until a
 * row passes or the rows run out.  cand_img [n_cand] strictly ascending with fail_times, cand_f (0.0: the sweep arm around
 * cand_f_init) per candidate.  Sent: the candidate lists, four integers per walked pair, per chunk the rows' tables.  The state
 * is not written.  The winner (image = -1: none) comes back in msfm_recon_winner, whose counts size msfm_recon_localize_fetch:
 * ranked [n_ranked] image ids, failed [n_failed] (the tried rows ahead of the winner; all tried rows without one), visible
 * [n_visible] (the winner's visible cameras).  The winner row's corr_feat / corr_point / corr_state stay on the device inside
 * the object as a pending localisation; the next localize call that succeeds or the destroy call drops them; a
 * refused call leaves the lists and the pending winner of the call before as they were.  MSFM_E_INVAL: what the two
 * flat calls refuse (a registered candidate, cand_img not ascending, option ranges). */
typedef struct msfm_recon_winner {
  int32_t image, row;                      /* -1: no row passed */
  int32_t n_corr, n_inliers, n_outliers;   /* of the winner's row */
  int32_t n_ranked, n_failed, n_visible, n_chunks;
  double f, R[9], t[3], avg_error;
} msfm_recon_winner;
int msfm_recon_localize(msfm_recon* recon, int n_cand, const int32_t* cand_img, const int32_t* fail_times, const double* cand_f,
                        const double* cand_f_init, const msfm_localize_pose_options* opt, msfm_recon_winner* out);
int msfm_recon_localize_fetch(const msfm_recon* recon, int32_t* ranked, int32_t* failed, int32_t* visible);
/* msfm_recon_commit_camera is LocalizeImage :705-748 for the pending winner, on the device: the new camera's feat_point row
 * is filled with -1 and gets the state-2 correspondences, state 1 marks its point bad, state 2 gives its point a view and
 * pt_new_added and appends one row, in correspondence order (an exclusive scan of state == 2).  The host supplies the
 * angle-axis block cam_pose6 and the model: an existing index, or n_models to append cam_model3 (model_mutable: its flag).
 * cam_R / cam_t are the localised values, cam_c = -(R^T t), cam_fk = (the localised f, the model's k1, k2).  Nothing that scales with the state is sent.
 * visible (optional) [1 + n_visible]: the camera itself, then the winner's visible cameras.  MSFM_E_INVAL, before any write:
 * no pending winner (none found, or committed already), a model beyond n_models, a new model without cam_model3. */
int msfm_recon_commit_camera(msfm_recon* recon, const double* cam_pose6, int model, const double* cam_model3, int model_mutable, int* new_cam,
                             int32_t* visible);
/* msfm_recon_new_points is msfm_new_points for one camera of the state and its visible list on the resident feat_point and
 * keypoints, followed by sfm_incremental.cc:899-910 on the device: every new point is appended (xyz, its mse, two views, not
 * bad, new, mutable), its two rows (id, new_cam, feat1), (id, cam2, feat2) go behind the existing rows, and feat_point gets the
 * inserts that took - what newpoints.apply_new_points does to the flat state.  Sent: the walk's tables and the cameras of the
 * visible list (O(visible)).  The host waits twice: for the accepted counts, which size the append (n_new; arrays that are too
 * short move into blocks of twice the need first, device to device), and at the end.  stats (optional, may be NULL): the whole
 * msfm_new_points_set of the call for msfm_new_points_set_fetch - that read-back is the flat call's; destroy it with
 * msfm_new_points_set_destroy.  MSFM_E_INVAL is what msfm_new_points refuses - new_cam or a visible camera outside n_cams, a
 * NaN or out-of-range threshold, no keypoints of an involved image - and is found before the first write. */
int msfm_recon_new_points(msfm_recon* recon, int new_cam, int n_visible, const int32_t* visible, const msfm_new_points_options* opt,
                          int* n_new, msfm_new_points_set** stats);
/* msfm_recon_adjust is msfm_round_adjust on the resident arrays: the same stages, rules, kernels and waits (see there).  It
 * sends the camera tables only - per camera a handful of integers and flags and, for the outlier stage, 15 doubles; nothing
 * that scales with points or rows.  point_xyz, pt_bad, pt_mse, pt_new_added and (after a solve) pt_mutable are written in
 * place; pt_views is not written; the cameras and models are updated in the object's host tables.  The result is a
 * msfm_round_set without point arrays: msfm_round_set_size reports n_points = 0 and this call's h2d_bytes,
 * msfm_round_set_fetch leaves the point pointers untouched and fills cameras, counts, adjust, solved and the summaries;
 * msfm_round_set_fetch_problem works as ever.  MSFM_E_INVAL - new_cam or a visible camera outside n_cams, do_partial without
 * new_cam, a NaN or negative threshold or weight - is found before the first write: the state is what it was and the context
 * stays usable.  What a solve itself reports (msfm_ba_create / msfm_ba_run) comes after the first stage may have written its
 * points, while the host tables keep the cameras of before the call: such an object is to be destroyed. */
int msfm_recon_adjust(msfm_recon* recon, int new_cam, int n_visible, const int32_t* visible, int do_partial, int do_full, int do_outliers,
                      const msfm_round_options* opt, msfm_round_set** out);
/* msfm_recon_create_from_seed is the rest of FindSeedPairThenReconstruct (sfm_incremental.cc:290-374) for the winner of a
 * msfm_seed_set, which keeps its winner's points on the device: the state of a model of two cameras, made where those points
 * are.  The set must come from this store and is only read (it may be destroyed behind the call).
 *   cameras  cam_img = (id_img1, id_img2); camera 0 is [I|0] with centre 0, camera 1 has the set's R, t, c;
 *            cam_fk[c] = (the set's f of camera c, k1, k2 of cam_model[cam_model_of_cam[c]]).  The caller gives the solver's
 *            blocks as msfm_recon_commit_camera's caller does: cam_pose [2][6] (angle-axis, t), n_models (1 or 2), cam_model
 *            [n_models][3], cam_model_of_cam [2], model_mutable (optional).
 *   points   p = 0 .. P-1 in the set's order: point_xyz = X, pt_mse = mse, pt_views 2, pt_bad 0, pt_mutable 1,
 *            pt_new_added 1 (structure.cc:30-37)
 *   rows     (p, 0, feat1) at 2p and (p, 1, feat2) at 2p + 1, feat1 / feat2 read from the store's matches through pt_match
 *   feat_point  Camera::AddPoints is a std::map::insert: a feature that occurs in two accepted matches belongs to the first
 *            point (the lower id; both points keep both rows).  The two rows start as -1, and every point inserts itself
 *            with an integer minimum, so the result does not depend on the scheduling.
 * The arguments are plain, as msfm_recon_commit_camera's are.  keypoints (optional) as in msfm_recon_init; without it the
 * store must hold the keypoints of both images; reserve_points / reserve_obs: capacities to start with, where larger than P /
 * 2P.  Nothing that
 * scales with P or the store's matches is sent: h2d_bytes counts the keypoints of a host-made store, the upload
 * msfm_recon_create makes too.  The host waits once.  MSFM_E_INVAL, with nothing kept and the context usable: a set without a
 * winner, a set made on another store, n_models outside {1, 2}, a cam_model_of_cam outside n_models, no keypoints of either
 * image. */
int msfm_recon_create_from_seed(msfm_ctx* ctx, const msfm_match_store* store, const msfm_seed_set* set, const double* cam_pose /*[2][6]*/,
                                int n_models /*1 or 2*/, const double* cam_model /*[n_models][3]*/, const int32_t* cam_model_of_cam /*[2]*/,
                                const uint8_t* model_mutable /*optional*/, const float* keypoints /*optional*/, int reserve_points,
                                int reserve_obs, msfm_recon** out);
/* msfm_recon_normalize is the point side of BundleAdjuster::Normalize and Perturb (optimizer.cc:155-232) on the resident
 * points of any msfm_recon.  The arithmetic is this, in binary64 with + - * / and fabs only and no fused multiply-add, so a
 * sequential loop agrees bit for bit:
 *   mid[k] = (0.0 + x_0k + x_1k + ...) / n         left to right over all n points, bad ones included
 *   mad    = (0.0 + d_0 + d_1 + ...) / n           left to right, d_i = (|x_i0 - mid0| + |x_i1 - mid1|) + |x_i2 - mid2|
 *   scale  = target_deviation / mad
 *   x_ik   = scale * (x_ik - mid[k])               then, with noise, x_ik = x_ik + noise_ik * point_sigma (multiply, then add)
 * noise [n_points][3] (NULL: none) is the only upload that scales with the state and is counted in h2d_bytes; the reference
 * draws it from std::rand, which no restatement reproduces, so it is an input.  The reference's values: target_deviation 100.0 (optimizer.cc:182), point_sigma 0.5 (:201).
 * The host waits once, for mid and scale, which it returns; the points are written behind that wait.  n_points == 0 is
 * MSFM_E_INVAL, a scale that is not finite (all points equal) MSFM_E_NUMERIC; the state is untouched in both cases.
 * The camera side - SetACPose(a, scale (c - mid)), then SetACPose(a + n_r, c) and SetRTPose(R, t + n_t) per camera
 * (optimizer.cc:190-231) - needs the C library's trigonometry and stays with the caller, who writes the result with
 * msfm_recon_set_cameras: cam_pose [n_cams][6], cam_R [n_cams][9], cam_t, cam_c [n_cams][3] replace the object's host
 * tables (a NULL pointer keeps that table). */
int msfm_recon_normalize(msfm_recon* recon, const double* noise, double target_deviation, double point_sigma, double mid[3], double* scale);
int msfm_recon_set_cameras(msfm_recon* recon, const double* cam_pose, const double* cam_R, const double* cam_t, const double* cam_c);
void msfm_recon_destroy(msfm_recon* recon);

/* ==================================================================================== *
 *  Single-process multi-GPU context
 * ==================================================================================== */

/* ---- one process, several GPUs (threading row: "multi-GPU context msfm_ctx_create_multi(n_gpus) owns the
 * communicator") ----
 * The reference's entry point is ONE process (SfM/test/test_sfm/test_sfm.cc:22-70 `main`; BundleAdjuster::RunOptimizetion,
 * optimizer.cc:59-133, is called from a single thread).  A multi context keeps that shape: it owns one msfm_ctx per device,
 * a host thread per device inside the library, and the communicator between them - RCCL's ncclCommInitAll over xGMI when
 * the devices are distinct, an in-process reduction (host barrier + a device-side sum in rank order) when the contexts share
 * one device (`devices` may name the same device more than once: how the path is tested on a one-GPU box).
 *   devices == NULL: devices 0 .. n_gpus-1.
 * The msfm_multi_* calls below are the single-context calls with the split inside: same arguments, same results
 * (bundle adjustment to 1e-9 of the one-context solve - the sums are formed in another order; everything else bit for bit). */
typedef struct msfm_multi msfm_multi;
int msfm_ctx_create_multi(int n_gpus, const int* devices, msfm_multi** out);
void msfm_multi_destroy(msfm_multi* mc);
int msfm_multi_size(const msfm_multi* mc);
msfm_ctx* msfm_multi_ctx(msfm_multi* mc, int rank);          /* the context of rank r (rank 0: where single-context work goes) */
const char* msfm_multi_last_error(const msfm_multi* mc);
/* ceres::Solve (optimizer.cc:133) with the points - and all their observations - split over the contexts in contiguous
 * ranges balanced by the work the mutability masks leave, cameras and intrinsics replicated, three reductions per linear
 * solve over the communicator.  Arguments and results as msfm_ba_solve. */
int msfm_multi_ba_solve(msfm_multi* mc, msfm_ba_problem* problem, const msfm_ba_options* options, msfm_ba_summary* summary);
/* Point3D::Trianglate2 / Trianglate / Reprojection (structure.cc:163-300) with the tracks split by observation count; no
 * collective (tracks are independent). */
int msfm_multi_triangulate_midpoint_batch(msfm_multi* mc, const msfm_tracks* tracks, double th_error, double th_angle, double* X,
                                          double* mse, uint8_t* ok);
int msfm_multi_triangulate_dlt_batch(msfm_multi* mc, const msfm_tracks* tracks, double th_error, double th_angle, double* X, double* mse,
                                     uint8_t* ok);
int msfm_multi_reproject_mse_batch(msfm_multi* mc, const msfm_tracks* tracks, const double* X, double* mse);
/* The matching loop of FineMatchingGraph::BuildMatchGraph (fine_matching_graph.cc:87-133) over a pair list, the idx1-major
 * list cut into contiguous slices balanced by M1 * M2, one per context; no collective (pairs are independent).
 *   desc[i]: [count[i]][dim] float descriptors of image i (host); pairs [n_pairs][2] = (idx1, idx2);
 *   code[p]: count[idx2 of pair p] match codes (MSFM_MATCH_*), n_all / n_good [n_pairs] (either may be NULL). */
int msfm_multi_match_pairs(msfm_multi* mc, int n_images, const float* const* desc, const int* count, int dim, const int* pairs, int n_pairs,
                           float ratio_good, float ratio_all, int32_t* const* code, int* n_all, int* n_good);

#ifdef __cplusplus
}
#endif
#endif /* MSFM_H_ */
