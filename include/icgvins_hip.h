/*
 * icgvins_hip.h — C ABI of the MI355X-native IC-GVINS hot path (libicgvins_hip.so).
 *
 * This is the drop-in boundary B3 of SURVEY.md §8(b): plain pointers and sizes, no C++/torch types, no exceptions.
 * Every entry point names the reference interface it replaces (paths relative to /root/reference/ic_gvins/ic_gvins/).
 *
 * Conventions
 *   - return value: 0 = ICG_OK, <0 = error code; icg_last_error(ctx) gives a message.
 *   - an icg_ctx owns one HIP stream + all device buffers for one (GPU, image size); it is NOT thread-safe;
 *     distinct contexts are independent.  Caller owns every host buffer passed in.
 *   - every call is batched: "jobs" index frame *slots* (device-resident CLAHE image + pyramid), so one call can
 *     serve many independent camera streams at once (the unit that fills an MI355X; SURVEY.md §0 "scale honesty").
 *   - calls are synchronous unless stated: results are in the host buffers when the call returns.
 *   - points are float pairs (x,y) == cv::Point2f; status bytes are 0/1 == the reference's vector<uint8_t>.
 *   - there is NO CPU fallback: without a HIP device icg_ctx_create fails with ICG_ERR_NODEVICE.
 */
#ifndef ICGVINS_HIP_H
#define ICGVINS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct icg_ctx icg_ctx;

enum {
    ICG_OK           = 0,
    ICG_ERR_INVALID  = -1, /* bad argument */
    ICG_ERR_HIP      = -2, /* HIP runtime error (see icg_last_error) */
    ICG_ERR_NOMEM    = -3,
    ICG_ERR_NODEVICE = -4, /* no usable gfx950 device: the product path refuses to run */
    ICG_ERR_CAPACITY = -5  /* batch larger than the capacity given at icg_ctx_create */
};

/* Camera intrinsics/distortion, tracking/camera.h:88-93 (fx,fy,cx,cy,skew ; k1,k2,p1,p2,k3). */
typedef struct icg_camera {
    double fx, fy, cx, cy, skew;
    double k1, k2, p1, p2, k3;
} icg_camera;

typedef struct icg_ctx_config {
    int device;     /* HIP device ordinal */
    int width;      /* image width  (camera_->width())  */
    int height;     /* image height (camera_->height()) */
    int n_slots;    /* frame slots kept resident (>= 2 per stream: frame_pre_ and frame_cur_, +1 per ref frame) */
    int max_batch;  /* max frames per icg_frames_preprocess / icg_detect call */
    int max_points; /* max points per point-batched call */
    int max_factors;/* max reprojection factors per icg_reproj_eval_batch call (0 = back-end unused) */
} icg_ctx_config;

/* ---- context ----------------------------------------------------------------------------------------- */
int icg_ctx_create(const icg_ctx_config *cfg, icg_ctx **out);
void icg_ctx_destroy(icg_ctx *ctx);
const char *icg_last_error(const icg_ctx *ctx);
int icg_ctx_sync(icg_ctx *ctx);
/* How a call waits for its kernels (no reference counterpart; the reference's OpenCV calls are synchronous CPU code):
 *   ICG_WAIT_SPIN   busy-wait on the stream: lowest latency, occupies a host core (default; one tracker per process)
 *   ICG_WAIT_POLL   query + sleep sleep_us between queries: the core is free for other contexts' threads (many contexts
 *                   per host core, see host/tracking_batch.h)
 * The environment variable ICG_WAIT_MODE=spin|poll[:us] overrides the setting of every context. */
#define ICG_WAIT_SPIN 0
#define ICG_WAIT_POLL 1
int icg_ctx_set_wait_mode(icg_ctx *ctx, int mode, int sleep_us);
/* hipStream_t of the context (for callers that want to record their own HIP events on it). */
void *icg_ctx_stream(icg_ctx *ctx);
int icg_set_camera(icg_ctx *ctx, const icg_camera *cam);
/* The context's camera TABLE: n_cams cameras resident on the device, one per camera stream the context serves — the reference constructs
 * a Tracking (and a GVINS) per camera (tracking/tracking.h:51, tracking/camera.h:88-93); a context holds ONE image size and N cameras.
 * Replaces the table the context held.  Read by the entries named *_cams (icg_lk_track_fb_cams, icg_reproj_error_batch_cams,
 * icg_tracker_create_cams); icg_set_camera's camera and every entry that uses it are unaffected.  The stand-alone point entries
 * (icg_undistort_points, icg_distort_points, icg_predict_mappoints, icg_predict_rotation) are not called by the host layer and stay on
 * icg_set_camera's camera.  ICG_ERR_INVALID: n_cams <= 0 or cams NULL (the table the context held stays). */
int icg_set_cameras(icg_ctx *ctx, int n_cams, const icg_camera *cams);
const char *icg_version(void);
/* number of pyramid levels built for the context's image size (== maxLevel+1 of calcOpticalFlowPyrLK). */
int icg_pyramid_levels(const icg_ctx *ctx);

/* Per-kernel timing with HIP events recorded on the context stream around every launch of `kernel_name`
 * (e.g. "lk_track_fb"); used by bench.py for the roofline figures.  enable=0 disables and clears. */
int icg_prof_enable(icg_ctx *ctx, int enable);
int icg_prof_get(icg_ctx *ctx, const char *kernel_name, int *launches, double *total_ms);
/* names of profiled kernels, '\n' separated, into buf */
int icg_prof_names(icg_ctx *ctx, char *buf, int buflen);

/* Device scratch for callers that keep inputs resident in HBM (bench harness): plain hipMalloc/hipFree/hipMemcpy. */
int icg_dev_alloc(icg_ctx *ctx, size_t bytes, void **dptr);
int icg_dev_free(icg_ctx *ctx, void *dptr);
int icg_dev_upload(icg_ctx *ctx, void *dptr, const void *host, size_t bytes);
int icg_dev_download(icg_ctx *ctx, void *host, const void *dptr, size_t bytes);

/* ---- F1: Tracking::preprocessing (tracking/tracking.cc:107-142) ----------------------------------------
 * For each job k: BGR->gray if channels==3 (tracking.cc:112), CLAHE(3.0, 21x21) (tracking.cc:63,139), then the
 * LK pyramid (the buildOpticalFlowPyramid every calcOpticalFlowPyrLK call redoes, tracking.cc:385-393) into slot
 * slots[k].  images[k] points to host memory (src_on_device=0) or device memory (src_on_device=1).
 * hist_mean (optional, n doubles) receives calculateHistigram() of the gray image (tracking.cc:88-105). */
int icg_frames_preprocess(icg_ctx *ctx, int n, const int32_t *slots, const uint8_t *const *images, int stride,
                          int channels, int src_on_device, double *hist_mean);
/* copy pyramid level `level` of a slot back to the host (Frame::image() == level 0, after CLAHE). */
int icg_frame_download(icg_ctx *ctx, int slot, int level, uint8_t *dst, int dst_stride);

/* ---- F2: cv::calcOpticalFlowPyrLK as called at tracking.cc:385-393 / 487-496 ---------------------------
 * win 21x21, maxLevel 3, (COUNT+EPS, 30, 0.01), OPTFLOW_USE_INITIAL_FLOW, minEigThreshold 1e-4.
 * next_pts: initial flow in, result out.  status/err as OpenCV (err may be NULL). */
int icg_lk_track(icg_ctx *ctx, int n, const int32_t *prev_slot, const int32_t *next_slot, const float *prev_pts,
                 float *next_pts, uint8_t *status, float *err);

/* ---- F2+F3(+F4): the fused forward/backward track of tracking.cc:380-403 and :482-506 --------------------
 * forward LK prev->next from guess_pts, backward LK next->prev from prev_pts, then
 * status = fwd && bwd && !isOnBorder(fwd) (tracking.cc:847-849) && ptsDistance(bwd, prev) < 0.5 (:841-845).
 * out_undist (optional) = Camera::undistortPoints(out_pts) (camera.cc:72-74), needs icg_set_camera.
 * keep_idx/n_keep (optional) = order-preserving compaction indices, i.e. what reduceVector (tracking.cc:831-839)
 * keeps, computed on device. */
int icg_lk_track_fb(icg_ctx *ctx, int n, const int32_t *prev_slot, const int32_t *next_slot, const float *prev_pts,
                    const float *guess_pts, float *out_pts, uint8_t *status, float *out_undist, int32_t *keep_idx,
                    int32_t *n_keep);

/* icg_lk_track_fb with one camera index per point: out_undist[i] = Camera::undistortPoints (camera.cc:72-74) of out_pts[i] under camera
 * cam_idx[i] of the context's table (icg_set_cameras) — the points of several Tracking instances, each with its own camera
 * (tracking/tracking.h:51), in one call.  out_pts, status, keep_idx and n_keep do not depend on the camera.
 * ICG_ERR_INVALID, nothing launched and no output touched: no table set, cam_idx NULL, an index outside the table, and icg_lk_track_fb's. */
int icg_lk_track_fb_cams(icg_ctx *ctx, int n, const int32_t *prev_slot, const int32_t *next_slot, const float *prev_pts,
                         const float *guess_pts, const int32_t *cam_idx, float *out_pts, uint8_t *status, float *out_undist,
                         int32_t *keep_idx, int32_t *n_keep);

/* ---- F4: Camera point maps (tracking/camera.cc) -------------------------------------------------------- */
int icg_undistort_points(icg_ctx *ctx, int n, float *pts);                 /* camera.cc:72-74  in place */
int icg_distort_points(icg_ctx *ctx, int n, float *pts);                   /* camera.cc:76-89  in place */
/* ---- F5: INS-aided predictions --------------------------------------------------------------------------
 * map points: world2pixel(pos, pose_cur) then distortPoints (tracking.cc:367-378).  pose = R(9 row-major), t(3);
 * pose_idx[k] selects the pose of point k (one pose per stream). */
int icg_predict_mappoints(icg_ctx *ctx, int n, const double *pw, const int32_t *pose_idx, int n_poses,
                          const double *poses12, float *pts_out);
/* reference features: distortCameraPoint(R_cur^T R_pre * pixel2cam(undistort(p))) (tracking.cc:465-479).
 * rot_idx[k] selects r_cur_pre (n_rots x 9 row-major, already R_cur^T*R_pre). */
int icg_predict_rotation(icg_ctx *ctx, int n, const float *pts_in, const int32_t *rot_idx, int n_rots,
                         const double *rots9, float *pts_out);

/* ---- F6: cv::findFundamentalMat(FM_RANSAC, thresh, conf, mask) as used at tracking.cc:547-555 -----------
 * Batched over independent point sets: set s owns points [offsets[s], offsets[s+1]).  Sets with fewer than 15
 * points are left untouched (mask = 1), as the reference skips them.  mask: 0/1 per point. */
int icg_fm_ransac(icg_ctx *ctx, int n_sets, const int32_t *offsets, const float *pts1, const float *pts2,
                  double thresh, double conf, uint8_t *mask);
/* the same call as icg_fm_ransac, kept under its earlier name.  Both make ONE launch: every set's whole RANSAC run — subset draws from the
 * set's cv::RNG, seven-point solves, scoring, the best / niters recurrence of RANSACPointSetRegistrator::run — inside the workgroup that owns
 * the set (csrc/ransac.hip k_fm_ransac_sets); the device-resident tracker runs the same kernel on its segments. */
int icg_fm_ransac_device(icg_ctx *ctx, int n_sets, const int32_t *offsets, const float *pts1, const float *pts2, double thresh,
                         double conf, uint8_t *mask);

/* ---- F7: Tracking::featuresDetection (tracking.cc:576-688) ----------------------------------------------
 * Gridded cv::goodFeaturesToTrack(quality 0.01, minDistance, mask) + cv::cornerSubPix((5,5),(-1,-1),(20,0.01))
 * per block ROI, for n jobs at once.  Job k detects on slot slots[k]; its mask discs (cv::circle radius
 * min_dist, tracking.cc:609-620) are centred on mask_pts[mask_off[k]..mask_off[k+1]); its per-block quotas
 * (track_max_block_features_ - features_cnts[b], tracking.cc:629) are quota[k*n_blocks + b] (<=0: skip block).
 * Output: out_pts holds up to max_per_job points per job in block order with block origin already added
 * (tracking.cc:669-685); out_count[k] = points found; out_block (optional) = block id per point. */
typedef struct icg_detect_grid {
    int block_cols, block_rows; /* block_cols_, block_rows_  tracking.cc:66-67 */
    int block_w, block_h;       /* block_indexs_[0]          tracking.cc:71-73 */
    int min_dist;               /* track_min_pixel_distance_ tracking.cc:85    */
    int max_per_block;          /* track_max_block_features_ tracking.cc:81    */
} icg_detect_grid;
int icg_detect(icg_ctx *ctx, int n, const int32_t *slots, const icg_detect_grid *grid, const int32_t *mask_off,
               const float *mask_pts, const int32_t *quota, int max_per_job, float *out_pts, int32_t *out_count,
               int32_t *out_block);

/* ---- F8: Tracking::triangulatePoint (tracking.cc:800-811), batched ---------------------------------------
 * T0/T1: per-point indices into Tcw (n_T x 12, row-major 3x4 == pose2Tcw(pose).topRows<3>()); pc0/pc1: pixel2cam. */
int icg_triangulate(icg_ctx *ctx, int n, const int32_t *T0_idx, const int32_t *T1_idx, int n_T, const double *Tcw12,
                    const double *pc0, const double *pc1, double *pw);

/* ---- R1: ReprojectionFactor::Evaluate (factors/reprojection_factor.h:55-147), batched ---------------------
 * obs_soa: 15 x n doubles, component-major: pts0[3], pts1[3], vel0[3], vel1[3], td0, td1, std (ctor :42-53).
 * poses: K x 7 [px,py,pz,qx,qy,qz,qw] (parameters[0], parameters[1]); ext: 7 (parameters[2]);
 * invdepth: L (parameters[3]); td (parameters[4]).
 * out_r: n x 2.  out_J (want_jac): n x 46 = J_pose_i[2x7], J_pose_j[2x7], J_ext[2x7] row-major (7th col 0),
 * J_invdepth[2], J_td[2] — exactly the blocks Ceres hands to Evaluate.
 * huber_delta > 0 additionally applies ResidualBlockInfo's robust correction (factors/residual_block_info.h:59-87),
 * i.e. R2 as used by marginalization; 0 = plain Evaluate. */
int icg_reproj_eval_batch(icg_ctx *ctx, int n, const double *obs_soa, const int32_t *idx_i, const int32_t *idx_j,
                          const int32_t *idx_lm, int n_poses, const double *poses, const double *ext, int n_lm,
                          const double *invdepth, double td, int want_jac, double huber_delta, double *out_r,
                          double *out_J);
/* Same with the static part (obs, indices) already resident: upload once per Ceres problem, evaluate many times. */
int icg_reproj_set_factors(icg_ctx *ctx, int n, const double *obs_soa, const int32_t *idx_i, const int32_t *idx_j,
                           const int32_t *idx_lm);
/* The same upload in two steps for callers that assemble a large factor set from many threads (the windows of many streams): the context
 * hands out PINNED host memory for n factors — *obs_soa: 15 x n doubles, component-major as above; *idx3: 3 x n int32, idx_i | idx_j |
 * idx_lm — the caller fills it in place, icg_reproj_commit_factors uploads it (equivalent to icg_reproj_set_factors on the same content).
 * The pointers are valid until the next stage / set call on ctx. */
int icg_reproj_stage_factors(icg_ctx *ctx, int n, double **obs_soa, int32_t **idx3);
int icg_reproj_commit_factors(icg_ctx *ctx);
int icg_reproj_eval_resident(icg_ctx *ctx, int n_poses, const double *poses, const double *ext, int n_lm,
                             const double *invdepth, double td, int want_jac, double huber_delta, double *out_r,
                             double *out_J);
/* the same evaluation with r (n x 2) and J (n x 46) left in the context's pinned staging memory: *r_view / *J_view are valid until the
 * next call on ctx.  ReprojectionBatch (the ceres::EvaluationCallback of boundary B1) hands each factor's Evaluate() its slice of the views. */
int icg_reproj_eval_resident_view(icg_ctx *ctx, int n_poses, const double *poses, const double *ext, int n_lm, const double *invdepth,
                                  double td, int want_jac, double huber_delta, const double **r_view, const double **J_view);

/* ---- M2: MarginalizationInfo::constructEquation (factors/marginalization_info.h:195-230) for the reprojection
 * factors of the last icg_reproj_eval_* call (Jacobians still resident): accumulates H0 += J^T J, b0 -= J^T e into
 * a dense (local_size x local_size) system on device and adds it to the host arrays H0/b0.
 * col_pose[k] (n_poses), col_ext, col_lm[l] (n_lm), col_td: local column index of each parameter block, -1 = constant. */
int icg_reproj_accumulate_normal(icg_ctx *ctx, int local_size, const int32_t *col_pose, int32_t col_ext,
                                 const int32_t *col_lm, int32_t col_td, double *H0, double *b0);

/* ---- f1 (SURVEY.md §8 "next" row): device-side landmark elimination for the Gauss-Newton / LM step of
 * GVINS::gvinsOptimization (ic_gvins.cc:1130-1239: Ceres LEVENBERG_MARQUARDT + DENSE_SCHUR).  Works on the robust-corrected r/J
 * left resident by the last icg_reproj_eval_resident(want_jac=1): assembles H = J^T J, b = -J^T r of the ACTIVE factors on the
 * device (camera columns 0..P-1 given by col_pose/col_ext/col_td, -1 = constant block; inverse depth l at column P+l), then
 * eliminates the 1x1 inverse-depth blocks:  S = Hcc - G^T diag(1/(h_ll+d_l)) G,  s = bc - G^T (b_l/(h_ll+d_l)),
 * d_l = clamp(h_ll, min_diag, max_diag) * damp (LM diagonal of the eliminated block; damp = 1/trust-region radius).
 * Outputs: S (P x P row-major), s (P), diag_cc (P, diagonal of Hcc before elimination: the host needs it for the LM diagonal
 * of the camera block; may be NULL), cost (0.5 sum rho(|r|^2) of the active factors at the linearization point; may be NULL).
 * reassemble = 0 re-uses the resident H, b with a new damp (after a rejected step; cost is not touched).
 * The full system stays on the device for icg_reproj_backsub:  delta_l = (b_l - G_l . delta_c) / (h_ll + d_l)  (n_lm values);
 * lm_terms (2 doubles, may be NULL) = sum b_l^2/(h_ll+d_l), sum d_l delta_l^2: the landmark part of the LM model decrease
 * 0.5 (delta^T b + delta^T D delta), where delta^T b = delta_c^T s + lm_terms[0].
 * icg_reproj_cost: the same cost for the CURRENT resident residuals (e.g. after a want_jac=0 evaluation at a trial point). */
int icg_reproj_schur(icg_ctx *ctx, int P, const int32_t *col_pose, int32_t col_ext, int32_t col_td, const uint8_t *active,
                     int reassemble, double damp, double min_diag, double max_diag, double *S, double *s, double *diag_cc,
                     double *cost);
int icg_reproj_backsub(icg_ctx *ctx, int P, const double *delta_c, double *delta_l, double *lm_terms);
int icg_reproj_cost(icg_ctx *ctx, const uint8_t *active, double *cost);
/* h_ll (n_lm values) of the system left resident by the last icg_reproj_schur: the diagonal of the inverse-depth block BEFORE damping.
 * M3 (factors/marginalization_info.h:170-192) uses it to decide whether the landmark block may be eliminated by plain reciprocals
 * (all h_ll well above the reference's 1e-8 eigenvalue floor) or has to go through the dense pseudo-inverse. */
int icg_reproj_landmark_diag(icg_ctx *ctx, double *h_ll);

/* f1, many windows per launch: the windows of many camera streams advance through their LM steps together, ONE evaluation / assembly /
 * reduction / back-substitution launch per step for all of them (a solver per stream is bounded by the runtime's launch rate).
 * icg_reproj_set_windows partitions the resident factor set: factors [fac_off[w], fac_off[w+1]) and landmarks [lm_off[w], lm_off[w+1])
 * belong to window w (factors sorted by window, landmarks contiguous per window, every pose used by one window only; poses and
 * landmarks keep their global indices).  The *_windows calls mirror icg_reproj_eval_resident / _schur / _backsub / _cost with one
 * extrinsic (ext: W x 7) and td per window, one reduced system of the common size P per window (S: W x P x P, s / diag_cc: W x P; a
 * window simply leaves the columns it does not use empty), per-window damping and per-window reassemble flags (0 = keep the window's
 * resident H, b and only apply the new damping).  cost (W) is written for the re-assembled windows only (0 elsewhere); lm_terms is
 * W x 2.  col_pose[k] is the column of pose k INSIDE its window's system. */
int icg_reproj_set_windows(icg_ctx *ctx, int n_windows, const int32_t *fac_off, const int32_t *lm_off);
int icg_reproj_eval_windows(icg_ctx *ctx, int n_poses, const double *poses, const double *ext, int n_lm, const double *invdepth,
                            const double *td, int want_jac, double huber_delta);
int icg_reproj_schur_windows(icg_ctx *ctx, int P, const int32_t *col_pose, const int32_t *col_ext, const int32_t *col_td, const uint8_t *active,
                             const uint8_t *reassemble, const double *damp, double min_diag, double max_diag, double *S, double *s,
                             double *diag_cc, double *cost);
/* the same call with the W x P x P reduced systems left where the reduction kernel writes them (the context's pinned staging memory):
 * *S_view is valid until the next call on ctx.  Saves the device-to-host copy and the copy-out of 9 MB per LM step at 256 C2 windows.
 * Only the lower triangle (rows >= columns) is written (the systems are symmetric; a Cholesky factorization reads nothing else): the
 * elements above the diagonal are undefined. */
int icg_reproj_schur_windows_view(icg_ctx *ctx, int P, const int32_t *col_pose, const int32_t *col_ext, const int32_t *col_td, const uint8_t *active,
                                  const uint8_t *reassemble, const double *damp, double min_diag, double max_diag, const double **S_view, double *s,
                                  double *diag_cc, double *cost);
/* the same call with the reduced systems left RESIDENT: the lower triangles stay in a device buffer of the context (nothing of S crosses
 * the link) for icg_reproj_solve_windows; s, diag_cc and cost come back as above.  The resident systems are valid until the next
 * icg_reproj_schur* call of any form (each rewrites the window systems the back-substitution reads) or icg_reproj_set_windows on ctx;
 * the host parts of icg_reproj_solve_windows outlive the other schur forms. */
int icg_reproj_schur_windows_resident(icg_ctx *ctx, int P, const int32_t *col_pose, const int32_t *col_ext, const int32_t *col_td,
                                      const uint8_t *active, const uint8_t *reassemble, const double *damp, double min_diag, double max_diag,
                                      double *s, double *diag_cc, double *cost);
/* The reduced camera solve and the landmark back-substitution of an LM step for all windows, on the systems
 * icg_reproj_schur_windows_resident left on the device.  For every window with solve[w] != 0:
 *   A = lower(S_w) + lower(host part of w) on the leading Pw[w] columns, then A_kk += dd[w * P + k] — each element (S + H) + dd, the operand
 *   order of the host loop; A x = rhs[w * P ..] by icg_chol_solve_batch's arithmetic (the host layer's choleskySolve, bit for bit);
 *   delta_c (W x P): x on the leading Pw[w] columns; zeros beyond Pw[w], for a window that is not solved and for one whose status is 1;
 *   status (W, optional): 0 ok or not solved, 1 not positive definite / non-finite.
 * Then icg_reproj_backsub_windows' kernels run on the delta_c that is already on the device: delta_l (n_lm) and lm_terms (W x 2), both
 * optional.  dd and rhs are W x P.
 * Host parts: the device keeps one per window (the packed lower triangle of the leading Pw x Pw block: row i holds columns 0 .. i) until it is
 * replaced.  host_S carries the parts of the windows with host_part_new[w] != 0 only, window after window; host_part_new = NULL or all zero
 * with host_S = NULL is valid.  A window that never received a part has none (A = S + dd).  Parts are dropped by
 * icg_reproj_set_windows and when icg_reproj_schur_windows_resident changes W or P.
 * ICG_ERR_INVALID: no resident systems of this P (icg_reproj_schur_windows_resident of the same P must be the LAST schur call), a NULL required pointer, Pw[w]
 * outside 1 .. P for a window that is solved or receives a part, a flagged part without host_S, a resident part whose column count is not
 * Pw[w] (the message names the window).  After an error nothing was launched. */
int icg_reproj_solve_windows(icg_ctx *ctx, int P, const int32_t *Pw, const uint8_t *solve, const uint8_t *host_part_new, const double *host_S,
                             const double *dd, const double *rhs, double *delta_c, int32_t *status, double *delta_l, double *lm_terms);
/* The host-factor part of the windows' reduced systems, built on the device: what the host layer's hostFactors forms from the factors the
 * device does not evaluate (preintegration, the marginalization prior, pose / mix / GNSS priors), bit for bit.  The partition is the resident
 * one (the W of icg_reproj_set_windows); window w owns the factor blocks [blk_off[w], blk_off[w+1]) (blk_off[0] = 0), in the order of the
 * problem's residuals.  Block b: nr[b] residuals (robust-corrected where the factor has a loss), a dense row-major nr[b] x nf[b] Jacobian of
 * the factor's free local columns, and their nf[b] columns inside the window's system (cols, block after block: distinct within a block,
 * each below Pw[w], in any order); r holds the residuals of all blocks, block after block.
 * For every window with rebuild[w] != 0 the call replaces the window's resident host part (the packed lower triangle icg_reproj_solve_windows
 * reads, of Pw[w] columns) and writes host_s / host_diag (W x P) on the leading Pw[w] columns, zeros up to P.  A window with rebuild[w] == 0 is
 * not touched, neither on the device nor in the outputs (its blocks are not read beyond nr and nf, which place the others' residuals and
 * columns).  part_out (NULL = not transferred) receives the packed triangles of the rebuilt windows, window after window.  Afterwards
 * icg_reproj_solve_windows is called with host_part_new = NULL.
 * Arithmetic: for a block, T[x][y] = sum_k J[k][x] * J[k][y] and g[x] = sum_k J[k][x] * r[k], k ascending, each sum started from +0.0 (a sum
 * of negative zeros is +0.0), one multiply and one add per term, no contraction.  Cell (a, b), a >= b, of the part starts at +0.0 and
 * receives += T[x][y], in block order, from every block that holds both columns; blocks that do not hold both add nothing.  s[c] starts at
 * +0.0 and receives -= g[x], diag[c] receives += T[x][x], in block order.  One thread owns a cell through all blocks (no atomics): a
 * window's outputs are the same bits alone, in any batch, in any batch order, and run after run.
 * Kept Jacobians: the context keeps every block's Jacobian in device memory, addressed by (window, position in the window's block list).
 * jac_off[b] >= 0: the block's Jacobian is at J + jac_off[b], is copied up and replaces the kept one; jac_off[b] == -1: the kept one is used
 * (a linearized prior's J0 is constant over a solve).  Only the Jacobians with an offset cross the link; r always does.  The kept Jacobians
 * are dropped by icg_reproj_set_windows and wherever the resident host parts are dropped (icg_reproj_solve_windows above).
 * ICG_ERR_INVALID (the message names the window and the block): no window partition, P not the resident reduced systems' P where there are
 * some, a NULL required pointer, Pw[w] outside 1 .. P, nr <= 0 or nf <= 0, a column outside [0, Pw[w]) or repeated within a block, -1 for a
 * block with no kept Jacobian or whose kept shape is not nr x nf, a rebuilt window whose block count differs from the kept one while any of
 * its blocks says -1.  ICG_ERR_CAPACITY: P > 512, nr above ICG_HOST_PART_MAX_NR, more than 65535 windows.  A rebuilt window with zero blocks
 * is valid: its part is zero.  After an error nothing was launched and no output was touched. */
#define ICG_HOST_PART_MAX_NR 1024
int icg_reproj_host_parts_build(icg_ctx *ctx, int P, const int32_t *Pw, const uint8_t *rebuild, const int32_t *blk_off, const int32_t *nr, const int32_t *nf,
                                const int32_t *cols, const int64_t *jac_off, const double *J, const double *r, double *host_s, double *host_diag,
                                double *part_out);
/* The same call for windows whose marginalization prior is resident on the device (icg_marg_prior_set) and was evaluated there
 * (icg_marg_prior_evaluate_resident): neither the prior's residual nor its Jacobian crosses the link.  The arguments of
 * icg_reproj_host_parts_build, then
 *   prior_of    one entry per block: -1 (any negative value) = the block is fed as above; p >= 0 = the block is prior p of the resident set (the
 *               set's window index, which need not be the partition's).  NULL: exactly icg_reproj_host_parts_build.
 *   prior_cols  for the prior blocks only, block after block in the order of the block list (the prior blocks of windows that are not rebuilt
 *               included: their nf places the others'): nf[b] column indices into that prior's J0, each in [0, r[p]).
 * A prior block of a rebuilt window has nr[b] == r[p].  Its residual is the resident one of the last icg_marg_prior_evaluate_resident; its
 * slots in r are placed by nr[b] like every block's but are not read.  Its Jacobian: jac_off[b] == ICG_HP_JAC_FROM_PRIOR fills the kept
 * Jacobian on the device, Jd[k][y] = J0[k][prior_cols[y]] (a copy: the values hostFactors gathers from the prior's Jacobian blocks when
 * prior_cols lists the free local columns of its blocks); -1 uses the kept one (J0 is constant between two marginalizations: the first
 * rebuild of a solve gathers, the later ones keep); an offset >= 0 uploads as above.  The gather and the copy of the residuals are one kernel
 * ahead of the unchanged accumulation (no atomics, a plain copy): the outputs are the bits icg_reproj_host_parts_build gives when it is fed
 * the same residuals and gathered columns, and a window's outputs are the same bits alone, in any batch, and run after run.
 * ICG_ERR_INVALID beyond the cases above (the message names the window and the block), for a block of a rebuilt window: prior_of[b] outside
 * the resident set, nr[b] != r[p], a prior_cols entry outside [0, r[p]), no set resident or none evaluated since it was set (icg_marg_prior_set
 * invalidates the kept residuals), prior blocks without prior_cols, ICG_HP_JAC_FROM_PRIOR for a block with prior_of[b] < 0 (or without
 * prior_of).  ICG_ERR_CAPACITY: more than 65535 prior blocks in the rebuilt windows.  After an error nothing was launched and no output was
 * touched. */
#define ICG_HP_JAC_FROM_PRIOR (-2)
int icg_reproj_host_parts_build_prior(icg_ctx *ctx, int P, const int32_t *Pw, const uint8_t *rebuild, const int32_t *blk_off, const int32_t *nr,
                                      const int32_t *nf, const int32_t *cols, const int64_t *jac_off, const double *J, const double *r, double *host_s,
                                      double *host_diag, double *part_out, const int32_t *prior_of, const int32_t *prior_cols);
/* icg_reproj_host_parts_build_prior with blocks that are factors of the resident P2 set (icg_preint_set) at the point of its last
 * icg_preint_evaluate_resident: neither the factor's residual nor its 15 x 30 Jacobian crosses the link.  The arguments of
 * icg_reproj_host_parts_build_prior, plus:
 *   preint_of    per block of the call: >= 0 = the block is factor preint_of[b] of the resident set (in any order), < 0 = it is not
 *   preint_cols  for the preintegration blocks, in block order (those of windows that are not rebuilt included), nf[b] indices into the 32
 *                columns of the factor's resident Jacobian (7 | 9 | 7 | 9): the free local columns of its non-constant parameter blocks,
 *                0-5, 7-15, 16-21, 23-31 when all four are free
 * Such a block of a rebuilt window has nr[b] == 15.  Its residual is the resident one; its slots in r are placed but not read.  Its
 * Jacobian: jac_off[b] == ICG_HP_JAC_FROM_PREINT fills the kept Jacobian with Jd[k][y] = Jf[k][preint_cols[y]] on the device (what every
 * rebuild asks for: the Jacobian changes with the point; it needs the last evaluation to have kept Jacobians), -1 keeps the previous
 * gather, an offset >= 0 uploads as for any block.  preint_of == NULL is icg_reproj_host_parts_build_prior; prior_of may be NULL.
 * ICG_ERR_INVALID beyond the cases there (the message names the window and the block), for a block of a rebuilt window: preint_of[b] outside
 * the resident set, nr[b] != 15, a preint_cols entry outside [0, 32) or 6 or 22 (the seventh pose columns), no set resident or not evaluated
 * since it was set (for ICG_HP_JAC_FROM_PREINT: not evaluated with want_jac by its last evaluation), preintegration blocks without
 * preint_cols, a block that is both prior and preintegration factor, ICG_HP_JAC_FROM_PREINT for a block with preint_of[b] < 0 (or without
 * preint_of).  ICG_ERR_CAPACITY: more than 65535 prior and preintegration blocks in the rebuilt windows.  After an error nothing was
 * launched and no output was touched. */
#define ICG_HP_JAC_FROM_PREINT (-3)
int icg_reproj_host_parts_build_preint(icg_ctx *ctx, int P, const int32_t *Pw, const uint8_t *rebuild, const int32_t *blk_off, const int32_t *nr,
                                       const int32_t *nf, const int32_t *cols, const int64_t *jac_off, const double *J, const double *r, double *host_s,
                                       double *host_diag, double *part_out, const int32_t *prior_of, const int32_t *prior_cols, const int32_t *preint_of,
                                       const int32_t *preint_cols);
/* icg_reproj_host_parts_build_preint with blocks that are factors of the resident ODOMETER P2 set (icg_preint_odo_set) at the point of its
 * last icg_preint_odo_evaluate_resident, as a third family beside the priors and the 15-state factors: neither such a factor's residual nor
 * its 19 x 32 Jacobian crosses the link.  The arguments of icg_reproj_host_parts_build_preint, plus:
 *   preint_odo_of    per block of the call: >= 0 = the block is factor preint_odo_of[b] of the resident odometer set, < 0 = it is not
 *   preint_odo_cols  for those blocks, in block order (those of windows that are not rebuilt included), nf[b] indices into the 34 columns of
 *                    the factor's resident Jacobian (7 | 10 | 7 | 10): 0-5, 7-16, 17-22, 24-33 when all four parameter blocks are free
 * Such a block of a rebuilt window has nr[b] == 19; the row stride of its source is 34.  jac_off[b] == ICG_HP_JAC_FROM_PREINT_ODO gathers
 * Jd[k][y] = Jf[k][preint_odo_cols[y]] on the device, -1 keeps the previous gather, an offset >= 0 uploads.  The three entries above are
 * this one with NULL for the arguments they do not have; the accumulation kernel is the same.
 * ICG_ERR_INVALID beyond the cases there (the message names the window and the block), for a block of a rebuilt window: preint_odo_of[b]
 * outside the resident set, nr[b] != 19, a preint_odo_cols entry outside [0, 34) or 6 or 23, no odometer set resident or not evaluated since
 * it was set (for the gather: not evaluated with want_jac), such blocks without preint_odo_cols, a block that is also a prior or a 15-state
 * factor, ICG_HP_JAC_FROM_PREINT_ODO for a block with preint_odo_of[b] < 0 (or without preint_odo_of).  ICG_ERR_CAPACITY: more than 65535
 * resident blocks of the three families in the rebuilt windows.  After an error nothing was launched and no output was touched. */
#define ICG_HP_JAC_FROM_PREINT_ODO (-4)
int icg_reproj_host_parts_build_preint_odo(icg_ctx *ctx, int P, const int32_t *Pw, const uint8_t *rebuild, const int32_t *blk_off, const int32_t *nr,
                                           const int32_t *nf, const int32_t *cols, const int64_t *jac_off, const double *J, const double *r,
                                           double *host_s, double *host_diag, double *part_out, const int32_t *prior_of, const int32_t *prior_cols,
                                           const int32_t *preint_of, const int32_t *preint_cols, const int32_t *preint_odo_of,
                                           const int32_t *preint_odo_cols);
/* icg_reproj_host_parts_build_preint_odo with blocks that are members of the resident NAV set (icg_nav_set) at the point of its last
 * icg_nav_evaluate_resident, as a fourth family: neither such a member's residual nor its Jacobian crosses the link.  The arguments of
 * icg_reproj_host_parts_build_preint_odo, plus:
 *   nav_of    per block of the call: >= 0 = the block is member nav_of[b] of the resident nav set, < 0 = it is not
 *   nav_cols  for those blocks, in block order (those of windows that are not rebuilt included), nf[b] indices into the member's block
 *             width (7, 9 or 10); index 6 of a 7-wide member (the +0.0 seventh pose column) is refused
 * Such a block of a rebuilt window has nr[b] == the member's number of residuals; the row stride of its source is the member's width.
 * jac_off[b] == ICG_HP_JAC_FROM_NAV gathers Jd[k][y] = Jm[k][nav_cols[y]] on the device, -1 keeps the previous gather, an offset >= 0
 * uploads.  The four entries above are this one with NULL for the arguments they do not have; the accumulation kernel is the same.
 * ICG_ERR_INVALID beyond the cases there (the message names the window and the block), for a block of a rebuilt window: nav_of[b] outside
 * the resident set, nr[b] != the member's, a nav_cols entry outside the width or 6 for a 7-wide member, no nav set resident or not evaluated
 * since it was set (for the gather: not evaluated with want_jac; and, once a correction of the set has marked a member, not corrected since
 * that evaluation), such blocks without nav_cols, a block that is also a member of another family, ICG_HP_JAC_FROM_NAV for a block with
 * nav_of[b] < 0 (without nav_of the value is refused as any unknown jac_off).  ICG_ERR_CAPACITY: more than 65535 resident blocks of the four families in the rebuilt windows.  After
 * an error nothing was launched and no output was touched. */
#define ICG_HP_JAC_FROM_NAV (-5)
int icg_reproj_host_parts_build_nav(icg_ctx *ctx, int P, const int32_t *Pw, const uint8_t *rebuild, const int32_t *blk_off, const int32_t *nr,
                                    const int32_t *nf, const int32_t *cols, const int64_t *jac_off, const double *J, const double *r, double *host_s,
                                    double *host_diag, double *part_out, const int32_t *prior_of, const int32_t *prior_cols, const int32_t *preint_of,
                                    const int32_t *preint_cols, const int32_t *preint_odo_of, const int32_t *preint_odo_cols, const int32_t *nav_of,
                                    const int32_t *nav_cols);
/* problem setup: pre-sizes the resident window systems and the staging memory for reduced systems of size P (a hint; optional) */
int icg_reproj_reserve_windows(icg_ctx *ctx, int P);
int icg_reproj_backsub_windows(icg_ctx *ctx, int P, const double *delta_c, double *delta_l, double *lm_terms);
int icg_reproj_cost_windows(icg_ctx *ctx, const uint8_t *active, double *cost);
/* h_ll of every landmark of the partition (n_lm values, global landmark order) from the window systems left resident by the last
 * icg_reproj_schur_windows*: icg_reproj_landmark_diag for many windows — the conditioning guard of the batched M3
 * (factors/marginalization_info.h:170-192 for the marginalizations of many streams, host/marg_batch.h). */
int icg_reproj_landmark_diag_windows(icg_ctx *ctx, double *h_ll);
/* The smallest of those diagonals per window (min_hll: W doubles), reduced on the device: the value the first conditioning guard of the
 * batched M3 tests (factors/marginalization_info.h:170-192, host/marg_batch.h step 4), so that one double per window crosses the link
 * instead of one per landmark.  Defined by the host loop over the window's landmarks in order,
 *     mn = h_ll[first];  mn = (h_ll[l] < mn) ? h_ll[l] : mn;
 * a NaN in the first landmark yields NaN, a NaN elsewhere is ignored, a window without landmarks gives 0.0.  Equal to that loop as a value;
 * the sign of a zero minimum is not specified.  ICG_ERR_INVALID as icg_reproj_landmark_diag_windows (no partition, no resident window
 * systems): nothing is launched and min_hll is not touched. */
int icg_reproj_landmark_min_windows(icg_ctx *ctx, double *min_hll);
/* the resident residuals of the last evaluation (n x 2 doubles): per-factor tests (chi-square culling) after a resident evaluation */
int icg_reproj_fetch_residuals(icg_ctx *ctx, double *out_r);
/* GVINS::removeReprojectionFactorsByChi2 (ic_gvins.cc:1269-1297) on the resident residuals of a want_jac = 0, huber = 0 evaluation:
 * factor f stays active iff it was active and NOT  (0.5 |r_f|^2) * 2.0 > chi2  (the reference's test on EvaluateResidualBlock's cost).
 * active (n bytes) is updated in place; only the flags cross the link instead of 16 bytes of residual per factor. */
int icg_reproj_chi2_cull(icg_ctx *ctx, double chi2, uint8_t *active);

/* ---- P1: preintegration inner loop (preintegration/preintegration_base.cc:39-70, preintegration_earth.cc:205-303,
 * preintegration_normal.cc:183-232), batched over independent intervals.
 * imu: total x 8 doubles (time, dt, dtheta[3], dvel[3]); interval s owns samples [offsets[s], offsets[s+1]) with
 * sample 0 = imu0.  state0: n x 16 (p3, q4 xyzw, v3, bg3, ba3).  params: 9 doubles
 * (gyr_arw, acc_vrw, gyr_bias_std, acc_bias_std, corr_time, gravity, iewn[3]).  variant: 0 Normal, 1 Earth.
 * outputs per interval: cur_state 16, delta_state 16, jac 225, cov 225, delta_time 1.
 * pn (optional, total x 4): the Earth variant's pn_ list (preintegration_earth.cc:235) — (dt, position) after sample
 * index of interval s is stored at row offsets[s] + index - 1.  Exactly those rows are written: the last row of every interval, and
 * every row in the Normal variant, keep what the caller put there.
 * ICG_ERR_INVALID (no output is touched): variant not 0 or 1, n_intervals < 0, a NULL required pointer, offsets[0] < 0, an interval
 * without a sample.  n_intervals == 0 is ICG_OK and touches nothing. */
int icg_preint_batch(icg_ctx *ctx, int variant, int n_intervals, const int32_t *offsets, const double *imu,
                     const double *state0, const double *params, double *cur_state, double *delta_state, double *jac,
                     double *cov, double *delta_time, double *pn);
/* icg_preint_batch for MANY STREAMS in one call: params is n x 9, interval s is integrated with row s (its own Earth rate, gravity and
 * noise figures), so intervals of different stations and estimators share one launch.  Every other argument, every layout and the pn rule
 * are icg_preint_batch's, and cur_state, delta_state, jac, cov, delta_time and pn of interval s have the bits icg_preint_batch returns for
 * that interval alone with that row.
 * sqrt_info (optional, n x 225) / status (optional, n; each on its own): the square-root information of every result,
 * LLT(cov^-1).matrixL()^T, formed by a second launch behind the integration on the device's cov: the bits and the status
 * icg_preint_evaluate_batch returns for that cov (status 1 and a zero matrix: singular covariance, e.g. an interval of one sample), which
 * are the host layer's Preintegration::updateSqrtInformation bit for bit.  Both NULL: the second launch is not made.
 * ICG_ERR_INVALID (nothing is launched, no output is touched; the message names the interval where there is one): variant not 0 or 1,
 * n_intervals < 0, a NULL required pointer, offsets[0] < 0, an interval without a sample.  n_intervals == 0 is ICG_OK and touches nothing. */
int icg_preint_batch_params(icg_ctx *ctx, int variant, int n_intervals, const int32_t *offsets, const double *imu,
                            const double *state0, const double *params, double *cur_state, double *delta_state, double *jac,
                            double *cov, double *delta_time, double *pn, double *sqrt_info, int32_t *status);

/* ---- P2: PreintegrationFactor::Evaluate (preintegration/preintegration_factor.h:45-69 -> PreintegrationNormal::evaluate /
 * ::residualJacobianPose0..Mix1, preintegration_normal.cc:38-142; PreintegrationEarth, preintegration_earth.cc:37-164), batched over
 * independent factors: the whitened 15-residual and its four Jacobian blocks at one evaluation point per factor.
 * Inputs per factor, in the layout icg_preint_batch writes: delta_state 16, jac 225, cov 225, delta_time 1; env 4 = gravity, iewn[3]
 * (per factor: one call serves intervals of different stations); points 32 = pose0[7] mix0[9] pose1[7] mix1[9] (p3, q4 xyzw | v3, bg3,
 * ba3).  Earth variant only: factor k owns the rows [pn_offsets[k], pn_offsets[k+1]) of pn (rows of 4: dt, position — the pn_ list,
 * preintegration_earth.cc:235, summed in row order); pn_offsets and pn may be NULL for variant 0.
 * Outputs per factor: residuals 15; jacobians 480 = 15x7 | 15x9 | 15x7 | 15x9, each row-major (NULL: residual only);
 * sqrt_info 225 = LLT(cov^-1).matrixL()^T (NULL: not returned); status 0 ok, 1 singular covariance (a zero pivot in the inversion, e.g.
 * an interval of a single IMU sample) — the output rows of such a factor are zero. */
int icg_preint_evaluate_batch(icg_ctx *ctx, int variant, int n_factors, const double *delta_state, const double *jac,
                              const double *cov, const double *delta_time, const double *env, const int32_t *pn_offsets,
                              const double *pn, const double *points, double *residuals, double *jacobians, double *sqrt_info,
                              int32_t *status);

/* ---- P1 of the odometer variants (PreintegrationOdo::integrationProcess / updateJacobianAndCovariance, preintegration_odo.cc:206-272;
 * PreintegrationEarthOdo, preintegration_earth_odo.cc:230-346; noise :289-301 / :371-383; on the two-sample integration of
 * preintegration_base.cc:39-70,86-92), batched over independent intervals like icg_preint_batch.  The error state is 19 wide
 * (dp, dv, dq, dbg, dba, ds, dsodo: s the preintegrated distance, sodo the odometer scale factor), the noise has 16 channels.
 * variant: 2 Odo, 3 EarthOdo (0 and 1 keep meaning Normal and Earth in icg_preint_batch).
 * imu9: total x 9 doubles (time, dt, dtheta[3], dvel[3], odovel: the distance increment of the sample).  state0: n x 17 (p3, q4 xyzw,
 * v3, bg3, ba3, sodo).  params25: [0..8] as icg_preint_batch, [9..11] odo_std, [12] odo_srw, [13..21] cvb = euler2matrix(abv)^T row-major
 * (formed by the caller: the installation angles themselves are not passed), [22..24] lodo.
 * Outputs per interval: cur_state 16; delta_state 20 = the 16 of icg_preint_batch, then s[3], then sodo; jac 361 and cov 361 (19 x 19
 * row-major); delta_time 1.  pn (optional, total x 4) as in icg_preint_batch, written by variant 3 only (preintegration_earth_odo.cc:261).
 * ICG_ERR_INVALID (no output is touched): variant not 2 or 3, n_intervals < 0, a NULL required pointer, offsets[0] < 0, an interval
 * without a sample.  n_intervals == 0 is ICG_OK and touches nothing. */
int icg_preint_odo_batch(icg_ctx *ctx, int variant, int n_intervals, const int32_t *offsets, const double *imu9,
                         const double *state0, const double *params25, double *cur_state, double *delta_state, double *jac,
                         double *cov, double *delta_time, double *pn);
/* icg_preint_odo_batch for many streams in one call, the 19-state twin of icg_preint_batch_params: params25 is n x 25, interval s is
 * integrated with row s; the integration outputs of interval s have the bits icg_preint_odo_batch returns for it alone with that row.
 * sqrt_info (optional, n x 361) / status (optional, n): formed behind the integration on the device's cov, the bits and the status of
 * icg_preint_odo_evaluate_batch for that cov (PreintegrationOdo::updateSqrtInformation bit for bit); both NULL: no second launch.
 * ICG_ERR_INVALID as icg_preint_batch_params, with variant 2 or 3. */
int icg_preint_odo_batch_params(icg_ctx *ctx, int variant, int n_intervals, const int32_t *offsets, const double *imu9,
                                const double *state0, const double *params25, double *cur_state, double *delta_state, double *jac,
                                double *cov, double *delta_time, double *pn, double *sqrt_info, int32_t *status);

/* ---- P2 of the odometer variants: PreintegrationFactor::Evaluate (preintegration_factor.h:45-69) -> PreintegrationOdo::evaluate /
 * ::residualJacobianPose0..Mix1 (preintegration_odo.cc:40-159); PreintegrationEarthOdo (preintegration_earth_odo.cc:41-183): the 19-state
 * twin of icg_preint_evaluate_batch.  variant: 2 Odo, 3 EarthOdo.
 * Inputs per factor, in the layout icg_preint_odo_batch writes: delta_state 20, jac 361, cov 361, delta_time 1; env 4 = gravity, iewn[3];
 * points 34 = pose0[7] mix0[10] pose1[7] mix1[10] (p3, q4 xyzw | v3, bg3, ba3, sodo: the odometer scale factor is mix[9],
 * preintegration_odo.cc:169-183).  EarthOdo only: pn_offsets / pn as in icg_preint_evaluate_batch (NULL for variant 2).
 * Outputs per factor: residuals 19; jacobians 646 = 19x7 | 19x10 | 19x7 | 19x10, each row-major (NULL: residual only); sqrt_info 361 =
 * LLT(cov^-1).matrixL()^T (NULL: not returned); status 0 ok, 1 singular covariance (a zero pivot in the inversion, e.g. odo_srw = 0 or an
 * interval of a single IMU sample) — the output rows of such a factor are zero.
 * ICG_ERR_INVALID (nothing is launched): variant not 2 or 3, n_factors <= 0, a NULL required pointer, pn_offsets missing, negative or not
 * monotone for variant 3, rows without pn. */
int icg_preint_odo_evaluate_batch(icg_ctx *ctx, int variant, int n_factors, const double *delta_state, const double *jac,
                                  const double *cov, const double *delta_time, const double *env, const int32_t *pn_offsets,
                                  const double *pn, const double *points, double *residuals, double *jacobians, double *sqrt_info,
                                  int32_t *status);

/* ---- P2 on a RESIDENT set of factors: what an integration result contributes to its factor is constant over a solve while every LM
 * iteration evaluates it at a new point, so it is uploaded once (icg_preint_set) and an evaluation ships the points up and one squared norm
 * per factor back (icg_preint_evaluate_resident); the whitened residuals and Jacobians stay on the device.
 * The device calls no sin / cos / sqrt here: the two quaternions of Preintegration::evaluate that need them come from the host
 * (Preintegration::earthRateQuaternion with the set, Preintegration::correctionQuaternion with every point), and what is left is + - * /
 * in the host's order, compiled without contraction on both sides: residuals, Jacobians and sq_norm have the bits of
 * Preintegration::evaluate given the same sqrt_info.
 * Per factor f, in the layout of icg_preint_evaluate_batch: variant[f] (0 Normal, 1 Earth: one set serves mixed windows), delta_state 16,
 * jac 225, delta_time 1, env 4; sqrt_info 225 is the host's square-root information (shipped, not recomputed: a factor with a singular
 * covariance does not belong in a set); q_nn 4 = rotvec2quat(-iewn T) as (x, y, z, w), read for Earth factors only; Earth factor f owns the
 * rows [pn_offsets[f], pn_offsets[f+1]) of pn (the rows of a Normal factor are not read).  pn_offsets / pn may be NULL when no factor is Earth.
 * Replaces the set the context held; the set stays until the next icg_preint_set or icg_ctx_destroy.  ICG_ERR_INVALID (the message names the
 * factor where there is one): n_factors <= 0, a NULL required pointer, a variant outside {0, 1}, pn_offsets[0] < 0 or not monotone, an Earth
 * factor without pn_offsets, rows without pn.  ICG_ERR_CAPACITY: more than ICG_PREINT_SET_MAX factors.  After a failed call no set is
 * resident. */
#define ICG_PREINT_SET_MAX (65535 * 16)
int icg_preint_set(icg_ctx *ctx, int n_factors, const int32_t *variant, const double *delta_state, const double *jac, const double *sqrt_info,
                   const double *delta_time, const double *env, const double *q_nn, const int32_t *pn_offsets, const double *pn);
/* Evaluates every factor of the resident set: points 32 per factor (pose0[7] mix0[9] pose1[7] mix1[9]), q_corr 4 per factor =
 * rotvec2quat(dq_dbg (bg0 - delta.bg)) as (x, y, z, w), used in place of the device's own.  Kept on the device, in buffers the set owns,
 * until the next evaluation or icg_preint_set: the whitened residuals (15 per factor) and, with want_jac != 0, the whitened Jacobian as ONE
 * row-major 15 x 32 matrix per factor, columns 7 | 9 | 7 | 9 (columns 6 and 22, the seventh pose columns, are +0.0).  Returned:
 * sq_norm[f] = sum_k r[k]^2, k ascending from +0.0 (twice the Ceres cost of a factor without a loss).  An evaluation with want_jac == 0
 * invalidates the kept Jacobians.  ICG_ERR_INVALID without a resident set or with a NULL argument: nothing is launched. */
int icg_preint_evaluate_resident(icg_ctx *ctx, const double *points, const double *q_corr, int want_jac, double *sq_norm);
/* The kept results of the last icg_preint_evaluate_resident in the layout of icg_preint_evaluate_batch: residuals 15 per factor, jacobians
 * 480 per factor = 15x7 | 15x9 | 15x7 | 15x9 (NULL: not fetched).  For tests and callers that want them (as icg_reproj_fetch_residuals).
 * ICG_ERR_INVALID: no resident set, NULL residuals, nothing evaluated since icg_preint_set, or Jacobians asked for after an evaluation with
 * want_jac == 0. */
int icg_preint_fetch_resident(icg_ctx *ctx, double *residuals, double *jacobians);

/* ---- P2 of the odometer variants on a RESIDENT set of factors: the 19-state twins of the three entries above, with a resident set of their
 * own (a context may hold a 15-state set and an odometer set at once; neither entry touches the other's).  The device calls no sin / cos /
 * sqrt: the two quaternions come from the host (PreintegrationOdo::earthRateQuaternion with the set, PreintegrationOdo::correctionQuaternion
 * with every point), and what is left is + - * / in the host's order without contraction: residuals, Jacobians and sq_norm have the bits of
 * PreintegrationOdo::evaluate given the same sqrt_info.
 * Per factor f, in the layout icg_preint_odo_batch writes: variant[f] (2 Odo, 3 EarthOdo: one set serves mixed windows), delta_state 20,
 * jac 361, delta_time 1, env 4 = gravity, iewn[3]; sqrt_info 361 is the host's square-root information (shipped, not recomputed); q_nn 4 =
 * rotvec2quat(-iewn T) as (x, y, z, w), read for EarthOdo factors only; EarthOdo factor f owns the rows [pn_offsets[f], pn_offsets[f+1]) of
 * pn (the rows of an Odo factor are not read).  pn_offsets / pn may be NULL when no factor is EarthOdo.
 * Replaces the odometer set the context held; it stays until the next icg_preint_odo_set or icg_ctx_destroy.  ICG_ERR_INVALID (the message
 * names the factor where there is one): n_factors <= 0, a NULL required pointer, a variant outside {2, 3}, pn_offsets[0] < 0 or not
 * monotone, an EarthOdo factor without pn_offsets, rows without pn.  ICG_ERR_CAPACITY: more than ICG_PREINT_SET_MAX factors.  After a failed
 * call no odometer set is resident. */
int icg_preint_odo_set(icg_ctx *ctx, int n_factors, const int32_t *variant, const double *delta_state, const double *jac, const double *sqrt_info,
                       const double *delta_time, const double *env, const double *q_nn, const int32_t *pn_offsets, const double *pn);
/* Evaluates every factor of the resident odometer set: points 34 per factor (pose0[7] mix0[10] pose1[7] mix1[10]), q_corr 4 per factor =
 * rotvec2quat(dq_dbg (bg0 - delta.bg)) as (x, y, z, w).  Kept on the device until the next evaluation or icg_preint_odo_set: the whitened
 * residuals (19 per factor) and, with want_jac != 0, the whitened Jacobian as ONE row-major 19 x 34 matrix per factor, columns
 * 7 | 10 | 7 | 10 (columns 6 and 23, the seventh pose columns, are +0.0).  Returned: sq_norm[f] = sum_k r[k]^2, k ascending from +0.0.  An
 * evaluation with want_jac == 0 invalidates the kept Jacobians.  ICG_ERR_INVALID without a resident set or with a NULL argument: nothing is
 * launched. */
int icg_preint_odo_evaluate_resident(icg_ctx *ctx, const double *points, const double *q_corr, int want_jac, double *sq_norm);
/* The kept results of the last icg_preint_odo_evaluate_resident in the layout of icg_preint_odo_evaluate_batch: residuals 19 per factor,
 * jacobians 646 per factor = 19x7 | 19x10 | 19x7 | 19x10 (NULL: not fetched).  For tests.  ICG_ERR_INVALID: no resident set, NULL residuals,
 * nothing evaluated since icg_preint_odo_set, or Jacobians asked for after an evaluation with want_jac == 0. */
int icg_preint_odo_fetch_resident(icg_ctx *ctx, double *residuals, double *jacobians);

/* ---- The small navigation factors (host/nav_factors.h), RESIDENT on the device for a whole solve, beside the prior, the 15-state and the
 * odometer sets (a context may hold one of each; none of these entries touches another set).  Member f has a kind and one parameter block:
 *   kind 0 GnssFactor          3 x 7    constants blh3, std3, lever3 (9)      kind 3 ImuMixPriorFactor       9 x 9    mix9, std9 (18)
 *   kind 1 ImuErrorFactor      6 x 9    none                                  kind 4 ImuErrorFactor, odo     7 x 10   none
 *   kind 2 ImuPosePriorFactor  6 x 7    pose7, std6 (13)                      kind 5 ImuMixPriorFactor, odo  10 x 10  mix10, std10 (20)
 * icg_nav_set: n members; the constants of member f are aux[aux_off[f] .. aux_off[f + 1]) (aux_off has n + 1 entries; a member may own
 * more doubles than its kind reads, never fewer).  Replaces the nav set the context held.  ICG_ERR_INVALID (the message names the member
 * where there is one): n <= 0, a NULL argument, a kind outside 0..5, aux_off[0] < 0 or offsets that are not monotone, fewer constants than
 * the kind reads.  ICG_ERR_CAPACITY: more than ICG_NAV_SET_MAX members.  After a failed call no nav set is resident. */
#define ICG_NAV_SET_MAX 65535
int icg_nav_set(icg_ctx *ctx, int n, const int32_t *kind, const int32_t *aux_off, const double *aux);
/* Evaluates every member at its parameter block points[point_off[f] ..] (7, 9 or 10 doubles; point_off[f] >= 0).  Kept on the device until
 * the next evaluation or icg_nav_set: the residuals, concatenated (nr[f] each, member after member), and with want_jac != 0 one row-major
 * nr x width Jacobian per member, concatenated; every element of it is written by every such evaluation, zeros as the host writes them
 * (the seventh pose columns are +0.0).  Returned: sq_norm[f] = sum_k r[k]^2, k ascending from +0.0.  The arithmetic is the classes'
 * Evaluate, operation for operation without contraction: the host's bit patterns.  want_jac == 0 invalidates the kept Jacobians.
 * ICG_ERR_INVALID without a resident set, with a NULL argument or a negative point_off: nothing is launched. */
int icg_nav_evaluate_resident(icg_ctx *ctx, const double *points, const int32_t *point_off, int want_jac, double *sq_norm);
/* The Ceres corrector of the robustified members (ResidualBlockInfo::Evaluate, host/marginalization.cc) applied to what the last evaluation
 * kept.  robust[f] != 0 marks a member; corr holds 3 doubles per member (read for the marked ones): sqrt_rho1, alpha_sq_norm,
 * residual_scaling — the host's (host/marginalization.h correctorScalars), no sqrt is taken on the device.  For a marked member, per column c:
 * rtj = sum_k r[k] J[k][c], k ascending from +0.0; J[k][c] = sqrt_rho1 * (J[k][c] - alpha_sq_norm * r[k] * rtj); then r[k] *= residual_scaling.
 * Unmarked members keep their bits.  A call that marks a member makes the set one with robustified members until the next icg_nav_set: the
 * host-part gather (icg_reproj_host_parts_build_nav) then waits for the correction of every evaluation.  Allowed once per evaluation with Jacobians: ICG_ERR_INVALID (nothing launched) for a second call, after a
 * residual-only evaluation, without a resident set or an evaluation, or with a NULL argument. */
int icg_nav_correct_resident(icg_ctx *ctx, const uint8_t *robust, const double *corr);
/* The kept residuals (sum nr) and Jacobians (sum nr x width; NULL: not fetched) of the last evaluation, corrected where a correction ran.
 * For tests.  ICG_ERR_INVALID: no resident set, NULL residuals, nothing evaluated since icg_nav_set, or Jacobians asked for after an
 * evaluation with want_jac == 0. */
int icg_nav_fetch_resident(icg_ctx *ctx, double *residuals, double *jacobians);

/* ---- M4: MarginalizationFactor::Evaluate (factors/marginalization_factor.h:47-101) for the priors of many windows, RESIDENT on the
 * device: a prior is constant between two marginalizations while every LM iteration evaluates it at a new point, so the priors are
 * uploaded once (icg_marg_prior_set) and an evaluation ships only x in and the results out (icg_marg_prior_evaluate).
 * Window w: retained size r[w] (1 .. ICG_MARG_MAX_R), blocks [block_off[w], block_off[w+1]) (block_off[0] = 0).  Block b: global size
 * block_size[b] (7 = pose, local size 6; otherwise local = global), first local column block_index[b] (the remained block index minus
 * the marginalized size).  Blocks may be listed in any column order and need not cover every column (an uncovered column has dx = 0);
 * they must not overlap.  Windows of one set may differ in r and layout.
 * x0: linearization point, the blocks' parameters concatenated by global size, window after window; J0: linearized_jacobians, r x r
 * row-major per window, concatenated; e0: linearized_residuals, r per window.
 * Replaces the set the context held; the set stays until the next icg_marg_prior_set or icg_ctx_destroy.  ICG_ERR_INVALID (message
 * names the window): n_windows <= 0, NULL pointer, r <= 0, block_off not monotone, a block with size <= 0, index < 0 or index + local
 * size > r.  ICG_ERR_CAPACITY: r above ICG_MARG_MAX_R or more than 65535 windows.  After a failed call no set is resident. */
#define ICG_MARG_MAX_R 1024
int icg_marg_prior_set(icg_ctx *ctx, int n_windows, const int32_t *r, const int32_t *block_off, const int32_t *block_size,
                       const int32_t *block_index, const double *x0, const double *J0, const double *e0);
/* Evaluates every resident prior (factors/marginalization_factor.h:47-101) at x (laid out like x0).  dx per block as :61-77 (pose:
 * position difference and sign(dq.w) * 2 * vec(q0^-1 * q), a zero-norm q0 yields the reference's inf / NaN, not an error);
 * residuals (sum of r[w]): e = e0 + J0 * dx, every row summed from 0 in column order with one multiply and one add per term — the same
 * IEEE value as the host code, in any batch.  Optional outputs, NULL = not computed and not transferred:
 *   jacobians  per window its blocks concatenated, block b an r x block_size[b] row-major matrix (columns >= local size are 0): the
 *              blocks Ceres hands to Evaluate (:83-98); r[w] * sum(block_size) doubles per window
 *   gradient   J0^T e per window (sum of r[w]), every column summed from 0 in row order
 *   sq_norm    e . e per window (n_windows), summed from 0 in row order (twice the Ceres cost)
 * ICG_ERR_INVALID without a resident set or with NULL x / residuals. */
int icg_marg_prior_evaluate(icg_ctx *ctx, const double *x, double *residuals, double *jacobians, double *gradient, double *sq_norm);
/* The same evaluation of every resident prior at x (laid out like x0) with the residuals LEFT on the device, in a buffer the set owns, for
 * icg_reproj_host_parts_build_prior: only x crosses the link on the way in and sq_norm (n_windows: e . e per window) on the way out.  The
 * arithmetic is icg_marg_prior_evaluate's: sq_norm[w] has the bits that call returns.  The kept residuals are those of the last call;
 * icg_marg_prior_set invalidates them.  ICG_ERR_INVALID without a resident set or with a NULL x / sq_norm: nothing is launched. */
int icg_marg_prior_evaluate_resident(icg_ctx *ctx, const double *x, double *sq_norm);

/* ---- M3: the Schur step on the marginalized pose / mix block and the linearization (factors/marginalization_info.h:153-192) for the
 * reduced systems of many windows, one workgroup per window.  Window w: H (P[w] x P[w], row-major) and b (P[w]), concatenated window after
 * window; the m[w] leading columns are eliminated (0 <= m < P; m = 0: Hp = H, bp = b), r = P - m remain.
 *   :170-192  Hmm = (H + H^T) / 2 on the m leading columns, its eigen-decomposition, inv_k = ev_k > eps ? 1 / ev_k : 0, Hinv from its
 *             lower triangle, T = Hrm Hinv, Hp = Hrr - T Hmr, bp = br - T bm
 *   :153-167  eigen-decomposition of Hp (eigenvalues ascending), J0[k][i] = sqrt(S_k) V[i][k], e0[k] = sqrt(Sinv_k) sum_i V[i][k] (-bp[i])
 *             with S_k = ev_k > eps ? ev_k : 0, Sinv_k = ev_k > eps ? 1 / ev_k : 0
 * The eigen-solver is the host layer's (Householder tridiagonalisation, implicit QL, 60 iterations per eigenvalue at most); every sum is
 * one thread's chain from 0 in the host's index order, one multiply and one add per term.  Only hypot may round differently from the host.
 * Outputs per window, concatenated: J0 (r x r row-major) and e0 (r) are required.  Optional, NULL = not computed / not transferred:
 *   Hp (r x r), bp (r), evals (r: the eigenvalues of Hp, ascending), min_ev_m (1: smallest eigenvalue of the m-block, +inf for m = 0),
 *   status (1, a bit set: 1 = a QL sweep hit its iteration cap, 2 = an eigenvalue of the m-block <= eps, 4 = an eigenvalue of Hp <= eps —
 *   a rank-deficient Hp is normal, bit 4 is information).
 * A window's outputs are the same bits alone, in any batch, in any batch order and run after run.
 * ICG_ERR_INVALID (the message names the window): n_windows <= 0, a NULL required pointer, eps < 0, P <= 0 or m outside [0, P).
 * ICG_ERR_CAPACITY (window named): P above ICG_MARG_LIN_MAX_P, more than 65535 windows.  After an error nothing was launched and no output
 * was touched. */
#define ICG_MARG_LIN_MAX_P 512
int icg_marg_linearize_batch(icg_ctx *ctx, int n_windows, const int32_t *P, const int32_t *m, const double *H, const double *b, double eps,
                             double *Hp, double *bp, double *J0, double *e0, double *evals, double *min_ev_m, int32_t *status);

/* ---- M3 -> M4 on the device: the linearization (factors/marginalization_info.h:153-192) stays where the prior evaluation
 * (factors/marginalization_factor.h:47-101) reads it.
 * icg_marg_linearize_batch_keep is icg_marg_linearize_batch — the same kernels, launches, argument checks and the same bits in every
 * output — and also leaves J0 / e0 of every window in a buffer the context owns (sum r^2 + sum r doubles: 41 MB for 256 windows of
 * r = 142).  J0 and e0 may be NULL here (not transferred).  *keep_id receives the id of the kept linearization: non-zero, unique in the
 * process and never reused; 0 after a failed call.  The kept linearization lives until the first of: the next icg_marg_linearize_batch or
 * icg_marg_linearize_batch_keep call on the context (whether that call succeeds or not), icg_marg_linearized_release, icg_ctx_destroy.
 * ICG_ERR_INVALID also for a NULL keep_id. */
int icg_marg_linearize_batch_keep(icg_ctx *ctx, int n_windows, const int32_t *P, const int32_t *m, const double *H, const double *b, double eps,
                                  double *Hp, double *bp, double *J0, double *e0, double *evals, double *min_ev_m, int32_t *status,
                                  uint64_t *keep_id);
/* ---- M2 -> M3 on the device: M3 (factors/marginalization_info.h:153-192) on reduced systems that never left the device.  The M2 system of a
 * window (factors/marginalization_info.h:195-230, landmark-eliminated) is the sum of its host-evaluated factors' J^T J, resident as a packed
 * lower triangle after icg_reproj_host_parts_build, and of S, whose lower triangle is resident after icg_reproj_schur_windows_resident
 * (P columns, row stride P).  For k in [0, n_sel) system k is window win[k] of the partition, Pw[k] x Pw[k]; one kernel forms, for i >= j,
 *     H[i][j] = H[j][i] = part[i (i + 1) / 2 + j] + S_w[i * P + j]
 * (the part first, then S; a window without a resident part takes +0.0 as its part and the addition is still made) in a buffer of the
 * context, and the kernels of icg_marg_linearize_batch run unchanged on it: every output holds the bits that call returns for these H and b.
 * b: the Pw[k] right-hand sides, concatenated (the caller adds host_s + s).  Outputs: as icg_marg_linearize_batch, concatenated in list
 * order; H_out (optional, sum Pw^2 doubles): the formed systems.  keep_id == NULL: the plain form, J0 / e0 are required.  keep_id != NULL: the
 * keep form, J0 / e0 may be NULL, system k is kept window k; lifetime and id rules are icg_marg_linearize_batch_keep's.
 * The resident S and parts are only read: icg_reproj_solve_windows works afterwards as before.
 * ICG_ERR_INVALID (the message names the list position and the window): no resident reduced systems of P columns, a NULL required pointer,
 * n_sel <= 0, win[k] outside the partition or listed twice, Pw[k] outside 1 .. P, a resident part whose column count is not Pw[k], m[k]
 * outside [0, Pw[k]), eps < 0.  ICG_ERR_CAPACITY as icg_marg_linearize_batch.  After an error nothing was launched and no output was
 * touched; the linearization the context kept is dropped by every call, failed or not. */
int icg_marg_linearize_resident(icg_ctx *ctx, int P, int n_sel, const int32_t *win, const int32_t *Pw, const int32_t *m, const double *b,
                                double eps, double *Hp, double *bp, double *J0, double *e0, double *evals, double *min_ev_m, int32_t *status,
                                double *H_out, uint64_t *keep_id);
/* Drops the linearization the context keeps, if any (its id is no longer known; the memory is reused by the next kept one). */
int icg_marg_linearized_release(icg_ctx *ctx);
/* icg_marg_prior_set (factors/marginalization_factor.h:47-101) with J0 / e0 taken from a kept linearization
 * (factors/marginalization_info.h:153-192): the same metadata, the same resident J / J^T / e0 / x0, the same replacement and invalidation
 * rules, the same bits in every later evaluation.  Window w takes J0 / e0 from window src[w] of linearization keep_id when src[w] >= 0 (a
 * kept window may serve several windows of the set, in any order) and from J0_host / e0_host when src[w] == -1: these hold only the -1
 * windows, concatenated in set order, and may be NULL when there are none (keep_id is not looked at when every window is -1).
 * The kept linearization may belong to ctx itself or to another context on the same device; the CALLER guarantees that the owning context
 * is inside no call (and is not destroyed) while this one runs.  A live id is never followed to freed memory: an id whose linearization is
 * gone is refused.
 * ICG_ERR_INVALID (message names the window where there is one): everything icg_marg_prior_set reports; NULL src; src[w] outside
 * [-1, kept windows); keep_id unknown or expired ("the kept linearization ... is gone"); r[w] != the kept window's r; a -1 window with NULL
 * host arrays; the owning context on another device.  ICG_ERR_CAPACITY as there.  After a failed call nothing was launched and no set is
 * resident. */
int icg_marg_prior_set_from_kept(icg_ctx *ctx, uint64_t keep_id, int n_windows, const int32_t *src, const int32_t *r, const int32_t *block_off,
                                 const int32_t *block_size, const int32_t *block_index, const double *x0, const double *J0_host,
                                 const double *e0_host);

/* ---- the reduced camera solve: solver_detail::choleskySolve of the host layer (host/dense_kernels.cc) for many systems at once, one wave per
 * system (csrc/chol.hip).  The systems are concatenated: system k is A (n[k] x n[k], row-major, only the lower triangle is read) and b (n[k]).
 * The arithmetic is the host's, operation for operation: column tiles of two, every inner product in dot8 order (eight interleaved partial
 * sums combined as ((p0+p4)+(p2+p6))+((p1+p5)+(p3+p7)), then the tail in order), one multiply and one add per term, IEEE division and square
 * root — x, L and status are the bits the host produces.
 *   x       required; sum of n[k] doubles.  The solution, or zeros for a system with status 1.
 *   L       optional (NULL = not transferred); the factor's lower triangle in A's layout.  Elements above the diagonal are not written, and
 *           nothing of a system with status 1.
 *   status  optional; 0 ok, 1 not positive definite or non-finite (a pivot d with !(d > 0) or !isfinite(d), tested in the host's order).
 * A failed system does not affect the others.  A system's outputs are the same bits alone, in any batch, in any batch order and run after run.
 * ICG_ERR_INVALID (the message names the system): n_systems <= 0, a NULL required pointer, n <= 0.  ICG_ERR_CAPACITY (system named): n above
 * ICG_CHOL_MAX_N, more than 65535 systems.  After an error nothing was launched and no output was touched. */
#define ICG_CHOL_MAX_N 512
int icg_chol_solve_batch(icg_ctx *ctx, int n_systems, const int32_t *n, const double *A, const double *b, double *x, double *L,
                         int32_t *status);

/* ---- f3 (SURVEY.md §8 "next" row): per-observation arithmetic of GVINS::gvinsOutlierCulling (ic_gvins.cc:1035-1128) and
 * GVINS::parametersStatistic (ic_gvins.cc:930-1033).  Observation i = landmark lm_idx[i] (world position pw, n_lm x 3) seen in
 * keyframe pose_idx[i] (poses12: n_poses x 12, R row-major camera->world | t) at the undistorted key point pix[i]:
 *   err_out[i]  = |Camera::reprojectionError(pose, pw, pp)|                (tracking/camera.cc:153-157)
 *   good_out[i] = Tracking::isGoodToTrack(pp, pose, pw, scale, depth_scale)  (tracking/tracking.cc:813-829) with
 *                 max_error = reprojection_error_std * scale, min_depth = MapPoint::NEAREST_DEPTH,
 *                 max_depth = MapPoint::FARTHEST_DEPTH * depth_scale.
 * The camera set with icg_set_camera is used. */
int icg_reproj_error_batch(icg_ctx *ctx, int n, const int32_t *pose_idx, const int32_t *lm_idx, int n_poses, const double *poses12,
                           int n_lm, const double *pw, const float *pix, double max_error, double min_depth, double max_depth,
                           double *err_out, uint8_t *good_out);
/* The same with one camera index per POSE: an observation is projected with camera pose_cam[pose_idx[i]] of the context's table
 * (icg_set_cameras) — the windows of several GVINS instances, each culled with its own camera_ (ic_gvins.cc:1068-1078, :985), in one launch.
 * ICG_ERR_INVALID, nothing launched and no output touched: no table set, pose_cam NULL, an index outside the table, and
 * icg_reproj_error_batch's. */
int icg_reproj_error_batch_cams(icg_ctx *ctx, int n, const int32_t *pose_idx, const int32_t *lm_idx, int n_poses, const double *poses12,
                                const int32_t *pose_cam, int n_lm, const double *pw, const float *pix, double max_error, double min_depth,
                                double max_depth, double *err_out, uint8_t *good_out);

/* ---- f4 (SURVEY.md §8 "next" row): the INS steps in front of the tracker, batched over independent streams -----------
 * Layouts: imu rows of 8 doubles (time, dt, dtheta[3], dvel[3]); state rows of 23 doubles (time, p3, q4 xyzw, v3, bg3, ba3,
 * sg3, sa3 = IntegrationState, preintegration/integration_state.h:35-52 without the odometer fields);
 * cfg8 = gravity[3], iewn[3], iswithearth, iswithscale (IntegrationConfiguration, integration_state.h:91-99).
 *
 * icg_ins_mechanize_batch: MISC::insMechanization (misc.cc:151-206) applied in sequence to the samples
 * offsets[s]+1 .. offsets[s+1]-1 of stream s (sample offsets[s] is imu_pre of the first step), starting from states23[s]
 * (updated in place to the state after the last sample).  traj23 (optional, total x 23): row offsets[s] = the start state,
 * row offsets[s]+k = the state after sample k — i.e. the (IMU, state) window the reference keeps in ins_window_
 * (ic_gvins.cc:270-290) and re-propagates in MISC::redoInsMechanization (misc.cc:208-261). */
int icg_ins_mechanize_batch(icg_ctx *ctx, int n_streams, const int32_t *offsets, const double *imu, const double *cfg8,
                            double *states23, double *traj23);
/* icg_ins_camera_pose_batch: the INS pose prior of n frames, MISC::getCameraPoseFromInsWindow (misc.cc:67-83) after its
 * bracket search: brackets16[i] = (time, p3, q4) of the window states before and after times[i]; interp[i] != 0 ->
 * statePoseInterpolation (misc.cc:85-100), interp[i] == 0 -> the first state as is (the reference's fallback to the newest
 * state when the time is outside the window); then stateToCameraPose (misc.cc:102-108) with the body->camera extrinsic
 * pose_b_c12 (R row-major 9, t 3).  pose12_out: n x 12, same layout (camera->world). */
int icg_ins_camera_pose_batch(icg_ctx *ctx, int n, const double *brackets16, const int32_t *interp, const double *pose_b_c12,
                              const double *times, double *pose12_out);

/* ---- device-resident tracker of a stream group (round 4) ---------------------------------------------------------------------
 * Replaces, for n independent camera streams at once, everything Tracking::track (tracking/tracking.cc:144-245) does BETWEEN its image
 * primitives: the state machine (first frame / initializing / tracking / lost), trackMappoint (:351-455), trackReferenceFrame (:457-574),
 * reduceVector (:831-845), the parallax sums and keyframe decision (:263-307, 873-922), triangulation bookkeeping (:690-798), the detection
 * lists (:576-688), and — as the throughput harness does for GVINS — the sliding-window side effects on the map (map.cc:27-127).  The
 * per-stream state (frames with their feature rows in the reference container's iteration order, map points, candidate lists, window) is
 * one flat block per stream in HBM; a step is ONE chain of launches on the context's stream — stage kernel, primitive, stage kernel, ... —
 * with the work lists of every primitive left in device memory by the stage kernel before it, and ONE wait at the end.  The host never
 * builds a list, never sizes a grid from results and never reads the tracker's state unless it asks for a block.
 *
 * The stage bodies are the functions of ic-gvins_amd/host/track_core.h, compiled for gfx950; the same source compiled for the host is the
 * CPU twin the parity tests pin against the track table and the reference's own tracker.  icg_tracker_config mirrors tc::Cfg of that file
 * (static_assert in csrc/tracker.hip); a block is sizeof(tc::Stream) bytes = icg_tracker_block_bytes(). */
typedef struct icg_tracker icg_tracker;
typedef struct icg_tracker_config {
    double fx, fy, cx, cy, skew, k1, k2, p1, p2, k3; /* camera (icg_camera) */
    int32_t width, height;
    int32_t track_max_features, check_histogram, window_size, pad0;
    double track_min_parallax, reprojection_error_std, track_max_interval; /* track_max_interval already x 0.95 (tracking.cc:57) */
    int32_t block_cols, block_rows, block_cnts, block_w, block_h, max_block_features, min_pixel_distance, max_per_job; /* tracking.cc:66-85 */
    uint64_t stream_id_base;
} icg_tracker_config;
typedef struct icg_tracker_result { /* per stream, after a step */
    int32_t active;          /* the stream had a frame in this step */
    int32_t state;           /* TrackState of the frame (tracking.h:38-44) */
    int32_t is_new_keyframe; /* Tracking::isNewKeyFrame() */
    int32_t overflow;        /* != 0: a capacity of the block was exceeded (the step fails) */
    int32_t n_features, n_candidates, window_keyframes, landmarks;
    uint64_t frames, keyframes, tracked_sum, digest; /* running statistics / digest of everything index-like the stream produced */
    uint64_t frame_id, keyframe_id, mappoint_id, last_input_fid; /* id factories (frame.cc:37-53, mappoint.cc:45-49) */
    int32_t need_detect_a;   /* the stream's next frame starts with a detection (first frame / initialization without candidates) */
    int32_t n_log;           /* landmark-container operations logged in the block since the last drain */
    int32_t lk_points, detect_jobs, ransac_sets, tri_points; /* work this frame handed to the primitives */
    /* the frame's line of tracking.txt (tracking.cc:236-238, 309-315), when it has one: stamp, dt, parallax, translation, rotation [deg] as
     * kept at the keyframe decision, and the frame's feature count before the window keeper ran; the caller appends its own time cost */
    int32_t log_valid, log_features;
    double log_data[5];
} icg_tracker_result;

/* buckets_after[k], k = 0..n_buckets_after-1: bucket count of a fresh std::unordered_map<ulong, T> after k insertions on the host's standard
 * library (the reference container whose iteration order the feature rows keep); n_buckets_after must cover the row capacity + 2. */
int icg_tracker_create(icg_ctx *ctx, int n_streams, const icg_tracker_config *cfg, const uint32_t *buckets_after, int n_buckets_after,
                       icg_tracker **out);
/* A tracker with a camera per stream: stream s tracks with camera stream_cam[s] of the context's table (icg_set_cameras), as the Tracking
 * the reference constructs for that camera would (tracking/tracking.h:51); stream_cam NULL means camera s and needs n_cams >= n_streams.
 * The camera fields of cfg are ignored (width / height are not).  The tracker copies the cameras it uses: a later icg_set_cameras on the
 * context does not move a live tracker's.  ICG_ERR_INVALID (no tracker is created): no table set, an index outside the table, NULL
 * stream_cam with fewer cameras than streams, and icg_tracker_create's. */
int icg_tracker_create_cams(icg_ctx *ctx, int n_streams, const icg_tracker_config *cfg, const int32_t *stream_cam,
                            const uint32_t *buckets_after, int n_buckets_after, icg_tracker **out);
void icg_tracker_destroy(icg_tracker *t);
size_t icg_tracker_block_bytes(void);
/* One frame per stream: images[k] (stride / channels as icg_frames_preprocess; NULL = stream k idles this step), its stamp and INS pose
 * prior (R row-major 9, t 3).  Returns after the whole chain has run; results[k] is filled for every stream. */
int icg_tracker_step(icg_tracker *t, const uint8_t *const *images, int stride, int channels, int images_on_device, const double *stamps,
                     const double *poses12, icg_tracker_result *results);
/* the block of one stream, to / from host memory (B2 view, dumps, optimizer write-back); both wait for the context's stream */
int icg_tracker_download(icg_tracker *t, int stream, void *block);
int icg_tracker_upload(icg_tracker *t, int stream, const void *block);
/* the landmark-container history of a stream has been replayed by the host: restart it (n_log = 0) */
int icg_tracker_reset_log(icg_tracker *t, int stream);
/* The same without the block: the first counts[k] entries (16 bytes each: id u64, map-point index u32, op i32 — 1 insert, 0 erase) of the
 * history of streams[k] are copied to out + k * entry_stride entries and the history restarts; one wait for all n_req streams.  counts[k]
 * is the n_log the stream's last result reported. */
int icg_tracker_fetch_logs(icg_tracker *t, int n_req, const int32_t *streams, const int32_t *counts, void *out, int entry_stride);

#ifdef __cplusplus
}
#endif
#endif /* ICGVINS_HIP_H */
