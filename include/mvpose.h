/*
 * mvpose.h — C-ABI of libmvpose.so, the MI355X-native (gfx950) multi-view 3D
 * pose hot path.  Drop-in boundary for the reference's per-frame
 * 2D-detect -> DLT-triangulate loop and its reprojection SGD
 * (sashapersonxyz/Multi-camera_3D_Pose_Estimation).
 *
 * Conventions
 *   - Every pointer named *_dev is a DEVICE pointer owned by the caller
 *     (e.g. a torch tensor's data_ptr()).  Pointers named *_host are host
 *     memory read synchronously during the call.
 *   - Every compute call takes a stream (a hipStream_t passed as void*; NULL =
 *     the default stream) and is asynchronous, stream-ordered work.
 *   - Every function returns int: MVP_OK (0) or a negative MVP_ERR_* code; it
 *     never throws across the ABI.  mvp_last_error() returns the message of the
 *     calling thread's last failure.
 *   - Handles may be used from one thread at a time; distinct handles/streams
 *     are independent.
 *   - No torch, numpy or C++ types cross this boundary.
 */
#ifndef MVPOSE_H
#define MVPOSE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVP_ABI_VERSION 1

#define MVP_OK 0
#define MVP_ERR_ARG (-1)      /* invalid argument / shape */
#define MVP_ERR_HIP (-2)      /* HIP runtime error */
#define MVP_ERR_NOMEM (-3)    /* allocation failure */
#define MVP_ERR_INTERNAL (-4) /* unexpected internal failure */

int mvp_abi_version(void);
const char* mvp_last_error(void);

/* ---------------------------------------------------------------------------
 * Camera parameter block: one MVP_CAM_DOUBLES-double record per camera,
 *   [ K(3x3 row-major) | dist(k1,k2,p1,p2,k3) | R(3x3) | T(3) | P = K[R|T] (3x4) | pad(2) ]
 * K/dist/R/T are utils.get_params_from_name's values (reference utils.py:807-828);
 * P is computed by the caller exactly as utils.py:1318-1319 does (np.dot, fp64),
 * or with mvp_camera_pack.
 * ------------------------------------------------------------------------- */
#define MVP_CAM_DOUBLES 40

/* Host helper: pack one camera record (P = K·[R|T] in fp64, row-major loops). */
int mvp_camera_pack(const double* K_host, const double* dist5_host, const double* R_host,
                    const double* T_host, double* out_record_host);

/* ---------------------------------------------------------------------------
 * Triangulation (replaces pose_estimation.get_pose_3D, pose_estimation.py:11-65,
 * and its T*J calls of utils.triangulate_points, utils.py:1277-1336, i.e.
 * cv.undistortPoints x2 + cv.triangulatePoints + cv.convertPointsFromHomogeneous).
 *
 * kpts_dev : [n_points][3][V] float32 — the reference kpts_2d layout (T,J,3,V)
 *            flattened over (T,J); rows are x, y, confidence.
 * cams_dev : [n_cams][MVP_CAM_DOUBLES] float64.
 * cam_idx_host / n_cam_idx : camera_indices (reference hard-codes [0,1],
 *            pose_estimation.py:319); 2 <= n_cam_idx <= 8, each < min(V, n_cams).
 * mode     : MVP_TRI_REFERENCE — per point, the two highest-confidence listed
 *              cameras in ASCENDING confidence order (np.argsort(conf)[-2:],
 *              pose_estimation.py:36), parameters keyed by selection position
 *              (pose_estimation.py:44-45), OpenCV 4.9 numerics;
 *            MVP_TRI_ALL_VIEWS — one 2·n_cam_idx x 4 DLT over all listed views
 *              (BASELINE config 3), parameters of camera cam_idx[i].
 * out_xyz_dev  : [n_points][3] float32 (cv.convertPointsFromHomogeneous result).
 * out_xyzw_dev : optional [n_points][4] float64 null vector (may be NULL).
 * ------------------------------------------------------------------------- */
#define MVP_TRI_REFERENCE 0
#define MVP_TRI_ALL_VIEWS 1
/* OR-ed into mode: solve every point with the exact JacobiSVDImpl_ restatement
 * (default: QR + inverse iteration, Jacobi where that has not converged or its f32
 * outputs are not certified equal to Jacobi's: the same float32 bits either way). */
#define MVP_TRI_EXACT_JACOBI 0x10
/* OR-ed into mode: throughput solver whose float32 outputs are certified bit-identical to the
 * exact path's (mixed f32/fp64 undistortion, normal-equation inverse iteration; a point whose
 * f32 roundings fall inside the error bound is re-solved on the exact path by a second launch).
 * The certification is EMPIRICAL, not a proof: the null vector's rounding-floor term uses
 * constants fitted on 1.4 M synthetic and random points (the exact Jacobi's own error measured
 * <= 0.025 eps*sqrt(trM/D2) where 0.2 is used, and D2/lambda3 <= 1.4; tri_common.h
 * null_vector_delta2).  tests/test_triangulate_gpu.py also asserts bit-identity on adversarial rigs (tiny
 * baselines, points near the epipoles, near-parallel rays).  Pass MVP_TRI_EXACT_JACOBI where a
 * proof is required.
 * Reference mode with 2 listed cameras; other cases run the default solver.  With
 * out_xyzw_dev != NULL every point takes the exact path (the float64 vectors are diagnostics). */
#define MVP_TRI_TOLERANCE 0x20

int mvp_triangulate(const float* kpts_dev, int64_t n_points, int V, const double* cams_dev,
                    int n_cams, const int* cam_idx_host, int n_cam_idx, int mode,
                    float* out_xyz_dev, double* out_xyzw_dev, void* stream);

/* Points the MVP_TRI_TOLERANCE solver re-solved on the exact path on this stream so far
 * (observability; synchronises the stream).  No reference counterpart. */
int mvp_triangulate_fallback_total(void* stream, unsigned long long* out_total_host);

/* ---------------------------------------------------------------------------
 * mvp_triangulate_robust — N-view triangulation with per-point outlier-view rejection, an
 * inlier mask and a reprojection-error read-out.  No reference counterpart (the reference
 * triangulates from two cameras only).
 *
 * kpts_dev, cams_dev, cam_idx_host / n_cam_idx as for mvp_triangulate in MVP_TRI_ALL_VIEWS mode:
 * view i reads column cam_idx[i] and the parameters of camera cam_idx[i]; fp64, OpenCV 4.9
 * undistortion restated, f32 undistorted points.
 *   Valid view: x and y finite, conf not NaN and conf >= min_conf, undistorted point finite.
 *   Reprojection error of view i against a homogeneous X: q = P_i·X in fp64; if q[2]·X[3] > 0
 *     (in front of the camera) hypot(q0/q2 - ux_i, q1/q2 - uy_i) in undistorted pixels against
 *     the f32 undistorted point, else +inf.
 *   Step A: fewer than 2 valid views -> xyz NaN, mask 0, errors NaN.  Otherwise the DLT over all
 *     valid views, its float32 xyz as mvp_triangulate writes it, and each valid view's error
 *     against (x, y, z, 1); if every one is <= inlier_px the point is done, mask = valid views.
 *   Step B (other points): for each pair (a, b), a < b, of valid views in lexicographic order,
 *     the fp64 null vector of the 4x4 two-view DLT is a hypothesis; its inliers are the valid
 *     views with error <= inlier_px against it.  Best = most inliers, then the larger sum of the
 *     inliers' confidences (f32, ascending view position), then the first pair.  Best count < 2:
 *     xyz NaN, mask 0, errors NaN.  Otherwise the final DLT over the best inlier set: mask = that
 *     set, and the errors of all valid views are those against the final float32 point (w = 1).
 *   Errors of invalid views are NaN.
 * The float32 xyz equals, bit for bit, OpenCV 4.9's triangulation (Jacobi SVD DLT +
 * convertPointsFromHomogeneous) over exactly the masked views in ascending position.
 *
 * inlier_px finite and > 0; min_conf not NaN.
 * out_xyz_dev  : [n_points][3] float32.
 * out_mask_dev : [n_points] uint8, bit i = view i (cam_idx[i]) used.
 * out_err_dev  : optional [n_points][n_cam_idx] float32 (may be NULL).
 * ------------------------------------------------------------------------- */
int mvp_triangulate_robust(const float* kpts_dev, int64_t n_points, int V, const double* cams_dev, int n_cams,
                           const int* cam_idx_host, int n_cam_idx, float inlier_px, float min_conf,
                           float* out_xyz_dev, uint8_t* out_mask_dev /* [n], bit i = view i used */,
                           float* out_err_dev /* [n][n_cam_idx], may be NULL */, void* stream);

/* ---------------------------------------------------------------------------
 * mvp_triangulate_peaks — mvp_triangulate_robust over up to MVP_MAX_PEAKS 2D candidates per view
 * (the modes of a heatmap, mvp_heatmap_peaks), choosing one candidate per inlier view.  No
 * reference counterpart.  With M = 1 it is mvp_triangulate_robust: xyz and mask bit for bit.
 *
 * peaks_dev : [n_points][M][3][V] float32, rows x, y, score; slot m of a point has the kpts
 * layout.  cams_dev, cam_idx_host / n_cam_idx, the undistortion and the reprojection error are
 * mvp_triangulate_robust's.
 *   Valid candidate (view i, slot m): x and y finite, score not NaN and >= min_conf, undistorted
 *     point finite.  Valid view: a view with at least one valid candidate.  Top candidate of a
 *     view: its valid candidate with the lowest slot.
 *   Step A: fewer than 2 valid views -> xyz NaN, mask 0, every sel -1, errors NaN.  Otherwise the
 *     DLT over the top candidates of all valid views, its float32 xyz, and each valid view's error
 *     (top candidate) against (x, y, z, 1); if every one is <= inlier_px the point is done,
 *     mask = the valid views, sel = their top slots.
 *   Step B (other points): hypotheses in lexicographic order of (a, b, ma, mb), a < b valid views,
 *     ma / mb valid candidates of a / b; each is the fp64 null vector of the 4x4 two-view DLT of
 *     that candidate pair.  Against a hypothesis every valid view (a and b like any other) chooses
 *     its valid candidate with the smallest error, ties to the lower slot, and is an inlier when
 *     that error is <= inlier_px.  Best = most inliers, then the larger sum of the inliers' chosen
 *     scores (f32, ascending view position), then the first hypothesis.  Best count < 2: the point
 *     fails as in step A.  Otherwise the final DLT over the inlier views with their chosen
 *     candidates: mask = that set, sel = those slots.
 * The float32 xyz equals, bit for bit, OpenCV 4.9's triangulation (Jacobi SVD DLT +
 * convertPointsFromHomogeneous) over exactly the masked views' selected candidates in ascending
 * position (mvp_triangulate_robust's contract and solver).
 *
 * 1 <= M <= MVP_MAX_PEAKS; inlier_px finite and > 0; min_conf not NaN.
 * out_xyz_dev  : [n_points][3] float32.
 * out_mask_dev : [n_points] uint8, bit i = view i (cam_idx[i]) used.
 * out_sel_dev  : [n_points][n_cam_idx] int8, the slot used by view i, -1 for a view not in the mask.
 * out_err_dev  : optional [n_points][n_cam_idx] float32 against the final float32 point (w = 1):
 *                a masked view's selected candidate; for a valid view outside the mask the
 *                smallest error over its valid candidates; NaN for invalid views and failed points.
 * out_kpts_dev : optional [n_points][3][V] float32, the kpts layout: column cam_idx[i] of a masked
 *                view holds its selected candidate, every other column slot 0 unchanged.
 * ------------------------------------------------------------------------- */
#define MVP_MAX_PEAKS 4

int mvp_triangulate_peaks(const float* peaks_dev, int64_t n_points, int M, int V, const double* cams_dev,
                          int n_cams, const int* cam_idx_host, int n_cam_idx, float inlier_px, float min_conf,
                          float* out_xyz_dev, uint8_t* out_mask_dev, int8_t* out_sel_dev,
                          float* out_err_dev /* may be NULL */, float* out_kpts_dev /* may be NULL */, void* stream);

/* ---------------------------------------------------------------------------
 * mvp_triangulate_refine — maximum-likelihood N-view triangulation from a seed, with the point's
 * 3D covariance.  No reference counterpart.  (The reference's SGD scores every camera against
 * camera 0's Gaussian, finding F5; here each camera is scored against its own.)
 *
 * kpts_dev, cams_dev, cam_idx_host / n_cam_idx as for mvp_triangulate_robust: view i reads column
 * cam_idx[i] and the parameters of camera cam_idx[i]; 2 <= n_cam_idx <= 8.  Everything is fp64.
 *   Used view: its bit in mask_dev[p] is set (or mask_dev is NULL); x and y finite; conf not NaN
 *     and conf >= min_conf; with MVP_REFINE_W_GAUSS also: its six Gaussian numbers are finite and
 *     not all zero (all zeros is the record of an empty heatmap), and
 *     S = [[vxx, vxy], [vxy, vyy]] + cov_floor·I is positive definite (S00 > 0 and det S > 0).
 *   Observation z_i and weight W_i of a used view:
 *     MVP_REFINE_W_UNIT   z = (x, y) of kpts,  W = I
 *     MVP_REFINE_W_CONF   z = (x, y) of kpts,  W = conf·I
 *     MVP_REFINE_W_GAUSS  z = (mx, my),        W = S⁻¹
 *     The Gaussian of point p = t·J + j in view i is gauss_dev[t][cam_idx[i]][j] =
 *     [mx, my, vxx, vxy, vxy, vyy] (the heatmaps_2d layout; the first vxy is the one read).
 *   Forward model pi_i(X): P = R·X + T, which requires P_z > 0; (x, y) = (P_x, P_y) / P_z;
 *     r2 = x² + y², radial = 1 + k1·r2 + k2·r2² + k3·r2³,
 *     xd = x·radial + 2·p1·x·y + p2·(r2 + 2x²), yd = y·radial + p1·(r2 + 2y²) + 2·p2·x·y;
 *     pixel = (K00·xd + K01·yd + K02, K11·yd + K12).  Observations are raw, distorted pixels:
 *     nothing is undistorted.
 *   Cost f(X) = ½ Σ r_iᵀ W_i r_i over the used views, r_i = pi_i(X) - z_i; +inf when any used view
 *     has P_z <= 0.
 *   Solver: Levenberg-Marquardt on the 3x3 normal equations with analytic Jacobians J_i = d pi_i /
 *     dX: H = Σ J_iᵀ W_i J_i, g = Σ J_iᵀ W_i r_i, lambda = 1e-3 at the start.  A trial solves
 *     (H + lambda·diag H)·delta = -g by Cholesky and is accepted when f(X + delta) is finite and
 *     <= f(X): then X <- X + delta and lambda <- max(lambda/10, 1e-12); otherwise lambda <-
 *     10·lambda.  The point has converged at the first trial whose proposed step satisfies
 *     |delta| <= tol·(|X| + tol), X being the point the step was proposed from, whether the trial
 *     is accepted or not (an accepted step is applied first).  At most max_iter trials.
 *   Failure: fewer than 2 used views; a seed that is not finite; f at the seed not finite; a
 *     Cholesky pivot of a trial's damped matrix that is not > 0.  A failed point returns the seed's
 *     bits as xyz, NaN cov and cost, status 0x80: a refined point is never less defined than its seed.
 *
 * xyz0_dev       : [n_points][3] float32 seed (any triangulator's output).
 * mask_dev       : optional [n_points] uint8, bit i = view i may be used (mvp_triangulate_robust's
 *                  out_mask); NULL = every listed view.
 * weights        : MVP_REFINE_W_*.  gauss_dev / J: [n_points/J][V][J][6] float64, required for
 *                  MVP_REFINE_W_GAUSS (J > 0 dividing n_points), ignored otherwise.
 * min_conf not NaN; cov_floor >= 0 (pixels², not NaN); 0 <= max_iter <= 63; tol finite, > 0.
 * out_xyz_dev    : [n_points][3] float32, the final X.
 * out_cov_dev    : optional [n_points][6] float32 (xx, xy, xz, yy, yz, zz): the inverse of the
 *                  undamped H at the final X, world units²; NaN when that H is not positive definite.
 * out_cost_dev   : optional [n_points] float32, f at the final X.
 * out_status_dev : optional [n_points] uint8: bits 0-5 the number of trials, 0x40 no trial met the
 *                  convergence test (max_iter = 0 included), 0x80 failed (then exactly 0x80).
 * With max_iter = 0 the call returns the seed, with cov and cost evaluated at the seed.
 * ------------------------------------------------------------------------- */
#define MVP_REFINE_W_UNIT 0
#define MVP_REFINE_W_CONF 1
#define MVP_REFINE_W_GAUSS 2

int mvp_triangulate_refine(const float* kpts_dev, int64_t n_points, int V, const double* cams_dev, int n_cams,
                           const int* cam_idx_host, int n_cam_idx, const float* xyz0_dev, const uint8_t* mask_dev,
                           int weights, const double* gauss_dev, int J, float min_conf, float cov_floor,
                           int max_iter, double tol, float* out_xyz_dev, float* out_cov_dev, float* out_cost_dev,
                           uint8_t* out_status_dev, void* stream);

/* ---------------------------------------------------------------------------
 * mvp_triangulate_points_f64 — replaces utils.triangulate_points (utils.py:1277-1336)
 * called with float64 keypoints, as the extrinsic branch does on its Gaussian samples
 * (pose_refinement.py:811): OpenCV keeps CV_64F through undistortPoints, triangulatePoints
 * and convertPointsFromHomogeneous, so nothing is rounded to f32.
 *
 * kpts_dev : [n_points][2 views][2] float64 (the reference's (n_pts, 2, 2) layout).
 * cams_dev : [2][MVP_CAM_DOUBLES] float64, camera 1 then camera 2; P (slots 26..37) as the
 *            caller computed it (the reference's np.dot in the parameters' own dtype).
 * out_xyz_dev  : [n_points][3] float64.  out_xyzw_dev: optional [n_points][4] float64.
 * Exact JacobiSVDImpl_ restatement for every point.
 * ------------------------------------------------------------------------- */
int mvp_triangulate_points_f64(const double* kpts_dev, int64_t n_points, const double* cams_dev,
                               double* out_xyz_dev, double* out_xyzw_dev, void* stream);

/* ---------------------------------------------------------------------------
 * 2D stage around the backbone (replaces, per camera frame, what
 * PoseEstimator.predict gets from mmpose at mmpose_pose_estimation.py:253-267).
 *
 * mvp_preprocess: TopdownAffine for each crop's bbox + PoseDataPreprocessor.
 *   frames_dev [n][H][W][3] uint8 (as the reference hands them to the model);
 *   minv_dev [n][6] float64 = the crop -> image map cv2.warpAffine uses
 *   internally (inverse of mmpose get_warp_matrix); mean3/std3 host f32;
 *   swap_rb = bgr_to_rgb.  out_dev [(1+with_flip)*n][out_h][out_w][4] bf16
 *   (RGB + zero channel); the flipped copies (flip test) follow the n originals.
 * mvp_heatmap_decode: flip-test average (flip_mode='heatmap', shift_heatmap)
 *   + MSRAHeatmap decode + restore to image pixels.  hm_dev/hm_flip_dev
 *   [N][K][H][W] f32 (hm_flip may be NULL: no flip test); flip_idx_host [K];
 *   center_scale_dev [N][4] f32 (cx, cy, sw, sh); outputs avg_dev (nullable)
 *   [N][K][H][W], kpts_dev [N][K][2] f32, scores_dev [N][K] f32, argmax_dev
 *   (nullable) [N][K] int32 flat index into H*W; kpts_tkv_dev (nullable)
 *   [N/V][K][3][V] f32 = the reference kpts_2d layout (crops ordered (t, v)).
 * mvp_heatmap_moments: revert_heatmap (warp of each map to the img_h x img_w
 *   image, float bilinear) fused with get_heatmap_means_cov
 *   (mmpose_pose_estimation.py:163-215): out_dev [N][K][6] float64
 *   (mx, my, vxx, vxy, vxy, vyy); minv_dev [N][6] = image -> heatmap map;
 *   separable != 0 asserts (host-checked with mvp_warp_is_separable) that every
 *   map's fixed-point source column depends on x only and source row on y only,
 *   enabling the column-resident fast path (per run of rows sharing a source
 *   row, columns whose taps are all clearly above / below thr are summed in
 *   closed form); separable == 2 runs that path walking every row of every
 *   column (diagnostics, tests).  separable_dev (nullable) [N] int: per-crop flags
 *   from mvp_bbox_geometry; crops flagged 0 take the general path, the others the
 *   `separable` mode.
 * ------------------------------------------------------------------------- */
int mvp_preprocess(const uint8_t* frames_dev, int n, int H, int W, const double* minv_dev, int out_h, int out_w,
                   const float* mean3_host, const float* std3_host, int swap_rb, int with_flip, uint16_t* out_dev,
                   void* stream);
int mvp_heatmap_decode(const float* hm_dev, const float* hm_flip_dev, int N, int K, int H, int W,
                       const int* flip_idx_host, int shift, const float* center_scale_dev, int input_w, int input_h,
                       float* avg_dev, float* kpts_dev, float* scores_dev, int32_t* argmax_dev, float* kpts_tkv_dev,
                       int V, void* stream);
/* mvp_heatmap_peaks: up to max_peaks local maxima of every map, each decoded as
 *   mvp_heatmap_decode decodes its argmax (no reference counterpart; the candidates of
 *   mvp_triangulate_peaks).  hm_dev [N][K][H][W] f32: the maps decoding looks at, i.e.
 *   mvp_heatmap_decode's avg_dev, crops ordered (t, v); center_scale_dev, input_w, input_h as there.
 *   Cell i = y*W + x with value v is a peak when v is no NaN, v > thr, and for every other
 *   in-bounds cell n (value u) of the (2·radius+1)² window around it: u is NaN, or v > u, or
 *   v == u and i < n.  Peaks are ordered by descending v, ties by ascending i (the decode's
 *   argmax order: on a NaN-free map whose maximum exceeds thr the first peak is the argmax cell);
 *   peak r > 0 is kept only if v_r >= min_rel * v_0 (f32 product); the first
 *   min(count, max_peaks) are written.  A written peak is decoded with the decode's arithmetic
 *   (val <= 0 -> -1, +-0.25 sign step inside 1 < px < W-1, 1 < py < H-1, f32 scale factor, fp64
 *   restore rounded to f32); its score is v.
 *   peaks_dev [N/V][K][max_peaks][3][V] f32, rows x, y, score in image pixels: peaks[:, :, m] has
 *   the kpts_tkv layout; unfilled slots hold x = y = NaN, score 0.  counts_dev (nullable)
 *   [N/V][K][V] int32, the peaks written.
 *   1 <= max_peaks <= MVP_MAX_PEAKS, 1 <= radius <= 3, thr not NaN, 0 <= min_rel <= 1, V >= 1
 *   dividing N, H*W <= 65536, K <= 32. */
int mvp_heatmap_peaks(const float* hm_dev, int N, int K, int H, int W, const float* center_scale_dev, int input_w,
                      int input_h, int max_peaks, int radius, float thr, float min_rel, int V, float* peaks_dev,
                      int32_t* counts_dev, void* stream);
int mvp_warp_is_separable(const double* minv_host, int img_h, int img_w, int* separable_out);
/* revert_heatmap only (not on the hot path, which fuses it into the moments): each crop's
 * K maps [N][K][h][w] f32 warped to the image, out [N][K][img_h][img_w] f32 — cv2.warpAffine
 * INTER_LINEAR / BORDER_CONSTANT with minv = the image -> heatmap map (as for moments). */
int mvp_heatmap_revert(const float* hm_dev, int N, int K, int h, int w, const double* minv_dev, int img_h,
                       int img_w, float* out_dev, void* stream);
int mvp_heatmap_moments(const float* hm_dev, int N, int K, int h, int w, const double* minv_dev, int img_h,
                        int img_w, float thr, int separable, const int* separable_dev, double* out_dev,
                        void* stream);
/* mvp_bbox_geometry: the reference's detector -> inference_topdown hand-off and TopdownAffine
 *   geometry on the device (replaces mmpose_pose_estimation.py:242-253 + mmpose bbox_xyxy2cs /
 *   _fix_aspect_ratio / get_warp_matrix -> cv2.getAffineTransform (cv::solve LU) and
 *   warpAffine's inversion).  Row i of boxes_dev ([n][stride] f32: x1, y1, x2, y2, ...) is the
 *   person box when its four coordinates are finite and (score_col < 0 or
 *   row[score_col] > bbox_thr), else the whole frame_w x frame_h image.  Writes crop_minv_dev
 *   [n][6] f64 (crop -> image, for mvp_preprocess), revert_minv_dev [n][6] f64 (image ->
 *   heatmap, for mvp_heatmap_moments / revert), center_scale_dev [n][4] f32 (for
 *   mvp_heatmap_decode) and separable_dev [n] int (mvp_warp_is_separable of the revert map).
 *   Fed directly with mvp_det_forward's best_dev (stride 6, score_col 4). */
int mvp_bbox_geometry(const float* boxes_dev, int stride, int n, int score_col, float bbox_thr, int frame_h,
                      int frame_w, double* crop_minv_dev, double* revert_minv_dev, float* center_scale_dev,
                      int* separable_dev, void* stream);

/* ---------------------------------------------------------------------------
 * Backbone graph runtime (replaces the HRNet-W32 forward inside mmpose's
 * inference_topdown, called at mmpose_pose_estimation.py:253 once per camera
 * frame, batch 1, on the CPU).  A static graph of convolutions on bf16 NHWC
 * activations, BN folded into the weights, executed batch-wide on one stream.
 * The graph (topology + packed weights) is built by the host
 * (mvpose/hrnet.py); the runtime validates it, plans one activation arena by
 * tensor liveness (buffers reused across the ~330 ops), and launches the HIP
 * kernels.
 *
 * Tensors: per-crop shape (h, w, c); dtype MVP_DT_BF16_NHWC or
 * MVP_DT_F32_NCHW.  The batch dimension is given at forward time.
 * Ops:
 *   MVP_OP_STEM : 3x3/s2 conv of a 4-channel (RGB+0) bf16 input to 64 ch, BN+ReLU
 *                 folded; w_off/b_off index the f32 blob ([64][3][3][4], [64]).
 *   MVP_OP_CONV : y = act(conv(in[0]) + bias [+ in[1]]), ks 1|3, stride 1|2;
 *                 w_off indexes the bf16 blob ([cout_pad][ks][ks][cin]),
 *                 b_off the f32 blob ([cout_pad]); cout_pad = cout <= 32 ? 32 :
 *                 round_up(cout, 64).  An F32_NCHW output tensor makes it the
 *                 heatmap head.
 *   MVP_OP_FUSE : out = act(sum_k nearest_upsample(in[k], up[k])), n_in <= 4
 *                 (HRModule multi-scale fuse).
 * Segments: every op carries a segment id; the ops of a segment are
 * contiguous.  seg_micro_batch_host[g] > 0 runs segment g in micro-batches of
 * that many crops (0 = whole batch at once): tensors produced and consumed only
 * inside a micro-batched segment are allocated for one micro-batch, so a chain
 * of layers keeps its intermediates in the 256 MiB Infinity Cache instead of
 * HBM.
 * ------------------------------------------------------------------------- */
#define MVP_DT_BF16_NHWC 0
#define MVP_DT_F32_NCHW 1

#define MVP_OP_STEM 0
#define MVP_OP_CONV 1
#define MVP_OP_FUSE 2

typedef struct mvp_tensor_desc {
    int h, w, c, dtype;
} mvp_tensor_desc;

typedef struct mvp_op_desc {
    int kind;
    int out;
    int n_in;
    int in[4];
    int up[4];
    int cin, cout, ks, stride, relu;
    int segment;
    int64_t w_off;
    int64_t b_off;
} mvp_op_desc;

int mvp_graph_create(const mvp_tensor_desc* tensors_host, int n_tensors, const mvp_op_desc* ops_host, int n_ops,
                     const int* seg_micro_batch_host, int n_segments, int input_tensor, int output_tensor,
                     const uint16_t* w_bf16_dev, int64_t w_elems, const float* f32_dev, int64_t f32_elems,
                     int max_batch, void** handle_out);
/* input_dev: [batch][h][w][c] of the input tensor; output_dev: the output tensor. */
int mvp_graph_forward(void* handle, const void* input_dev, int batch, void* output_dev, void* stream);
int mvp_graph_arena_bytes(void* handle, int64_t* bytes_out);
/* The weight blobs passed to mvp_graph_create were rewritten in place (e.g. an RCCL
 * broadcast from rank 0 after every rank built its graph): re-derive every weight
 * the graph copied out of them at create time (cat-fused 1x1 weights / biases, the
 * sibling-fused 3x3/s2 weights, and the slot-order weight images of the 128/256-channel
 * branch planes, the streamed-weight 3x3/s2 convs and transition1).
 * Blocking (device-synchronising). */
int mvp_graph_refresh_weights(void* handle);
int mvp_graph_destroy(void* handle);
/* Diagnostics (no reference counterpart): the kernel launches one mvp_graph_forward of `batch`
 * crops issues, in order, as records of 4 int64 {launching op, route, crops, MACs of every op
 * the launch covers}; route 1 fused BasicBlock, 2 transition twin, 3 s2 siblings, 4 head +
 * fuse, 5 Bottleneck, 6 stem pair, 7 stem, 8 conv, 9 1x1 pair, 10 fuse sum.  Every op is covered
 * by exactly one launch (mvp_graph_create checks it).  *covered_macs_out (optional) = the sum.
 * tools/fwd_breakdown.py pairs the records with a kernel trace. */
int mvp_graph_plan(void* handle, int batch, int64_t* rec_out, int max_records, int* n_records,
                   int64_t* covered_macs_out);
/* Diagnostics: the kernel family each of those launches runs, one id per record of
 * mvp_graph_plan in the same order.  The graph chooses a launch's kernel when it is created,
 * from the op's shape, its route and the MVPOSE_* switches as the environment had them then;
 * where the choice depends on the batch (the crop-streaming kernels, from one crop per CU) a
 * smaller last micro-batch may show another kernel than the full ones.  mvp_graph_kernel_name:
 * the kernel function's base name as a kernel trace shows it ("" for an unknown id). */
int mvp_graph_kernels(void* handle, int batch, int* kernels_out, int max_records, int* n_records);
const char* mvp_graph_kernel_name(int kernel);

/* ---------------------------------------------------------------------------
 * Person detector: RTMDet-m (the reference's `detectors.coco_base`,
 * examples/model_paths.yaml:2-4) as run by PoseEstimator.predict through mmdet's
 * inference_detector (mmpose_pose_estimation.py:98-99, :234-241), followed by the
 * reference's hand-off rule (:242-250): the first detection with label 0 and score >
 * bbox_thr.  After mmdet's NMS the first detection is the highest-scoring prior that
 * survives score_thr and the min-size filter, so the hot path is: letterbox ->
 * CSPNeXt-m / CSPNeXtPAFPN / RTMDetSepBNHead -> per-prior score + box -> per-frame
 * argmax.  A per-frame NMS kernel gives mmdet's full detection list.
 *
 * mvp_det_letterbox: frames_dev [n][h][w][3] uint8 -> out_dev [n][size][size][4] bf16:
 *   mmdet Resize(scale=(size, size), keep_ratio=True) with cv2 INTER_LINEAR semantics
 *   (exact 2x downscale = INTER_AREA's fast path), Pad(114) bottom / right, then
 *   (x - mean[c]) / std[c] in f32 (channel 3 = 0).  new_h / new_w are the resized extent
 *   (mmcv rescale_size: int(h * s + 0.5), s = min(size / long, size / short)).
 *
 * Graph ops (views = channel slices of NHWC bf16 tensors: concat is a shared buffer):
 *   MVP_DET_STEM : 3x3/s2 conv of the 4-channel letterboxed input to 32 channels,
 *                  f32 weights [32][3][3][4] + bias [32], act.
 *   MVP_DET_CONV : y = act(conv(x) + bias [+ res]), ks 1|3, stride 1|2, bf16 weights
 *                  [cout_pad][ks][ks][cin] (cout_pad as mvp_graph), f32 bias.  aux = the live
 *                  couts L (0 = all): the caller guarantees zero weights and bias for couts
 *                  >= L, whose outputs are then stored as 0 without being computed.
 *   MVP_DET_DW   : 5x5 depthwise conv + bias + act, f32 weights [c/8][25][8], bias [c].
 *   MVP_DET_CA   : channel attention in place on `in`: x *= hardsigmoid(W·mean(x) + b),
 *                  f32 W^T [c][c] (w_off) and b [c].
 *   MVP_DET_SPP  : `in` = slice 0 (c channels) of a 4c buffer; writes max-pools 5/9/13
 *                  (stride 1, -inf padding) into slices 1..3.
 *   MVP_DET_UP2  : out = nearest 2x upsample of in.
 *   MVP_DET_HEAD : one FPN level's predictions from `in` = [cls feat | reg feat]
 *                  (c = 2 * 192): f32 weights [5][192] (cls, reg l/t/r/b) + bias [5];
 *                  writes cand rows [prior][6] = {sigmoid score, x1, y1, x2, y2, logit}
 *                  at prior offset `aux`, box = prior (x, y) * stride -+ exp(reg) * stride,
 *                  clipped to [0, size] (mmdet distance2bbox on img_shape).
 *   MVP_DET_DWPW : a CSPNeXtBlock's conv2 (DepthwiseSeparableConvModule) in one launch:
 *                  t = act(dw5x5(in) + b_dw) rounded to bf16 (never stored), then
 *                  out = act(t . W_pw + b_pw) [+ res]; in.c = C in {64, 96},
 *                  cout_pad(out.c) == C.  w_off: dw f32 weights [C/8][25][8]; b_off: f32
 *                  [b_dw (C) | b_pw (C)]; aux: pw bf16 weights [C][1][1][C].  Bit-identical to
 *                  MVP_DET_DW followed by a 1x1 MVP_DET_CONV.
 * act: 0 none, 1 ReLU (after a residual add), 2 SiLU (before it: CSPNeXtBlock's
 * conv2(conv1(x)) + x).
 * ------------------------------------------------------------------------- */
#define MVP_DET_STEM 0
#define MVP_DET_CONV 1
#define MVP_DET_DW 2
#define MVP_DET_CA 3
#define MVP_DET_SPP 4
#define MVP_DET_UP2 5
#define MVP_DET_HEAD 6
#define MVP_DET_DWPW 7

typedef struct mvp_det_view {
    int t;    /* tensor id, -1 = none */
    int coff; /* first channel of the slice */
    int c;    /* channels of the slice */
} mvp_det_view;

typedef struct mvp_det_op {
    int kind;
    mvp_det_view in, out, res;
    int ks, stride, act;
    int64_t w_off, b_off;
    int64_t aux;
} mvp_det_op;

int mvp_det_letterbox(const uint8_t* frames_dev, int n, int h, int w, int size, const float* mean3_host,
                      const float* std3_host, void* out_dev, void* stream);
/* tensors_host: (h, w, c, unused) per image; tensor `input_tensor` is the letterboxed image
 * (c = 4).  n_priors = total rows the HEAD ops write. */
int mvp_det_create(const mvp_tensor_desc* tensors_host, int n_tensors, const mvp_det_op* ops_host, int n_ops,
                   int input_tensor, int size, int n_priors, const uint16_t* w_bf16_dev, int64_t w_elems,
                   const float* f32_dev, int64_t f32_elems, int max_batch, void** handle_out);
/* frames_dev [n][h][w][3] uint8 -> cand_dev [n][n_priors][6] f32 and best_dev [n][6] f32 =
 * {x1, y1, x2, y2, score, prior} of the highest-scoring prior with score > score_thr and a
 * positive width / height after rescaling to the frame (x / (new_w / w), y / (new_h / h));
 * ties -> lowest prior index; score = -1 when none.  letterboxed_dev: NULL (internal) or a
 * caller buffer [n][size][size][4] bf16 that receives the letterboxed input. */
int mvp_det_forward(void* handle, const uint8_t* frames_dev, int n, int h, int w, float score_thr, float* cand_dev,
                    float* best_dev, void* letterboxed_dev, void* stream);
/* mmdet post-processing on cand_dev from mvp_det_forward: per frame, priors with score >
 * score_thr, the nms_pre best of each level (level l = prior rows [level_off[l],
 * level_off[l + 1])), boxes rescaled to the frame, min-size filter, greedy NMS at iou_thr
 * in descending score order (ties: lower prior first), the first max_det kept ->
 * dets_dev [n][max_det][5] {x1, y1, x2, y2, score} (score-descending), counts_dev [n]. */
int mvp_det_nms(const float* cand_dev, int n, int n_priors, const int* level_off_host, int n_levels, int nms_pre,
                float score_thr, float iou_thr, int max_det, float fx, float fy, float* dets_dev, int* counts_dev,
                void* stream);
int mvp_det_arena_bytes(void* handle, int64_t* bytes_out);
/* Layer-by-layer access for parity tests: mvp_det_run_ops runs the letterbox (when
 * op_begin == 0) and ops [op_begin, op_end) on the handle's arena; mvp_det_tensor_copy
 * copies the first n images of arena tensor t to (to_arena = 0) or from (1) buf_dev. */
int mvp_det_run_ops(void* handle, const uint8_t* frames_dev, int n, int h, int w, int op_begin, int op_end,
                    float* cand_dev, void* stream);
int mvp_det_tensor_copy(void* handle, int t, int n, void* buf_dev, int to_arena, void* stream);
/* Producer passes folded into their consumer 1x1 conv at create time (the neck's nearest-2x
 * upsamples; the channel-attention scale pass): folded_out[k] = 1 when op k's pass runs inside
 * the next conv reading its tensor (a DET_UP2 then launches nothing and leaves its output slice
 * unwritten; a DET_CA computes its scales and leaves its tensor unscaled); folded_out[0] = 2
 * when the letterbox runs inside the stem (op 0 stages its rows from the raw frames; the input
 * tensor stays unwritten unless mvp_det_forward is given letterboxed_dev); else 0.  Results are
 * bit-identical either way.  The switch that turns folding off is one of the detector's
 * MVPOSE_DET_* switches, all documented in one place: DetSwitches in csrc/det_select.h. */
int mvp_det_folded_ops(void* handle, int* folded_out, int n_ops);
/* Diagnostics: the kernel variant of every launch of one mvp_det_forward (letterboxed_dev NULL),
 * in launch order: the letterbox when it is not folded into the stem, each op's kernel (a DET_CA
 * launches its pool and fc passes and, unless folded, its scale pass; a folded DET_UP2 nothing),
 * then the per-frame selection.  mvp_det_create chooses every op's variant from its shape, the
 * folds, the device's CU count and the MVPOSE_DET_* switches as the environment had them then;
 * no later change of the environment reaches a live handle.  *n_records = the launches;
 * kernels_out receives them when max_records (0: count only) has room.  mvp_det_kernel_name: the
 * variant's name ("" for an unknown id; the variants are DetKernel in csrc/det_select.h). */
int mvp_det_kernels(void* handle, int* kernels_out, int max_records, int* n_records);
const char* mvp_det_kernel_name(int kernel);
int mvp_det_destroy(void* handle);

/* ---------------------------------------------------------------------------
 * Reprojection-error trajectory refinement (Optimized_3d_Pose_Estimation,
 * reference pose_refinement.py:579-668 + sgd_optimize :894-1096, trajectory-only
 * path the CLI runs at :1210-1214).
 *
 * One workgroup refines one trajectory: the whole optimisation (every
 * iteration, every overlapping window, forward costs, analytic gradient,
 * clip_grad_norm_, Adam, running-mean early stop, best-trajectory snapshot)
 * runs inside ONE launch.  M independent trajectories run as M workgroups.
 *
 * Camera record (MVP_SGD_CAM_FLOATS f32): [K 9 | R 9 (matrix) | T 3 | dist 5].
 * ------------------------------------------------------------------------- */
#define MVP_SGD_CAM_FLOATS 26
#define MVP_SGD_N_COSTS 4 /* total, likelihood, smoothness, body_length */

typedef struct mvp_sgd_params {
    /* Python floats in the reference: kept in double so the f32 casts match torch's. */
    double lr, beta1, beta2, adam_eps;        /* torch.optim.Adam (eps 1e-8) */
    double lambda_smooth, lambda_body_length; /* a cost is skipped when its lambda <= 0 (:978-983) */
    double tolerance;                         /* running-mean improvement threshold (:1073) */
    double max_grad_norm;                     /* clip_grad_norm_ max_norm (1.0 at :1045) */
    int patience, max_iter;                  /* loop runs while no_improve < patience && it <= max_iter */
    int batch_size;                          /* window length; windows start every batch_size/2 (:786-796) */
    int ignore_distortions;
    int own_camera_gaussians;                /* 0 = reference: all cameras vs camera-0 Gaussians (:663, :885) */
} mvp_sgd_params;

/* Float workspace needed by mvp_sgd_refine for M trajectories of T x J points seen by V cameras. */
int mvp_sgd_workspace_floats(int M, int T, int V, int J, int64_t* out);

/* gauss [M][T][V][J][6] f32 (mx,my,cxx,cxy,cyx,cyy), traj0 [M][T][J][3] f32 (T already sliced by
 * time_interval; windows cover the first floor(T/batch_size)*batch_size rows), cams [V][26] f32, seg [n_seg][2] int
 * joint pairs (a -> b, length |X_b - X_a|) with seg_len [n_seg] f32 in the body-length YAML order.
 * Outputs: final [M][T][J][3], best [M][T][J][3] (NaN if never improved),
 * batch_costs [M][max_iter+1][n_windows][4], iter_means [M][max_iter+1][4] (the reference's
 * running means), iters [M] (iterations executed).  All pointers are device pointers except p. */
int mvp_sgd_refine(const float* gauss, const float* traj0, const float* cams, int M, int T, int V, int J,
                   const int* seg, const float* seg_len, int n_seg, const mvp_sgd_params* p, float* workspace,
                   float* final_traj, float* best_traj, float* batch_costs, float* iter_means, int* iters,
                   void* stream);

/* Joint trajectory + extrinsic refinement: sgd_optimize(extrinsic_optimization_IDs=ids,
 * optimize_trajectory=True) (pose_refinement.py:894-1096 with :931-954 — the listed cameras'
 * R (3x3 matrix, the reference's default learnable form) and T are leaf tensors in the same
 * Adam optimizer as the trajectory, ahead of it, and in the same clip_grad_norm_).  As
 * mvp_sgd_refine, plus learn_cam_host [n_learn] (host) camera slots (0 <= slot < V, distinct,
 * n_learn <= 2) whose R, T receive the likelihood gradient (dcost/dR_ij = dcost/dP_i X_j,
 * dcost/dT_i = dcost/dP_i, P = R X + T) and their own Adam state.  cams_final / cams_best
 * [M][n_learn][12] f32 (R row-major | T; best = NaN if never improved) are device pointers;
 * the cams records themselves are not modified. */
int mvp_sgd_refine_cams(const float* gauss, const float* traj0, const float* cams, int M, int T, int V, int J,
                        const int* seg, const float* seg_len, int n_seg, const mvp_sgd_params* p, float* workspace,
                        float* final_traj, float* best_traj, float* batch_costs, float* iter_means, int* iters,
                        const int* learn_cam_host, int n_learn, float* cams_final, float* cams_best, void* stream);

/* project_points_torch (pose_refinement.py:94-179): pts [n][3] f32 -> uv [n][2] f32 for one camera
 * record (R as a 3x3 matrix). */
/* Extrinsic-from-samples refinement (sgd_optimize(extrinsic_optimization_IDs=[id],
 * optimize_trajectory=False), reference pose_refinement.py:684-706, :800-831, :915-943):
 * one pass over the triangulated Gaussian samples samples_dev [n_points][3] f32, ordered
 * (t, joint, sample) with n_samples per (t, joint); targets_dev [n_points / n_samples][6] f32
 * = (mean x, mean y, Σ⁻¹ 00, 01, 10, 11) per (t, joint); cam_dev = the learnable camera's
 * MVP_SGD_CAM_FLOATS record (R as a matrix).  Writes per-block fp64 partial sums
 * partial_dev [n_blocks][14] = [Σ 0.5 dᵀΣ⁻¹d over finite terms, finite count, Σ dq/dR (9,
 * row-major), Σ dq/dT (3)]; the caller reduces them (cost = sum / count, gradients / count). */
int mvp_extrinsic_sample_grad(const float* samples_dev, const float* targets_dev, int n_samples, int64_t n_points,
                              const float* cam_dev, int ignore_distortions, int n_blocks, double* partial_dev,
                              void* stream);
/* One Adam step of that branch on the device (pose_refinement.py:1039-1050, learnable R as a
 * 3x3 matrix and T): reduces partial_dev [n_blocks][14] of mvp_extrinsic_sample_grad, casts
 * cost and gradient to f32 like the host path, clip_grad_norm_([R, T], max_norm), torch
 * single-tensor Adam on R and T with state_dev [m (12) | v (12) | step (int32)] (zero it before
 * the first step), and updates R (cam_dev[9..18)) and T (cam_dev[18..21)) in place, so the next
 * mvp_extrinsic_sample_grad sees the new camera.  The step's cost goes to cost_hist_dev[step-1]
 * and the new R, T (12 floats) to param_hist_dev[step-1][12]: the host reads the history every
 * few iterations for the early-stop bookkeeping instead of once per step. */
int mvp_extrinsic_adam_step(const double* partial_dev, int n_blocks, float* cam_dev, float* state_dev, double lr,
                            double beta1, double beta2, double adam_eps, double max_norm, float* cost_hist_dev,
                            float* param_hist_dev, void* stream);
int mvp_project_points(const float* pts, int64_t n, const float* cam, int ignore_distortions, float* uv,
                       void* stream);

/* ---------------------------------------------------------------------------
 * linear_interpolation (pose_refinement.py:15-84; always run by the refinement
 * CLI, :1170-1172): outlier-filtered local linear fit per (t, point, dim).
 * pts_dev/out_dev [T][P][D] f32; k <= 30; see csrc/interp.hip for the rules.
 * ------------------------------------------------------------------------- */
int mvp_linear_interpolation(const float* pts_dev, int T, int P, int D, int k, float k_std, float median_std,
                             int use_rolling_average, int filter_distance_from_median, float* out_dev,
                             void* stream);

/* ---------------------------------------------------------------------------
 * Covariance-weighted trajectory smoothing with gap filling (no reference counterpart; the
 * smoothness prior is the reference's second-difference cost, pose_refinement.py:836-845, the
 * likelihood is mvp_triangulate_refine's covariance).
 *
 * Chains are independent.  Chain p has unknowns X_t in R³, t = 0..T-1.  Frame (t, p) is
 * OBSERVED when all of these hold:
 *   - its three input coordinates are finite;
 *   - valid[t][p] != 0, where valid is given;
 *   - where cov is given: its six numbers (xx, xy, xz, yy, yz, zz) are finite and
 *     S = cov + cov_floor·I is positive definite (all three Cholesky pivots > 0).
 * An observed frame has W_t = S⁻¹ (W_t = I / sigma0² without cov); an unobserved frame has
 * W_t = 0 and its input coordinates are never used.  The output minimises
 *
 *   E(X) = ½ Σ_t (X_t − z_t)ᵀ W_t (X_t − z_t) + ½ λ Σ_{t=2}^{T−1} |X_t − 2 X_{t−1} + X_{t−2}|²
 *
 * i.e. solves (blockdiag(W) + λ·(D₂ᵀD₂ ⊗ I₃)) X = blockdiag(W) z, D₂ the (T−2)×T second-
 * difference matrix: symmetric, block-pentadiagonal in 3x3 blocks, positive definite whenever the
 * chain has >= 2 observed frames.  Consequences: gaps are filled by the cubic-spline-like
 * interpolant; before the first and after the last observed frame the track continues as a
 * straight line; T = 2 with both frames observed returns the inputs; data exactly affine in t are
 * returned unchanged for every λ.  λ = 1/σ_a², σ_a the standard deviation of a joint's second
 * difference per frame.
 *
 * Everything is fp64 on the device from the float32 inputs; FMA contraction is allowed, so the
 * results carry no bit-exactness contract (as for mvp_triangulate_refine).
 *
 * Failure: a chain fails when it has fewer than 2 observed frames or when any pivot of the
 * factorisation is not > 0.  A failed chain returns its input bits as out_xyz (NaNs included),
 * NaN residuals and status 0x80: a smoothed chain is never less defined than its input.
 *
 * The solve is parallel in time by the partition method: chunks of `chunk` interior frames with
 * 2-frame separators between them, one lane per (chain, chunk), then one reduced block-
 * tridiagonal system per chain on the separators (csrc/smooth.hip).  chunk = 0 picks the length
 * automatically; otherwise 4 <= chunk <= 4096.  The result does not depend on chunk beyond fp64
 * rounding.
 *
 * mvp_trajectory_smooth_plan : what a call with (T, P, chunk) will use: the chunk length, the
 *   number of chunks per chain and the workspace size in bytes (any of the three may be NULL).
 * mvp_trajectory_smooth : xyz_dev [T][P][3] f32; cov_dev [T][P][6] f32 or NULL; valid_dev [T][P]
 *   uint8 or NULL; workspace_dev >= the plan's bytes, owned by the caller (its contents are
 *   scratch).  out_xyz_dev [T][P][3] f32 (must not be xyz_dev); out_resid_dev [T][P] f32 or NULL =
 *   (X_t − z_t)ᵀ W_t (X_t − z_t), the squared Mahalanobis distance of the fp64 solution before it
 *   is rounded, NaN for unobserved frames and failed chains; out_observed_dev [T][P] uint8 (1/0)
 *   or NULL; out_status_dev [P] uint8 (0 or 0x80) or NULL.  Requires T >= 1, P >= 1,
 *   lambda_smooth and sigma0 finite and > 0, cov_floor >= 0.  Stream-ordered: no host
 *   synchronisation and no allocation inside the call.
 * ------------------------------------------------------------------------- */
int mvp_trajectory_smooth_plan(int T, int P, int chunk, int* chunk_used, int* n_chunks, int64_t* workspace_bytes);
int mvp_trajectory_smooth(const float* xyz_dev, const float* cov_dev, const uint8_t* valid_dev, int T, int P,
                          double lambda_smooth, float sigma0, float cov_floor, int chunk, void* workspace_dev,
                          int64_t workspace_bytes, float* out_xyz_dev, float* out_resid_dev,
                          uint8_t* out_observed_dev, uint8_t* out_status_dev, void* stream);

/* ---------------------------------------------------------------------------
 * Posterior covariance of the smoothed trajectory (no reference counterpart).
 *
 * With A = blockdiag(W) + λ·(D₂ᵀD₂ ⊗ I₃), exactly mvp_trajectory_smooth's matrix (the same observed
 * rule, W_t, sigma0 and cov_floor), the smoothed X is the mean of a Gaussian with covariance
 * Σ = A⁻¹: the exact posterior of that model.  The call returns its 3x3 diagonal blocks Σ_{t,t} and
 * its lag-1 blocks Σ_{t,t+1}, in world units², for EVERY frame: an unobserved frame has a
 * covariance too, held by the prior and its observed neighbours, and it grows towards the middle of
 * a gap.  Σ does not depend on the coordinates beyond whether they are finite.
 *
 * The factorisation is mvp_trajectory_smooth's (partition method, same elimination order); the
 * blocks of Σ come from the Takahashi recursion run back over its factors, every symmetric block
 * held as a packed triangle (csrc/smooth_solver.h).  fp64, FMA contraction
 * allowed; the result does not depend on chunk beyond fp64 rounding.
 *
 * Failure: mvp_trajectory_smooth's rules (fewer than 2 observed frames, or a pivot not > 0).  A
 * failed chain gets NaN in all of out_cov and out_cross and status 0x80; other chains status 0.
 *
 * mvp_trajectory_smooth_cov_plan : as mvp_trajectory_smooth_plan, for this call's (larger)
 *   workspace.
 * mvp_trajectory_smooth_cov : inputs as mvp_trajectory_smooth.  out_cov_dev [T][P][6] f32, required:
 *   (xx, xy, xz, yy, yz, zz) of Σ_{t,t}; out_cross_dev [T][P][9] f32 or NULL: Σ_{t,t+1} row-major,
 *   row = coordinate of X_t, column = coordinate of X_{t+1}, NaN at t = T−1; out_status_dev [P]
 *   uint8 or NULL.  Requires what mvp_trajectory_smooth requires; argument errors return
 *   MVP_ERR_ARG before any device work.  Stream-ordered: no host synchronisation and no allocation.
 * Time, one MI355X, T = 100 000, P = 17, chunk 0: 3.65 ms against mvp_trajectory_smooth's 2.46 ms on
 * the same inputs, 1.49x.
 * Out of scope: blocks further than lag 1; uncertainty of λ itself.
 * ------------------------------------------------------------------------- */
int mvp_trajectory_smooth_cov_plan(int T, int P, int chunk, int* chunk_used, int* n_chunks, int64_t* workspace_bytes);
int mvp_trajectory_smooth_cov(const float* xyz_dev, const float* cov_dev, const uint8_t* valid_dev, int T, int P,
                              double lambda_smooth, float sigma0, float cov_floor, int chunk, void* workspace_dev,
                              int64_t workspace_bytes, float* out_cov_dev, float* out_cross_dev,
                              uint8_t* out_status_dev, void* stream);

/* ---------------------------------------------------------------------------
 * Epipolar lag-cost scan: the data term of pose-based frame synchronisation (no reference
 * counterpart; the reference synchronises by hand, synchronize_videos.py).  For a calibrated pair
 * of cameras, keypoints of the same joint satisfy the epipolar constraint only when their frames
 * show the same instant; the scan scores that constraint for every pair of listed views and every
 * frame lag.
 *
 * kpts_dev [T][J][3][V] float32 (the kpts_2d layout; rows x, y, confidence), cams_dev,
 * cam_idx_host / n_cam_idx = nv as for mvp_triangulate_robust: view i reads column cam_idx[i] and
 * the parameters of camera cam_idx[i]; 2 <= nv <= 8.
 *   Pairs: (a, b), a < b positions in cam_idx, in lexicographic order: NP = nv·(nv−1)/2, pair 0 =
 *     (0, 1), pair 1 = (0, 2), ...
 *   Usable keypoint: x and y finite, conf not NaN and conf >= min_conf (the rule of
 *     mvp_triangulate_robust).  Its ideal pixel (u, v) is the float32 undistorted pixel the
 *     triangulators use (OpenCV 4.9 undistortPoints restated: 5 iterations in fp64, P = K,
 *     rounded to float32); x = (u, v, 1) in fp64.
 *   Fundamental matrix, fp64, from the records of cameras cam_idx[a], cam_idx[b]:
 *     F_ab = K_b⁻ᵀ [t]ₓ R K_a⁻¹ with R = R_b R_aᵀ, t = T_b − R T_a ([t]ₓ the cross-product
 *     matrix), so that x_bᵀ F_ab x_a = 0 for noise-free matches.  The distance below does not
 *     depend on the scale of F.
 *   Cost: for every lag l in [−L, L], L = max_lag, every frame t with 0 <= t < T and
 *     0 <= t + l < T and every joint j whose keypoint is usable in view a at frame t and in view b
 *     at frame t + l, the squared Sampson distance of x_a = x(a, t, j) and x_b = x(b, t + l, j):
 *       d² = (x_bᵀ F x_a)² / ((F x_a)₀² + (F x_a)₁² + (Fᵀ x_b)₀² + (Fᵀ x_b)₁²)
 *     A term whose denominator is 0 or whose d² is not finite is skipped.
 *       sum[p][l + L] = Σ min(d², trunc_px²)   (float64)
 *       cnt[p][l + L] = number of terms         (int64)
 *     The truncated quadratic is continuous in d², so rounding cannot move a term across the
 *     threshold by more than its own rounding error.
 * Arithmetic is fp64 (x_bᵀ F x_a cancels to ~1e-6 of its terms at 1 000-pixel coordinates); FMA
 * contraction is allowed, so sum carries no bit contract against another implementation, but the
 * same inputs give the same bits on every call: no floating-point atomics, a block-level
 * reduction and a fixed-order final pass.
 *
 * mvp_epipolar_lag_cost_plan : what a call with (T, J, n_cam_idx, max_lag) will use: the time
 *   tile in frames (a workgroup scores one tile of view a against all lags, csrc/sync.hip) and
 *   the workspace size in bytes (either may be NULL).
 * mvp_epipolar_lag_cost : workspace_dev >= the plan's bytes, owned by the caller (its contents
 *   are scratch); out_sum_dev [NP][2L+1] float64, out_cnt_dev [NP][2L+1] int64.  Requires T >= 1,
 *   1 <= J <= 1024, T·J < 2^31, 0 <= max_lag < T, min_conf not NaN, trunc_px finite and > 0.
 *   Stream-ordered: no host synchronisation and no allocation inside the call.
 * ------------------------------------------------------------------------- */
int mvp_epipolar_lag_cost_plan(int T, int J, int n_cam_idx, int max_lag, int* tile_out, int64_t* workspace_bytes);
int mvp_epipolar_lag_cost(const float* kpts_dev, int T, int J, int V, const double* cams_dev, int n_cams,
                          const int* cam_idx_host, int n_cam_idx, int max_lag, float min_conf, float trunc_px,
                          void* workspace_dev, int64_t workspace_bytes, double* out_sum_dev, int64_t* out_cnt_dev,
                          void* stream);

/* ---------------------------------------------------------------------------
 * Cross-view association of 2D skeletons: which skeleton of camera a and which of camera b are
 * the same person (no reference counterpart; the reference handles one person per camera).  Per
 * frame, the skeletons of all listed views are scored against each other by the epipolar
 * constraint of the block above and grouped so that a group holds at most one skeleton per view.
 *
 * kpts_dev [T][P][J][3][V] float32: kpts[:, p] is the kpts_2d layout of person slot p.  Slots are
 * independent per view (slot p of view a and slot p of view b need not be the same person); a slot
 * is empty when its keypoints are NaN.  cams_dev, cam_idx_host / n_cam_idx = nv as for
 * mvp_triangulate_robust: view i reads column cam_idx[i] and the parameters of camera cam_idx[i].
 *   Nodes: node n = i·P + p stands for (view position i, slot p); N = nv·P <= 64.
 *   Usable keypoint, ideal pixel x = (u, v, 1), F_ab, squared Sampson distance d²: exactly those of
 *     the epipolar lag-cost scan (min_conf as there).  A node is usable when at least min_joints of
 *     its J keypoints are usable.
 *   Affinity, fp64: for nodes n of view a and m of view b, a < b, over the joints usable in both
 *     nodes, skipping the terms whose denominator is 0 or whose d² is not finite:
 *       c(n, m) = mean_j min(d_j², trunc_px²)
 *     defined when at least min_joints terms remain, else "undefined", stored as −1.  Each
 *     unordered node pair is computed once: the matrix is symmetric by construction.
 *   Grouping, per frame: clusters start as the usable nodes, one each.  link(A, B) is the maximum
 *     of the defined affinities between a node of A and a node of B (complete linkage), undefined
 *     when there is none; the pair (A, B) is admissible when A and B share no view.  Repeat: among
 *     the admissible pairs with a defined link <= max_cost_px², merge the one with the smallest
 *     link, ties broken by the smallest (smallest node of A, smallest node of B) with A the
 *     cluster whose smallest node is smaller; stop when there is no such pair.  With undefined
 *     stored as −1, the links of a merged cluster are the element-wise maximum of two rows.
 *     0 < max_cost_px < trunc_px, so a link of exactly trunc_px² is never merged.
 *   Numbering: the final clusters, sorted by the key (−number of views in the cluster, smallest
 *     node), are groups 0, 1, ...
 * Arithmetic is fp64 with FMA contraction allowed; no atomics, so the same inputs give the same
 * bits on every call.  The group numbers equal those of an exact evaluation of the above whenever
 * every comparison the algorithm makes (a link against max_cost_px², the best link of a round
 * against the second best) has a relative margin above 1e-9.  max_cost_px and trunc_px are the
 * float32 values given, squared in fp64.
 *
 * mvp_associate_views_plan : checks (T, P, J, n_cam_idx) and the four parameters as the call
 *   does, and reports the LDS bytes of the association kernel's workgroup (one wavefront per
 *   frame, csrc/associate.hip) and the workspace size in bytes (either may be NULL).
 * mvp_associate_views : workspace_dev >= the plan's bytes, owned by the caller (it holds the
 *   undistorted pixels and the F matrices; its contents are scratch).
 *   out_group_dev [T][nv][P] int8: the node's group number, −1 for a node that is not usable.
 *   out_count_dev [T][2] uint8: {groups, groups seen by at least 2 views}.
 *   out_affinity_dev [T][NP][P][P] float64 or NULL: c of (view a slot p, view b slot q) for pair
 *     (a, b) in the pair order of the lag-cost scan, −1 where undefined.
 *   Requires T >= 1, 2 <= nv <= 8, P >= 1, nv·P <= 64, 1 <= J <= 255, T·P·J < 2^31,
 *   0 < max_cost_px < trunc_px both finite, 1 <= min_joints <= J, min_conf not NaN.
 *   Stream-ordered: no host synchronisation and no allocation inside the call.
 * ------------------------------------------------------------------------- */
int mvp_associate_views_plan(int T, int P, int J, int n_cam_idx, float min_conf, float trunc_px, float max_cost_px,
                             int min_joints, int* lds_bytes, int64_t* workspace_bytes);
int mvp_associate_views(const float* kpts_dev, int T, int P, int J, int V, const double* cams_dev, int n_cams,
                        const int* cam_idx_host, int n_cam_idx, float min_conf, float trunc_px, float max_cost_px,
                        int min_joints, void* workspace_dev, int64_t workspace_bytes, int8_t* out_group_dev,
                        uint8_t* out_count_dev, double* out_affinity_dev, void* stream);

/* ---------------------------------------------------------------------------
 * Left/right label swaps per camera, undone by multi-view consistency (no reference counterpart;
 * the reference takes the 2D detector's joint labels on trust).  The commonest gross error of a
 * top-down detector is a left/right exchange in one camera: a person seen from behind is mirrored
 * as a whole, a walker's legs are exchanged for a few frames.  For every frame, listed view and
 * unit of symmetric joint pairs this block decides whether that view's labels are exchanged: the
 * cameras must agree with each other (the epipolar constraint of the blocks above), and each
 * camera with its own previous frame (continuity in the image).
 *
 * kpts_dev [T][J][3][V] float32, cams_dev, cam_idx_host / n_cam_idx = nv, 2 <= nv <= 8: exactly
 * as for mvp_epipolar_lag_cost.
 * pairs_host [NS][2] int32: the (left, right) joint of every symmetric pair, 1 <= NS <= 64,
 *   indices in [0, J), all 2·NS of them distinct.
 * unit_host [NS] int32 in [0, U), every unit used, 1 <= U <= NS: the pairs of one unit are
 *   exchanged together (U = 1: the whole body).
 *   Usable keypoint, ideal pixel x, F_ab, squared Sampson distance d²: exactly those of the
 *     epipolar lag-cost scan.  View pairs p = (a, b), a < b, in its order, NP = nv·(nv−1)/2.
 *     A keypoint that is usable by that rule but whose ideal pixel comes out NaN (the
 *     undistortion overflows at absurd coordinates) counts as not usable here: it has no d².
 *   Cost tables, float64, for frame t, unit u; τ = trunc_px, μ = motion_trunc_px, w =
 *   motion_weight (the float32 values given, promoted to fp64):
 *     Symmetric pair k is complete in view a at t when both of its keypoints are usable there;
 *       n[t][u][a] = the number of complete pairs of unit u.
 *     Epipolar tables: over the pairs k of unit u that are complete in a and in b at t with all
 *       four d² finite and all four denominators non-zero (otherwise k contributes to neither),
 *       in ascending k:
 *         same[t][u][p]  = Σ min(d²(l_a, l_b), τ²) + min(d²(r_a, r_b), τ²)
 *         cross[t][u][p] = Σ min(d²(l_a, r_b), τ²) + min(d²(r_a, l_b), τ²)
 *     Motion tables: zero at t = 0; for t >= 1 over the pairs complete in a at both t and t − 1,
 *       with the raw float32 pixel positions q promoted to fp64:
 *         keep[t][u][a]   = w · Σ min(|q_l(t) − q_l(t−1)|², μ²) + min(|q_r(t) − q_r(t−1)|², μ²)
 *         change[t][u][a] = w · Σ min(|q_l(t) − q_r(t−1)|², μ²) + min(|q_r(t) − q_l(t−1)|², μ²)
 *     Prior table: prior[t][u][a] = swap_prior_px² · n[t][u][a].
 *     The products are done when the tables are built: the solver below only adds and compares,
 *     so FMA contraction cannot change its bits.  The tables themselves are fp64 with contraction
 *     allowed and carry no bit contract, but no atomics: the same inputs give the same bits.
 *   State, per unit: s in [0, 2^nv), bit a set when view a's labels of that unit are exchanged at
 *     t.  Units are solved independently.
 *   Frame cost E(t, s), accumulated in this order: start at 0; + prior[t][u][a] for a ascending
 *     over the set bits of s; then for p ascending + same[t][u][p] when bits a and b of s are
 *     equal, else + cross[t][u][p].
 *   Recursion: D_0(s) = E(0, s).  For t >= 1 start from G = D_{t−1} and flip(s) = 0.  For each
 *     view a = 0 .. nv−1 in turn, with s' = s xor 2^a:
 *         k = G(s) + keep[t][u][a],   c = G(s') + change[t][u][a];
 *     when c < k (strictly) the new G(s) = c and the new flip(s) = flip_old(s') | 2^a, otherwise
 *     the new G(s) = k and flip(s) stays.  Every state of a pass reads the old G and flip.  Then
 *     D_t(s) = G(s) + E(t, s) and bp[t][s] = flip(s), one byte.
 *   Answer: s_{T−1} is the smallest s that attains min D_{T−1}; s_{t−1} = s_t xor bp[t][s_t].
 *   Apply: out_kpts is a copy of kpts in which, for every set bit of s_t, the full (x, y, conf)
 *     records of l and r of the unit's pairs are exchanged in that view's column (columns that
 *     cam_idx does not list are copied).  An optional second array [T][V][J][C] float64 (the
 *     heatmaps_2d layout, C = 6) is treated the same way.  Applying the same mask twice restores
 *     the input's bits.
 * Consequences: complementing s in all views leaves the epipolar terms unchanged; the prior (a
 * detector is more often right than wrong) and the motion terms then fix which side is "left".
 * With two views and a mirror that begins after frame 0, the motion term singles out the view
 * whose labels jumped.  A unit with no data at a frame carries its state through unchanged: ties
 * keep.  Pairs a few pixels apart (eyes, ears) carry no evidence and are best left out.
 *
 * mvp_label_swap_plan : checks (T, J, nv, NS, U) and reports the workspace bytes that serve both
 *   mvp_label_swap_costs and mvp_label_swap_solve (may be NULL).
 * mvp_label_swap_solve_plan : checks (T, U, nv) and reports the bytes mvp_label_swap_solve alone
 *   needs (may be NULL), for tables that do not come from mvp_label_swap_costs.
 * mvp_label_swap_costs : the tables.  workspace_dev >= the plan's bytes, owned by the caller (its
 *   contents are scratch).  out_same_dev, out_cross_dev [T][U][NP] float64; out_keep_dev,
 *   out_change_dev, out_prior_dev [T][U][nv] float64; out_n_dev [T][U][nv] int32 or NULL.
 * mvp_label_swap_solve : the recursion and the backtrack on tables in that layout (they need not
 *   come from mvp_label_swap_costs).  workspace_dev holds bp: at least U · ceil256(T · 2^nv)
 *   bytes, which the plan's bytes cover.  out_swap_dev [T][U] uint8 = s_t per unit;
 *   out_cost_dev [U] float64 or NULL = min D_{T−1}.  One wavefront per unit runs the frames in
 *   sequence: latency-bound by construction.
 * mvp_label_swap_apply : gauss_dev and out_gauss_dev both NULL or both given; the outputs must not
 *   be the inputs; cam_idx_host must not list a column twice.
 * All require T >= 1, J >= 2, T·J < 2^31, 2 <= nv <= 8; the costs also trunc_px and
 * motion_trunc_px finite and > 0, motion_weight and swap_prior_px finite and >= 0, min_conf not
 * NaN.  Argument errors return MVP_ERR_ARG before any device work.  Stream-ordered: no host
 * synchronisation, no allocation and no host decision inside the calls.
 * ------------------------------------------------------------------------- */
int mvp_label_swap_plan(int T, int J, int n_cam_idx, int n_pairs, int n_units, int64_t* workspace_bytes);
int mvp_label_swap_solve_plan(int T, int n_units, int n_cam_idx, int64_t* workspace_bytes);
int mvp_label_swap_costs(const float* kpts_dev, int T, int J, int V, const double* cams_dev, int n_cams,
                         const int* cam_idx_host, int n_cam_idx, const int* pairs_host, int n_pairs,
                         const int* unit_host, int n_units, float min_conf, float trunc_px, float motion_trunc_px,
                         float motion_weight, float swap_prior_px, void* workspace_dev, int64_t workspace_bytes,
                         double* out_same_dev, double* out_cross_dev, double* out_keep_dev, double* out_change_dev,
                         double* out_prior_dev, int32_t* out_n_dev, void* stream);
int mvp_label_swap_solve(const double* same_dev, const double* cross_dev, const double* keep_dev,
                         const double* change_dev, const double* prior_dev, int T, int n_units, int n_cam_idx,
                         void* workspace_dev, int64_t workspace_bytes, uint8_t* out_swap_dev, double* out_cost_dev,
                         void* stream);
int mvp_label_swap_apply(const float* kpts_dev, const double* gauss_dev, int T, int J, int V, int C,
                         const int* cam_idx_host, int n_cam_idx, const int* pairs_host, int n_pairs,
                         const int* unit_host, int n_units, const uint8_t* swap_dev, float* out_kpts_dev,
                         double* out_gauss_dev, void* stream);

/* ---------------------------------------------------------------------------
 * Tracking of people through time: which group of frame t is the person of which group of an
 * earlier frame, so that a person keeps one number through the recording and through short
 * dropouts.  No reference counterpart (the reference handles one person per camera).  The input is
 * what triangulating the groups of the block above gives: per frame G skeletons of J joints in
 * world units, in no particular order from frame to frame.
 *
 * xyz_dev [M][T][G][J][3] float32: M independent sequences of T frames.
 *   Seen, present: a joint is seen when its three coordinates are finite; group (t, g) is present
 *     when at least one of its joints is seen.
 *   Lags: K = max_gap + 1; max_gap is the number of consecutive missing frames a track survives.
 *   Cost, fp64 from the f32 inputs: for present groups (t, g) and (t − k, h), over the joints seen
 *     in both, in ascending joint order,
 *       c = (Σ sqrt(dx² + dy² + dz²)) / count
 *     defined when count >= min_joints.
 *   Limit: limit_k = max_jump·(1 + gap_growth·(k − 1)), in fp64 from the two float32 values given.
 *   Open observation: at frame t, observation (t', h) is open when it is the latest observation of
 *     its track and t − t' <= K.
 *   Candidates of frame t: the triples (k, h, g) with 1 <= k <= K, t − k >= 0, (t − k, h) open,
 *     (t, g) present, c defined and c <= limit_k.
 *   Linking: the candidates sorted ascending by (c, k, h, g) are taken greedily: a candidate links
 *     g to the track of (t − k, h) when neither that track nor g has been taken in this frame.
 *     (k, h) names exactly one track, so the order is total.
 *   New tracks: the present groups left over start new tracks in ascending g; track numbers count
 *     up from 0 in order of first appearance.
 * Consequences: with max_gap = 0 and min_joints = 1 the track numbers are those of frame-to-frame
 * greedy linking (mvpose.people.link_tracks(xyz, max_jump)).  A track that is not observed for
 * more than max_gap frames is closed; the person then comes back under a new number.
 * Arithmetic is fp64 with FMA contraction allowed; no atomics on anything, so the same inputs give
 * the same bits on every call.  The track numbers and lags equal those of an exact evaluation of
 * the above whenever every comparison the algorithm makes (a cost against its limit, two
 * candidates' costs of one frame) has a relative margin above 1e-9.
 *
 * mvp_track_people_plan : checks (M, T, G, J, max_gap) as the call does and reports the LDS bytes
 *   of the kernel's workgroup (one wavefront per sequence, csrc/track.hip; may be NULL):
 *   (max_gap + 2)·G·(12·J + 4) + (max_gap + 1)·G²·4: a ring of the last K + 1 frames' joints, one
 *   int32 per (ring slot, group), and one int32 per combination (k, h, g).
 * mvp_track_people :
 *   out_track_dev [M][T][G] int32: the group's track number, −1 for an absent group.
 *   out_n_tracks_dev [M] int32: the number of tracks of each sequence.
 *   out_link_cost_dev [M][T][G] float64 or NULL: c of the link a group was taken by; NaN for a
 *     group that starts a track and for an absent group.
 *   out_link_lag_dev [M][T][G] uint8 or NULL: that link's k; 0 for a new track and for an absent
 *     group.
 *   Requires M >= 1, T >= 1, 1 <= G <= 8, 1 <= J <= 255, 0 <= max_gap <= 15, max_jump finite and
 *   > 0, gap_growth finite and >= 0, 1 <= min_joints <= J, M·T·G·J < 2^31 and the plan's LDS bytes
 *   <= 65536.  Argument errors return MVP_ERR_ARG before any device work.
 *   Stream-ordered: one launch, no allocation, no host synchronisation and no decision on the
 *   host.
 * ------------------------------------------------------------------------- */
int mvp_track_people_plan(int M, int T, int G, int J, int max_gap, int* lds_bytes);
int mvp_track_people(const float* xyz_dev, int M, int T, int G, int J, int max_gap, float max_jump,
                     float gap_growth, int min_joints, int32_t* out_track_dev, int32_t* out_n_tracks_dev,
                     double* out_link_cost_dev, uint8_t* out_link_lag_dev, void* stream);

/* ---------------------------------------------------------------------------
 * Bundle adjustment of the extrinsics over the 2D keypoints: R, T of the cameras that may have
 * moved since calibration, the 3D points, and a covariance of the camera unknowns.  No reference
 * counterpart (the reference's extrinsic branch is mvp_sgd_refine_cams: f32, Adam, at most two
 * learnable cameras, tied to trajectory windows, no uncertainty).
 *
 * kpts_dev [n_points][3][V], cams_dev, cam_idx_host / n_cam_idx (2..8) as for
 * mvp_triangulate_refine: view i reads column cam_idx[i] and the parameters of camera cam_idx[i].
 * Everything is fp64 with FMA contraction allowed; no atomics on floating-point data, so the same
 * inputs give the same bits on every call.
 *   Used view, observation z_i, weight W_i: exactly mvp_triangulate_refine's rules (mask_dev,
 *     min_conf, the three MVP_REFINE_W_* modes, gauss_dev / J, cov_floor).
 *   Unknowns: free_mask has bit i set when view i's R, T are optimised; F = popcount(free_mask),
 *     0 < F <= n_cam_idx - 1 (at least one listed view stays fixed), no bit at or above n_cam_idx.
 *     The other unknowns are the 3D points.  K and the distortion are never touched.  A free camera
 *     is perturbed as
 *       R <- exp([dw]x)·R   (Rodrigues; for |dw| < 1e-12: I + [dw]x)        T <- T + du
 *     so that for P = R·X + T: dP/d dw = -[P - T]x, dP/d du = I, dP/dX = R.
 *   Active point: at least 2 used views, a finite seed xyz0, and P_z > 0 in every used view at the
 *     seed (with the input cameras).  The active set is fixed at the start.  Inactive points take no
 *     part and return their seed's bits with point status 0x80.  A free view observed by fewer than
 *     3 active points ends the call at once with info status 3: cameras and points are returned
 *     unchanged.
 *   Cost: s² = rᵀ·W·r is the whitened squared residual of one used view, r = pi_i(X) - z_i (the
 *     forward model of mvp_triangulate_refine).  rho(s) = ½s² when huber_delta <= 0 or s <= delta,
 *     else delta·(s - ½delta); the IRLS weight is omega = 1 or delta/s, W~ = omega·W.
 *       f = Σ rho  +  Σ over the free views of ½|T_i - T_i⁰|²/sigma²
 *     the second sum only when trans_prior_sigma = sigma > 0, T⁰ being the input camera's T.  f is
 *     +inf when any used view of an active point has P_z <= 0.  With a single fixed camera the
 *     overall scale of (points, free translations) is unobservable from the pixels: the prior pins
 *     it, and sigma > 0 is then needed for S to be well conditioned.  With two or more fixed cameras
 *     their baseline sets the scale, nothing is unobservable, and sigma may be 0.
 *   Linearisation at a state with damping lambda, per active point p over its used views i:
 *       J_X = A·R_i (2x3),  J_c = A·[-[P - T]x, I] (2x6, free views),  A = d pixel / dP
 *       V_p = Σ J_Xᵀ W~ J_X,  g_p = Σ J_Xᵀ W~ r,  W_pi = J_cᵀ W~ J_X (6x3)
 *       U_i += J_cᵀ W~ J_c,  g_ci += J_cᵀ W~ r
 *       V*_p = V_p + lambda·diag V_p = L·Lᵀ (Cholesky)
 *       U*_i = U_i + lambda·diag U_i (+ I/sigma² on the translation block)
 *       g_ci += (T_i - T_i⁰)/sigma² with the prior
 *     Reduced system over the 6F camera unknowns, free views in ascending position, each (dw, du):
 *       S = blockdiag(U*) - Σ_p Y_p·Y_pᵀ,  Y_p = [W_pi·L⁻ᵀ]_i (6F x 3),  b = -g_c + Σ_p Y_p·(L⁻¹ g_p)
 *     S·dc = b by Cholesky, then dX_p = -V*⁻¹·(g_p + Σ_i W_piᵀ·dc_i).
 *   Solver: Levenberg-Marquardt, lambda = 1e-3 at the start.  A trial linearises at the current
 *     state, solves, and forms the trial state (cameras as above, X + dX).  It is accepted when
 *     f(trial) is finite and <= f: the state becomes the trial state and lambda <- max(lambda/10,
 *     1e-12); otherwise lambda <- 10·lambda.  A Cholesky pivot that is not > 0 (NaN included) in any
 *     active point's V* or in S is a rejected trial.  The run stops: converged (status 0) at the
 *     first accepted trial with f - f(trial) <= tol·f; stalled (status 2) when lambda > 1e12; out
 *     of trials (status 1) after max_iter trials — tested in this order after each trial.  With
 *     max_iter = 0 the call returns the seed state with f evaluated there (status 1).
 *
 * mvp_bundle_adjust_plan : checks (n_points >= 1, n_cam_idx, free_mask) as the calls do and reports
 *   the bytes of the caller-owned workspace (contents are scratch) both calls need.
 * mvp_bundle_adjust_system : ONE linearisation at the given cameras, the given f32 points xyz_dev
 *   (the active test is made at them) and the given lambda (finite, >= 0); no solve, no state.
 *   out_S_dev [6F][6F] full symmetric, out_b_dev [6F], out_cost_dev [1] (Σ rho; the prior's cost is
 *   0 at the input cameras, its I/sigma² is in S), out_counts_dev [2] int64 {active points, used
 *   views of active points}.  A failed pivot of some V* shows as NaN in S and b.
 * mvp_bundle_adjust : the whole optimisation, stream-ordered, with no host synchronisation and no
 *   decision on the host: the number of launches is fixed by max_iter (0..63), and a flag in the
 *   workspace turns the launches after the end into early returns.
 *   out_cams_dev [n_cams][MVP_CAM_DOUBLES]: a copy of cams_dev with the free views' R, T replaced
 *     and their P = K[R|T] recomputed with the loops of mvp_camera_pack.
 *   out_xyz_dev [n_points][3] float32; out_point_status_dev optional [n_points] uint8 (0 active,
 *     0x80 inactive).
 *   out_cam_cov_dev optional [6F][6F] float64: the inverse of S at the final state with lambda = 0
 *     (the prior's I/sigma² stays in it); NaN when that S, or some point's V, is not positive definite.
 *   out_info_dev [MVP_BA_INFO_DOUBLES]: f at the seed, f final, trials, accepted trials, status,
 *     final lambda, active points, used views.
 * min_conf not NaN; cov_floor >= 0; huber_delta and trans_prior_sigma not NaN (<= 0: off);
 * tol finite, > 0.  Argument errors return MVP_ERR_ARG before any device work.
 * ------------------------------------------------------------------------- */
#define MVP_BA_INFO_DOUBLES 8

int mvp_bundle_adjust_plan(int64_t n_points, int n_cam_idx, unsigned int free_mask, int64_t* workspace_bytes);
int mvp_bundle_adjust_system(const float* kpts_dev, int64_t n_points, int V, const double* cams_dev, int n_cams,
                             const int* cam_idx_host, int n_cam_idx, unsigned int free_mask, const float* xyz_dev,
                             const uint8_t* mask_dev, int weights, const double* gauss_dev, int J, float min_conf,
                             float cov_floor, double huber_delta, double trans_prior_sigma, double lambda,
                             void* workspace_dev, int64_t workspace_bytes, double* out_S_dev, double* out_b_dev,
                             double* out_cost_dev, int64_t* out_counts_dev, void* stream);
int mvp_bundle_adjust(const float* kpts_dev, int64_t n_points, int V, const double* cams_dev, int n_cams,
                      const int* cam_idx_host, int n_cam_idx, unsigned int free_mask, const float* xyz0_dev,
                      const uint8_t* mask_dev, int weights, const double* gauss_dev, int J, float min_conf,
                      float cov_floor, double huber_delta, double trans_prior_sigma, int max_iter, double tol,
                      void* workspace_dev, int64_t workspace_bytes, double* out_cams_dev, float* out_xyz_dev,
                      uint8_t* out_point_status_dev, double* out_cam_cov_dev, double* out_info_dev, void* stream);

/* ---------------------------------------------------------------------------
 * Trajectories fitted to the 2D keypoints, so that a frame seen by a single view still counts.  No
 * reference counterpart: the reference's SGD refinement (mvp_sgd_refine) scores every camera's
 * pixels against the trajectory plus the same second-difference cost, but in f32 with Adam over
 * thousands of steps, with no per-view mask, no robust loss and no weights of the view's own.
 * triangulate -> smooth needs two usable views of a joint in a frame; on a two-camera rig one
 * camera losing a joint removes it from 3D, and mvp_trajectory_smooth fills the gap from its ends
 * alone, although the camera that still sees the joint fixes two of its three coordinates.
 *
 * kpts_dev [T][P][3][V] float32: for one person the kpts_2d layout with P = J; several people are
 * concatenated along that axis.  Chains p are independent; chain p has unknowns X_t in R³,
 * t = 0..T-1.  cams_dev, cam_idx_host / n_cam_idx (2..8) as for mvp_triangulate_refine.
 *   Used view, observation z_i, weight W_i, forward model pi_i: exactly mvp_triangulate_refine's
 *     rules for point (t, p): mask_dev [T][P] uint8 (bit i: view i may be used) or NULL, min_conf,
 *     the three MVP_REFINE_W_* modes, gauss_dev [T][V][P][6] float64 (required for
 *     MVP_REFINE_W_GAUSS), cov_floor.  The used set depends on the keypoints alone and is the same
 *     at every state.  nviews(t, p) is its size.
 *   rho, omega: exactly mvp_bundle_adjust's Huber loss on the whitened residual s = sqrt(rᵀ·W·r),
 *     r = pi_i(X_t) - z_i: rho = ½s² when huber_delta <= 0 or s <= delta, else delta·(s - ½delta);
 *     omega = 1 or delta/s; W~ = omega·W.
 *   Valid chain: its seed is finite in every frame; every used view has P_z > 0 at the seed; at
 *     least 2 frames have at least 2 used views (that pins the affine-in-t null space of the
 *     prior); the cost at the seed is finite.  An invalid chain returns its seed's bits as
 *     out_xyz (NaNs included), NaN resid and cost, and status 0x80.
 *   Cost per chain:
 *       f(X) = Σ_t Σ_used rho  +  ½ λ Σ_{t=2}^{T-1} |X_t - 2 X_{t-1} + X_{t-2}|²
 *     and +inf when a used view has P_z <= 0.  λ = lambda_smooth in 1 / (world unit)²  per pixel-
 *     weight unit: with unit weights the data term is in pixels², so λ = (σ_px / σ_a)², σ_a the
 *     standard deviation of a joint's second difference per frame in world units.
 *   Linearisation at a state: per frame H~_t = Σ_used Jᵀ W~ J (3x3) and g~_t = Σ_used Jᵀ W~ r,
 *     J = d pi_i / dX.  With D₂ the (T-2)xT second-difference matrix,
 *       A = blockdiag(H~) + λ·(D₂ᵀD₂ ⊗ I₃),    G = g~ + λ·(D₂ᵀD₂ ⊗ I₃)·X.
 *     A frame with one used view contributes its rank-2 block, a frame with none contributes
 *     nothing and is carried by the prior.
 *   Solver, per chain: Levenberg-Marquardt, mu = 1e-3 at the start.  A trial solves
 *     (A + mu·diag A)·d = -G (block-pentadiagonal, by the partition method of
 *     mvp_trajectory_smooth; chunk as there) and forms X + d.  It is accepted when f(X + d) is
 *     finite and <= f: the state becomes X + d and mu <- max(0.1·mu, 1e-12); otherwise
 *     mu <- 10·mu.  A pivot of the solve that is not > 0 (NaN included) is a rejected trial.  The
 *     run stops: converged (status bit 0x40 clear) at the first accepted trial with
 *     f - f(trial) <= tol·f; stalled (0x40) when mu > 1e12; out of trials (0x40) after max_iter
 *     (0..63) trials — tested in this order after each trial.  Status bits 0-5 hold the number of
 *     trials.  With max_iter = 0 the call returns the seed with the cost evaluated there (0x40).
 * Everything is fp64 on the device from the float32 inputs, FMA contraction allowed (no bit
 * contract against another implementation).  No floating-point atomics: a chain's cost is summed
 * per tile of 256 frames in a fixed order and the tiles in ascending order, so the same inputs give
 * the same bits on every call.  The result does not depend on chunk beyond fp64 rounding.
 * Long stretches seen by one view only: the depth along that view's rays is then held by the prior
 * alone, and with a weak prior (small λ) it wanders: over tens of frames the fit can be worse than
 * the smoother's blind interpolation.  Such recordings need a stiffer prior (larger λ).
 *
 * mvp_trajectory_fit_plan : what a call with (T, P, chunk) will use: the chunk length, the chunks
 *   per chain and the bytes of the caller-owned workspace (contents are scratch); any may be NULL.
 * mvp_trajectory_fit_system : ONE linearisation of the data term at the given float32 trajectory
 *   xyz_dev [T][P][3]; no solve, no state, no validity test.  out_H_dev [T][P][6] float64 (xx, xy,
 *   xz, yy, yz, zz) and out_g_dev [T][P][3] float64: H~_t and g~_t (a used view behind its camera
 *   contributes what the arithmetic gives; a frame that is not finite gives NaN);
 *   out_nviews_dev [T][P] uint8; out_cost_dev [P][2] float64: {Σ rho (+inf behind a camera), the
 *   smoothness term with λ = 1, i.e. ½ Σ |second difference|²}.  All four are required.
 * mvp_trajectory_fit : the whole optimisation from the seed xyz0_dev [T][P][3] float32,
 *   stream-ordered, with no host synchronisation, no allocation and no decision on the host: the
 *   number of launches is fixed by max_iter, and a per-chain flag in the workspace makes the lanes
 *   of a finished chain return at once.
 *   out_xyz_dev [T][P][3] float32; out_resid_dev [T][P] float32 or NULL: Σ_used s² (not rho) at
 *   the final state, NaN when nviews = 0 and for invalid chains; out_nviews_dev [T][P] uint8 or
 *   NULL; out_cost_dev [P][2] float64 or NULL: f at the seed and at the final state;
 *   out_status_dev [P] uint8 or NULL.
 * Requires T >= 1, P >= 1, T·P < 2^31, 2 <= n_cam_idx <= 8, lambda_smooth and tol finite and > 0,
 * cov_floor >= 0, min_conf and huber_delta not NaN (huber_delta <= 0: off), 0 <= max_iter <= 63,
 * chunk = 0 or 4..4096.  Argument errors return MVP_ERR_ARG before any device work.
 * mvp_trajectory_fit_cov_plan, mvp_trajectory_fit_cov : the covariance of a fitted trajectory.  With
 *   A = blockdiag(H~) + λ·(D₂ᵀD₂ ⊗ I₃), H~ this fit's linearisation at the given xyz_dev (normally
 *   the fit's output; the used-view rules and the IRLS weights ω of huber_delta as above, no
 *   Marquardt factor), the call returns the diagonal and lag-1 blocks of Σ = A⁻¹.  This is the
 *   Gauss-Newton / Laplace covariance at that state: exact for the linearised model with the
 *   weights frozen there, not the posterior of the robust nonlinear cost.  A chain fails, with NaN
 *   in all of out_cov and out_cross and status 0x80 (others 0), when xyz_dev is not finite in some
 *   frame, a used view has P_z <= 0 there, fewer than 2 frames have >= 2 used views, or a pivot is
 *   not > 0.  Outputs, units and layout as mvp_trajectory_smooth_cov; out_cov_dev is required.
 *   Requires what mvp_trajectory_fit requires of the arguments both have.  Stream-ordered, no
 *   allocation, no host synchronisation.  Time, one MI355X, T = 100 000, P = 17, two views, chunk 0:
 *   3.71 ms against 2.23 ms for one trial of mvp_trajectory_fit, 1.67x.
 * Out of scope: blocks of Σ further than lag 1, the uncertainty of λ itself, and a covariance for
 * mvp_skeleton_fit (its chains are coupled: the per-chain inverse is not its posterior);
 * coupling between chains such as bone lengths (chains stay independent here; mvp_skeleton_fit
 * below couples them).  Sub-frame time offsets between the cameras: mvp_trajectory_fit_lag below.
 * ------------------------------------------------------------------------- */
int mvp_trajectory_fit_plan(int T, int P, int chunk, int* chunk_used, int* n_chunks, int64_t* workspace_bytes);
int mvp_trajectory_fit_system(const float* kpts_dev, int T, int P, int V, const double* cams_dev, int n_cams,
                              const int* cam_idx_host, int n_cam_idx, const float* xyz_dev, const uint8_t* mask_dev,
                              int weights, const double* gauss_dev, float min_conf, float cov_floor,
                              double huber_delta, double* out_H_dev, double* out_g_dev, uint8_t* out_nviews_dev,
                              double* out_cost_dev, void* stream);
int mvp_trajectory_fit(const float* kpts_dev, int T, int P, int V, const double* cams_dev, int n_cams,
                       const int* cam_idx_host, int n_cam_idx, const float* xyz0_dev, const uint8_t* mask_dev,
                       int weights, const double* gauss_dev, float min_conf, float cov_floor, double huber_delta,
                       double lambda_smooth, int max_iter, double tol, int chunk, void* workspace_dev,
                       int64_t workspace_bytes, float* out_xyz_dev, float* out_resid_dev, uint8_t* out_nviews_dev,
                       double* out_cost_dev, uint8_t* out_status_dev, void* stream);
int mvp_trajectory_fit_cov_plan(int T, int P, int chunk, int* chunk_used, int* n_chunks, int64_t* workspace_bytes);
int mvp_trajectory_fit_cov(const float* kpts_dev, int T, int P, int V, const double* cams_dev, int n_cams,
                           const int* cam_idx_host, int n_cam_idx, const float* xyz_dev, const uint8_t* mask_dev,
                           int weights, const double* gauss_dev, float min_conf, float cov_floor, double huber_delta,
                           double lambda_smooth, int chunk, void* workspace_dev, int64_t workspace_bytes,
                           float* out_cov_dev, float* out_cross_dev, uint8_t* out_status_dev, void* stream);

/* ---------------------------------------------------------------------------
 * The trajectory fit with sub-frame time offsets between the cameras.  No reference counterpart: the
 * reference aligns its recordings to a whole frame by hand.  Free-running cameras are never closer
 * than a fraction of a frame; a wrist at 3-5 m/s moves 10-17 cm per frame at 30 fps, and a solver
 * that takes the views of frame t for one instant puts that into the 3D point as a bias.
 *
 * Time: frame t of view i was taken at rig instant t + s_i (mvp_epipolar_lag_cost's convention).
 * The caller splits s_i = n_i + a_i, n_i = floor(s_i), 0 <= a_i < 1, aligns the recordings by the
 * integers n_i, and passes frac_host [n_cam_idx] float64, a_i of the listed view i.  Each a_i has
 * to be finite with 0 <= a_i < 1.
 *   Unknowns: X_t, chain p's position at the integer rig instants t = 0..T-1.  Chains are independent.
 *   Observation: view i's frame t scores the point
 *       Y = (1 - a_i)·X_t + a_i·X_{t+1}     (Y = X_t itself when a_i = 0: X_{t+1} is not read)
 *     with r = pi_i(Y) - z_i.  Used view, observation, weight, mask, rho, omega and the forward
 *     model are mvp_trajectory_fit's, with one rule added: a view with a_i > 0 is not used in frame
 *     T-1, whose neighbour does not exist.  nviews(t, p) counts accordingly.
 *   Cost per chain: f(X) = Σ_t Σ_used rho + ½ λ Σ_{t=2}^{T-1} |X_t - 2 X_{t-1} + X_{t-2}|², and +inf
 *     when a used view has P_z <= 0 at its Y.
 *   Linearisation: with H_i = Jᵀ W~ J and g_i = Jᵀ W~ r, J = d pi_i / dY, all at Y, the used
 *     observation (t, i) gives node t (1-a_i)²·H_i and (1-a_i)·g_i, node t+1 a_i²·H_i and a_i·g_i,
 *     and the pair (t, t+1) the symmetric block C_t += a_i(1-a_i)·H_i (a view with a_i = 0 adds
 *     exact zeros to node t+1 and to C_t, whatever its H_i is).  With H~_t, g~_t the nodes'
 *     sums,
 *       A = blockdiag(H~) + offdiag(C) + λ·(D₂ᵀD₂ ⊗ I₃),    G = g~ + λ·(D₂ᵀD₂ ⊗ I₃)·X,
 *     offdiag(C) holding C_t in the blocks (t, t+1) and (t+1, t).  The Marquardt factor multiplies
 *     the diagonal entries of A only.
 *   Valid chain, the Levenberg-Marquardt loop, the status byte, the stop tests and chunk: word for
 *     word mvp_trajectory_fit's, with P_z tested at the Ys of the seed.  A seed frame that is not
 *     finite makes its chain invalid as there.
 *   Offset derivative: per chain p and listed view i, over the used (t, i) with t + 1 < T (a view
 *     with a_i = 0 included; its frame T-1 excluded), with d = J·(X_{t+1} - X_t) at Y:
 *       ga[p][i] = Σ_t dᵀ W~ r,      ha[p][i] = Σ_t dᵀ W~ d.
 *     ga is the derivative of the chain's cost with respect to a_i at fixed X, and so, at a fitted
 *     state, the total derivative of the minimised cost (the envelope theorem): offsets can be
 *     refined from fits alone.  ha is the Gauss-Newton curvature at fixed X; the minimised cost's
 *     is much smaller (the trajectory gives way), so a Newton step needs differences of ga between
 *     fits, not ha.
 * fp64 on the device, FMA contraction allowed, no floating-point atomics, fixed summation orders
 * (a lane gathers its own node's terms; costs, ga and ha per tile of 256 frames in a fixed order,
 * the tiles ascending): the same inputs give the same bits on every call.  With every a_i = 0 the
 * call states mvp_trajectory_fit's problem; its sums are formed in another order, so the results
 * agree to fp64 rounding, not bit for bit.
 *
 * mvp_trajectory_fit_lag_plan : as mvp_trajectory_fit_plan, for the workspace of mvp_trajectory_fit_lag.
 * mvp_trajectory_fit_lag_system : ONE linearisation at the float32 trajectory xyz_dev [T][P][3]; no
 *   solve, no state, no validity test.  out_H_dev [T][P][6] (H~_t), out_C_dev [T][P][6] (C_t, the
 *   block between t and t+1, (xx, xy, xz, yy, yz, zz); row T-1 is zero), out_g_dev [T][P][3] (g~_t),
 *   out_nviews_dev [T][P] uint8, out_cost_dev [P][2] float64 as mvp_trajectory_fit_system's,
 *   out_dlag_dev [P][n_cam_idx][2] float64: {ga, ha}.  All six are required.
 * mvp_trajectory_fit_lag : the whole fit from the seed xyz0_dev, stream-ordered, with no host
 *   synchronisation, no allocation and no decision on the host.  Outputs as mvp_trajectory_fit's
 *   (out_resid: Σ_used s² of frame t's observations at their Y), and out_dlag_dev
 *   [P][n_cam_idx][2] float64 or NULL: {ga, ha} at the final state, NaN for an invalid chain.
 * Requires what mvp_trajectory_fit requires, and frac_host as above: frac_host NULL, or an entry
 * that is not finite, < 0 or >= 1, returns MVP_ERR_ARG naming frac before any device work.
 * Out of scope: a covariance for this fit, bone coupling with offsets, offsets that drift over a
 * recording, offsets in mvp_triangulate* and mvp_bundle_adjust, interpolation of a higher order
 * than linear (on a strongly curved path the linear model biases the offsets: DESIGN.md §4.17).
 * ------------------------------------------------------------------------- */
int mvp_trajectory_fit_lag_plan(int T, int P, int chunk, int* chunk_used, int* n_chunks, int64_t* workspace_bytes);
int mvp_trajectory_fit_lag_system(const float* kpts_dev, int T, int P, int V, const double* cams_dev, int n_cams,
                                  const int* cam_idx_host, int n_cam_idx, const double* frac_host,
                                  const float* xyz_dev, const uint8_t* mask_dev, int weights, const double* gauss_dev,
                                  float min_conf, float cov_floor, double huber_delta, double* out_H_dev,
                                  double* out_C_dev, double* out_g_dev, uint8_t* out_nviews_dev, double* out_cost_dev,
                                  double* out_dlag_dev, void* stream);
int mvp_trajectory_fit_lag(const float* kpts_dev, int T, int P, int V, const double* cams_dev, int n_cams,
                           const int* cam_idx_host, int n_cam_idx, const double* frac_host, const float* xyz0_dev,
                           const uint8_t* mask_dev, int weights, const double* gauss_dev, float min_conf,
                           float cov_floor, double huber_delta, double lambda_smooth, int max_iter, double tol,
                           int chunk, void* workspace_dev, int64_t workspace_bytes, float* out_xyz_dev,
                           float* out_resid_dev, uint8_t* out_nviews_dev, double* out_cost_dev, uint8_t* out_status_dev,
                           double* out_dlag_dev, void* stream);

/* ---------------------------------------------------------------------------
 * The trajectory fit with a person's joints coupled by bone lengths: the third of the costs the
 * reference refines against (reprojection, smoothness, body-part lengths; mvp_sgd_refine has all
 * three in f32 under Adam, mvp_trajectory_fit the first two).  A known upper-arm length pins the
 * depth of an elbow that one camera has lost on the ray of the camera that still sees it, which a
 * stiffer smoothness prior does not do.
 *
 * Every input of mvp_trajectory_fit with the same meaning, and P = G·J: chain p = g·J + j is joint
 * j of person (group) g, 1 <= J <= 255.  seg_host [n_seg][2] int, 0 <= n_seg <= 64: segment s joins
 * joints (a, b), a != b, both < J, no unordered pair twice.  seg_len_dev [G][n_seg] float32: one
 * set of lengths L per person, in world units; a length that is not finite or not > 0 makes that
 * segment dead for that person.  lambda_bone = β, finite and >= 0, in pixel-weight units per
 * (world unit)²: with unit weights β = (σ_px / σ_L)², σ_L the tolerance of a length.
 *   Valid chain: mvp_trajectory_fit's rule without its last clause: the seed is finite in every
 *     frame; every used view has P_z > 0 at the seed; at least 2 frames have at least 2 used views.
 *     An invalid chain takes no part: it returns its seed's bits with chain status 0x80, and the
 *     segments that end at it are dead.
 *   Valid group: at least one valid chain, and the group's cost at the seed is finite.  Every chain
 *     of an invalid group is returned as it came (chain status 0x80, NaN resid), the group's status
 *     is 0x80 and its costs are NaN.
 *   Cost per group, over its valid chains and live segments, r = |X_{t,b} - X_{t,a}|,
 *     n = (X_{t,b} - X_{t,a}) / r:
 *       f_g = Σ_chains (Σ_t Σ_used rho + ½ λ Σ_t |second difference|²) + ½ β Σ_t Σ_s (r - L_{g,s})²
 *     and +inf when a used view of a valid chain has P_z <= 0.  A term with r == 0 costs ½ β L² and
 *     contributes no gradient and no curvature.
 *   Linearisation: per chain mvp_trajectory_fit's H~_t and g~_t, plus for every live segment that
 *     ends at the chain's joint
 *       to g~_t at end b: β·(r - L)·n, at end a its negative (the exact gradient);
 *       to H~_t at both ends: 2β·[n nᵀ + max(0, 1 - L/r)·(I - n nᵀ)].
 *     That block is twice the positive-semidefinite part of the term's own Hessian; the factor 2
 *     bounds the a-b cross block, which is dropped.  So the chains stay independent inside a
 *     trial, and the coupling acts from trial to trial.
 *   Trial, per group with one mu_g: every valid chain solves (A_p + mu_g·diag A_p)·d_p = -G_p by
 *     mvp_trajectory_fit's solver and forms X_p + d_p.  A pivot that is not > 0 in any chain of the
 *     group rejects the group's trial.  Accept and stop are mvp_trajectory_fit's rules on f_g:
 *     mu_g = 1e-3 at the start, accepted when f_g(trial) is finite and <= f_g (mu_g <-
 *     max(0.1·mu_g, 1e-12)), else mu_g <- 10·mu_g; converged (0x40 clear) at the first accepted
 *     trial with f - f(trial) <= tol·f; stalled (0x40) when mu_g > 1e12; out of trials (0x40) after
 *     max_iter (0..63) trials.  Group status bits 0-5 hold the number of trials.  A group is
 *     accepted or rejected as a whole.  With max_iter = 0 the call returns the seed with f_g
 *     evaluated there (0x40).
 * Everything is fp64 on the device, FMA contraction allowed, no floating-point atomics: a segment's
 * cost is counted once, at its end a; a chain's terms are summed per tile of 256 frames as
 * mvp_trajectory_fit sums them, a group's chains in ascending order, the bones after the chains; the
 * same inputs give the same bits on every call.  With J = 1 the call states mvp_trajectory_fit's
 * problem: a chain whose cost at the seed is not finite is then an invalid group.  (With n_seg = 0
 * and J > 1 the chains share no term, but a person's chains are still accepted, rejected and
 * stopped together.)
 * Convergence across the coupling is linear, at a rate set by β against the data curvature (about
 * 5 per cm² per view with confidence weights on the synthetic two-camera rig): in the numpy
 * prototype β = 1..10 converged in 18-32 trials at tol 1e-4, β = 100 did not in 60.  On that rig
 * (120 frames, camera 1 losing the left elbow and wrist for 40 frames, λ = 0.25, β = 1, the 12
 * segments of examples/body_part_lengths.yaml at their true lengths) the restatement in
 * tests/skel_fit_ref.py and the device both end 3.3 cm RMS from the truth over the lost joints in
 * 18 trials, where mvp_trajectory_smooth's blind fill is 17.0 cm and the fit without bones 65.8 cm
 * off: a factor 5.2.  At T = 100 000, G = 1, J = 17, 12 segments, 2 views on one MI355X a trial
 * takes 2.3-2.6 ms against mvp_trajectory_fit's 2.2-2.3 ms: the solve both share dominates, the
 * bones add 0.1-0.2 ms in the linearise and cost kernels.
 *
 * mvp_skeleton_fit_plan : what a call with (T, P, J, chunk) will use: the chunk length, the chunks
 *   per chain and the bytes of the caller-owned workspace (contents are scratch); any may be NULL.
 * mvp_skeleton_fit_system : ONE linearisation at the given float32 trajectory xyz_dev [T][P][3]; no
 *   solve, no state, no validity test (every segment with a live length is live).
 *   out_H_dev [T][P][6] and out_g_dev [T][P][3] float64: H~_t and g~_t, data plus bone terms, β
 *   applied; out_nviews_dev [T][P] uint8; out_cost_dev [G][3] float64: {Σ rho (+inf behind a
 *   camera), the smoothness term with λ = 1, ½ Σ (r - L)², i.e. the bone term with β = 1}.  All
 *   four are required.
 * mvp_skeleton_fit : the whole optimisation from the seed xyz0_dev, stream-ordered, with no host
 *   synchronisation, no allocation and no decision on the host: the number of launches is fixed
 *   by max_iter.
 *   out_xyz_dev [T][P][3] float32; out_resid_dev [T][P] float32 or NULL and out_nviews_dev [T][P]
 *   uint8 or NULL as mvp_trajectory_fit's; out_bone_dev [T][G][n_seg] float32 or NULL: r - L at the
 *   final state, NaN for a dead segment or an invalid group; out_cost_dev [G][4] float64 or NULL:
 *   {f at the seed, f final, the bone term (β applied) at the seed, final};
 *   out_group_status_dev [G] uint8 or NULL; out_chain_status_dev [P] uint8 (0 or 0x80) or NULL.
 * Requires everything mvp_trajectory_fit requires, P a multiple of J, the seg_host rules above,
 * β finite and >= 0, seg_len_dev not NULL when n_seg > 0.  Argument errors return MVP_ERR_ARG before
 * any device work.
 * Out of scope: the exact coupled Gauss-Newton step (for example conjugate gradients preconditioned
 * by the per-chain solve); estimating the lengths inside the fit; joint-angle limits; the left /
 * right depth flip that a single bone leaves open (the seed decides the side).
 * ------------------------------------------------------------------------- */
int mvp_skeleton_fit_plan(int T, int P, int J, int chunk, int* chunk_used, int* n_chunks, int64_t* workspace_bytes);
int mvp_skeleton_fit_system(const float* kpts_dev, int T, int P, int V, const double* cams_dev, int n_cams,
                            const int* cam_idx_host, int n_cam_idx, const float* xyz_dev, const uint8_t* mask_dev,
                            int weights, const double* gauss_dev, float min_conf, float cov_floor, double huber_delta,
                            int J, const int* seg_host, int n_seg, const float* seg_len_dev, double lambda_bone,
                            double* out_H_dev, double* out_g_dev, uint8_t* out_nviews_dev, double* out_cost_dev,
                            void* stream);
int mvp_skeleton_fit(const float* kpts_dev, int T, int P, int V, const double* cams_dev, int n_cams,
                     const int* cam_idx_host, int n_cam_idx, const float* xyz0_dev, const uint8_t* mask_dev,
                     int weights, const double* gauss_dev, float min_conf, float cov_floor, double huber_delta,
                     double lambda_smooth, int J, const int* seg_host, int n_seg, const float* seg_len_dev,
                     double lambda_bone, int max_iter, double tol, int chunk, void* workspace_dev,
                     int64_t workspace_bytes, float* out_xyz_dev, float* out_resid_dev, uint8_t* out_nviews_dev,
                     float* out_bone_dev, double* out_cost_dev, uint8_t* out_group_status_dev,
                     uint8_t* out_chain_status_dev, void* stream);

/* ---------------------------------------------------------------------------
 * MPEG-4 Part 2 ('mp4v') decoding, host side — replaces cv.VideoCapture on the reference's
 * recordings (utils.py:849-909 read_video_as_frames; synchronize_videos.py:64,240 writes them with
 * cv2.VideoWriter_fourcc(*'mp4v')).  Simple Profile: I / P-VOPs, video packets, H.263 or MPEG
 * quantisation; frames out as BGR24 (cv2's channel order) or I420.  No device memory involved.
 *
 * mvp_mp4v_create : config = the VOS/VO/VOL headers (an MP4 'esds' DecoderSpecificInfo, or the
 *                   head of an elementary stream); returns the frame size.
 * mvp_mp4v_decode : one sample (any GOV / VOL headers and VOPs it holds); writes the frame after
 *                   its last VOP (a not-coded VOP repeats the previous frame) to bgr_out
 *                   [H][W][3] and / or yuv_out (I420, W x H luma then two (W+1)/2 x (H+1)/2
 *                   chroma planes); *vops_out = VOPs in the sample.
 * mvp_mp4v_selfcheck : verifies the decoder's VLC / scan tables (prefix-free, complete, the intra
 *                   TCOEF codes a permutation of the inter ones, LMAX order).
 * ------------------------------------------------------------------------- */
int mvp_mp4v_create(const uint8_t* config, size_t config_bytes, void** handle, int* width, int* height);
int mvp_mp4v_decode(void* handle, const uint8_t* data, size_t bytes, uint8_t* bgr_out, uint8_t* yuv_out,
                    int* vops_out);
int mvp_mp4v_destroy(void* handle);
int mvp_mp4v_selfcheck(void);

/* Split decode: the host entropy-decodes, the device reconstructs (bit-identical to
 * mvp_mp4v_decode's frames; the decoded frames land in device memory).
 *
 * mvp_mp4v_parse : one sample with at most one VOP, on a handle that never decodes.  Writes one
 *                  32-byte record per macroblock, raster order, to rec_out (host memory, rec_cap
 *                  records >= macroblocks):
 *                    uint8 kind (0 intra, 1 inter, 2 not coded = copy, 3 not reached), uint8 nnz[6],
 *                    uint8 pad, int16 mv[4][2] (luma 8x8 vectors, half-pel), int16 cmv[2] (chroma),
 *                    uint32 first coefficient entry;
 *                  and the inverse-quantised coefficients as uint32 entries (raster position << 16 |
 *                  uint16 value), block by block, to coef_out (*n_coef entries, at most coef_cap;
 *                  384 per macroblock always suffices).  vop_out[0] = 1 coded VOP, 0 not coded,
 *                  -1 no VOP in the sample; vop_out[1] = vop_rounding_type.
 * mvp_mp4v_reconstruct : stream-ordered; jobs_dev = n_jobs device records of 48 bytes
 *                  {const rec*, const coef*, uint8 cur*, const uint8 ref*, uint8 bgr* or NULL,
 *                   int32 coded, int32 rounding}, all device pointers: the VOP's records and
 *                  entries, the picture it writes and the previous one (each an I420 picture with
 *                  macroblock-aligned planes: Y 16*mb_w x 16*mb_h, then U and V 8*mb_w x 8*mb_h;
 *                  a slot's first pictures hold 128), and the [height][width][3] BGR frame out.
 *                  Jobs must write distinct pictures; a coded VOP's cur is the slot's older
 *                  picture (the host decoder's swap), a not-coded VOP outputs cur unchanged. */
int mvp_mp4v_parse(void* handle, const uint8_t* data, size_t bytes, void* rec_out, int64_t rec_cap,
                   uint32_t* coef_out, int64_t coef_cap, int64_t* n_coef, int* vop_out);
int mvp_mp4v_reconstruct(const void* jobs_dev, int n_jobs, int width, int height, void* stream);
/* mvp_mp4v_parse over samples data[0..n) in one call (one GIL release per GOP from Python):
 * sample k's records at rec_out + k * 32 * macroblocks, its coefficients packed after sample
 * k-1's in coef_out (n_coef[k] entries), vop_out[2k..2k+1].  Stops before a sample that might not
 * fit (fewer than 384 entries per macroblock left); *n_done = samples parsed. */
int mvp_mp4v_parse_many(void* handle, int n, const uint8_t* const* data, const size_t* bytes, void* rec_out,
                        uint32_t* coef_out, int64_t coef_cap, int64_t* n_coef, int* vop_out, int* n_done);

/* ---------------------------------------------------------------------------
 * Baseline JPEG split decode — Motion-JPEG AVI frames and the reference's frame<N>.jpg
 * directories (utils.py:851-860): the host entropy-decodes, the device reconstructs, and the
 * frames land in device memory bit-identical to libjpeg-turbo's decode (islow IDCT, fancy
 * upsampling, jdcolor's fixed-point YCbCr -> RGB), stored BGR.
 *
 * Supported: SOF0, 8-bit, Huffman coded, one interleaved scan of 1 component (grayscale, 1x1) or
 * of 3 components YCbCr with luma sampling 1x1, 2x1 or 2x2 over 1x1 chroma; 8-bit DQT; DHT, or
 * the Annex K tables in every slot 0 / 1 a frame leaves undefined; DRI / RSTn; 0xFF00 stuffing,
 * fill bytes; APPn / COM skipped; bytes after EOI ignored.  Anything else is reported in
 * mvp_jpeg_frame_info.status (MVP_JPEG_*), never guessed:
 *   PROCESS     not baseline sequential Huffman (SOF1, SOF2, arithmetic coding, DNL ...)
 *   PRECISION   12-bit samples or a 16-bit quantisation table
 *   COMPONENTS  a component count other than 1 or 3
 *   SAMPLING    other sampling factors
 *   SCANS       more than one scan, or a scan that does not interleave all components
 *   COLOUR      an Adobe APP14 segment, or component ids 'R' 'G' 'B' without JFIF: libjpeg may
 *               pick a colour transform other than YCbCr
 *   RANGE       a dequantised coefficient value * q outside int16, where libjpeg-turbo's SIMD
 *               and C paths differ (no 8-bit encoder writes such a frame)
 * A malformed or truncated stream is MVP_ERR_ARG with the position in mvp_last_error(); no call
 * reads past data + bytes.
 *
 * mvp_jpeg_info  : the frame's size, components, luma sampling and status from its headers.
 *                  check_range != 0 also walks the scan, which RANGE, a second scan and a
 *                  truncated scan need; without it those are left to mvp_jpeg_parse.
 * mvp_jpeg_parse : one frame.  A supported frame (info->status == MVP_JPEG_OK) writes
 *                    qt_out[3][64]  the components' quantisation tables, natural (row-major) order;
 *                    off_out[blocks + 1]  (off_cap entries > blocks): block b owns the entries
 *                      [off[b], off[b + 1]) of coef_out.  Blocks are numbered in scan order over the
 *                      MCU-padded component planes: MCU by MCU in raster order (an MCU is
 *                      8 h_samp x 8 v_samp pixels); inside an MCU the h_samp x v_samp luma blocks in
 *                      raster order, then the Cb block, then the Cr block.  info->blocks counts them;
 *                    coef_out  the non-zero QUANTISED coefficients as uint32 entries (natural-order
 *                      position << 16 | uint16 value), *n_coef of them; coef_cap must be at least
 *                      min(64 blocks, 4 bytes + blocks) + 64 (an entry takes two bits of the scan).
 *                      Dequantisation is the device's (the products need more than 16 bits).
 *                  An unsupported frame writes only *info and *n_coef = 0 and returns MVP_OK.
 * mvp_jpeg_parse_many : mvp_jpeg_parse over frames data[0..n) in one call (one GIL release from
 *                  Python): frame k's info[k], qt_out + 192 k, off_out + k off_stride (off_stride
 *                  entries, > the frames' blocks), its entries packed after frame k-1's in coef_out
 *                  (n_coef[k]; its offsets count from its own first entry).  Stops before a frame
 *                  that might not fit (fewer entries left than mvp_jpeg_parse asks for); *n_done =
 *                  frames handled.  A malformed frame returns its error with *n_done = its index.
 * mvp_jpeg_reconstruct : stream-ordered; jobs_dev = n_jobs device records of 48 bytes
 *                  {const uint32 off*, const uint32 coef*, const uint16 qt*, uint8 planes*,
 *                   uint8 bgr*, uint8 components, h_samp, v_samp, pad[5]}, all device pointers: one
 *                  frame's offsets, entries and tables as mvp_jpeg_parse wrote them, scratch for its
 *                  padded component planes (*plane_bytes of mvp_jpeg_scratch; 8-byte aligned) and
 *                  the [height][width][3] BGR frame out.  All frames are width x height; their
 *                  sampling may differ.  Two launches: blocks -> planes (dequantise, IDCT), planes
 *                  -> BGR (upsample, colour).
 * mvp_jpeg_scratch : the most blocks and plane bytes a width x height frame of any supported
 *                  sampling has (what to size off_stride - 1 and the scratch with).
 * ------------------------------------------------------------------------- */
#define MVP_JPEG_OK 0
#define MVP_JPEG_PROCESS 1
#define MVP_JPEG_PRECISION 2
#define MVP_JPEG_COMPONENTS 3
#define MVP_JPEG_SAMPLING 4
#define MVP_JPEG_SCANS 5
#define MVP_JPEG_COLOUR 6
#define MVP_JPEG_RANGE 7

typedef struct mvp_jpeg_frame_info {
    int32_t width, height;
    int32_t components;      /* 1 or 3 when supported */
    int32_t h_samp, v_samp;  /* luma sampling factors */
    int32_t status;          /* MVP_JPEG_OK or the reason the frame is unsupported */
    int32_t blocks;          /* 8x8 blocks of the scan (supported frames) */
    int32_t reserved;
} mvp_jpeg_frame_info;

int mvp_jpeg_info(const uint8_t* data, size_t bytes, int check_range, mvp_jpeg_frame_info* info);
int mvp_jpeg_parse(const uint8_t* data, size_t bytes, mvp_jpeg_frame_info* info, uint16_t* qt_out, uint32_t* off_out,
                   int64_t off_cap, uint32_t* coef_out, int64_t coef_cap, int64_t* n_coef);
int mvp_jpeg_parse_many(int n, const uint8_t* const* data, const size_t* bytes, mvp_jpeg_frame_info* info,
                        uint16_t* qt_out, uint32_t* off_out, int64_t off_stride, uint32_t* coef_out, int64_t coef_cap,
                        int64_t* n_coef, int* n_done);
int mvp_jpeg_scratch(int width, int height, int* blocks, int64_t* plane_bytes);
int mvp_jpeg_reconstruct(const void* jobs_dev, int n_jobs, int width, int height, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MVPOSE_H */
