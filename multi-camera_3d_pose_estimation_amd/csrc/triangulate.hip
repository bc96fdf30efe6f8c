// Batched multi-view triangulation for gfx950 — one (frame, joint) problem per lane.  Where it lives:
//   tri_common.h            the OpenCV numerics contract; undistortion, Jacobi SVD, QR / inverse
//                           iteration and its certification, dlt_null_vector, the f32
//                           dehomogenisation; the entry points' shared argument checks
//   triangulate.hip         (this file) MVP_TRI_REFERENCE and MVP_TRI_ALL_VIEWS kernels, the
//                           float64 pair kernel; mvp_triangulate, mvp_triangulate_points_f64
//   triangulate_tol.hip     MVP_TRI_TOLERANCE: the certified two-camera solver, its exact fallback
//                           launch and per-stream list; mvp_triangulate_fallback_total
//   triangulate_robust.hip  outlier-view rejection; mvp_triangulate_robust
//   triangulate_peaks.hip   the robust scheme over up to MVP_MAX_PEAKS candidates per view, choosing
//                           one per inlier view; mvp_triangulate_peaks
//   triangulate_refine.hip  Levenberg-Marquardt refinement + covariance; mvp_triangulate_refine
#pragma clang fp contract(off)

#include "tri_common.h"

namespace {

// Solver stages.  kExact: the restatement for every lane (OpenCV undistortion
// with IEEE divisions, Jacobi SVD).  kFast: fast undistortion (the same rounding) + QR /
// inverse iteration, with the Jacobi restatement (on the same A) for the lanes whose
// iteration has not provably converged or whose f32 outputs are not certified equal to the
// restatement's (null_vector_certified): bit-identical to kExact.
//
// Measured and dropped (tools/pmc_tri.sh, V=2, 1.7 M points): moving the Jacobi
// fallback to a second launch over marked lanes cuts the fast kernel from 110 to
// 66 VGPRs (4 -> 7 waves per SIMD) but made it slower (69 vs 58 us; VALU busy
// 59 % vs 73 %), and the marker sweep cost another 23 us.
enum Stage { kExact = 0, kFast = 1, kTol = 2 };

template <int S>
__device__ __forceinline__ void undistort_view(float u, float v, const double* __restrict__ c, const CamFast& cf,
                                               float& ox, float& oy) {
    if constexpr (S == kExact)
        undistort_point(u, v, c, ox, oy);
    else
        undistort_point_fast(u, v, c, cf, ox, oy);
}

// MVP_TRI_REFERENCE: top-2 listed cameras by confidence (ascending), params keyed
// by selection position (reference quirk, pose_estimation.py:36-45).
template <int S>
__device__ __forceinline__ void triangulate_reference_body(
    const float* __restrict__ kpts, int64_t n, int V, const double* __restrict__ cams, int n_cams,
    CamIdx ci, int n_ci, float* __restrict__ out, double* __restrict__ out4) {
    __shared__ double scam[kMaxCams][MVP_CAM_DOUBLES];
    __shared__ CamFast sfast[kMaxCams];
    load_cams(scam, sfast, cams, n_cams);
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    const float* __restrict__ kp = kpts + p * 3 * V;
    // stable ascending argsort, NaN last; keep the last two (pose_estimation.py:36)
    int best = 0, second = -1;
    float cbest = kp[2 * V + ci.v[0]];
    float csecond = 0.f;
#pragma unroll
    for (int i = 1; i < kMaxCams; i++) {
        if (i < n_ci) {
            const float c = kp[2 * V + ci.v[i]];
            const bool after_best = isnan(c) ? true : (isnan(cbest) ? false : (c >= cbest));
            if (after_best) {
                second = best;
                csecond = cbest;
                best = i;
                cbest = c;
            } else {
                const bool after_second =
                    (second < 0) ? true : (isnan(c) ? true : (isnan(csecond) ? false : (c >= csecond)));
                if (after_second) {
                    second = i;
                    csecond = c;
                }
            }
        }
    }
    const int pos0 = second, pos1 = best;  // top_indices = [lower-conf, higher-conf]
    const int col0 = ci.v[pos0], col1 = ci.v[pos1];
    float u0x, u0y, u1x, u1y;
    // points come from the selected columns; parameters from camera key = position
    undistort_view<S>(kp[col0], kp[V + col0], scam[pos0], sfast[pos0], u0x, u0y);
    undistort_view<S>(kp[col1], kp[V + col1], scam[pos1], sfast[pos1], u1x, u1y);
    double A[4][4];
    add_view_rows(A, 0, u0x, u0y, scam[pos0] + 26);
    add_view_rows(A, 2, u1x, u1y, scam[pos1] + 26);
    double nv[4];
    dlt_null_vector<S == kExact, 4>(A, nv);
    write_result(nv, p, out, out4);
}

// MVP_TRI_ALL_VIEWS: one 2·NV x 4 DLT over the NV listed views.
template <int S, int NV>
__device__ __forceinline__ void triangulate_all_views_body(
    const float* __restrict__ kpts, int64_t n, int V, const double* __restrict__ cams, int n_cams,
    CamIdx ci, float* __restrict__ out, double* __restrict__ out4) {
    __shared__ double scam[kMaxCams][MVP_CAM_DOUBLES];
    __shared__ CamFast sfast[kMaxCams];
    load_cams(scam, sfast, cams, n_cams);
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    const float* __restrict__ kp = kpts + p * 3 * V;
    double A[2 * NV][4];
#pragma unroll
    for (int j = 0; j < NV; j++) {
        const int col = ci.v[j];
        float ux, uy;
        undistort_view<S>(kp[col], kp[V + col], scam[col], sfast[col], ux, uy);
        add_view_rows(A, 2 * j, ux, uy, scam[col] + 26);
    }
    double nv[4];
    dlt_null_vector<S == kExact, 2 * NV>(A, nv);
    write_result(nv, p, out, out4);
}

template <int S>
__global__ __launch_bounds__(kBlock) void triangulate_reference_kernel(
    const float* __restrict__ kpts, int64_t n, int V, const double* __restrict__ cams, int n_cams, CamIdx ci,
    int n_ci, float* __restrict__ out, double* __restrict__ out4) {
    triangulate_reference_body<S>(kpts, n, V, cams, n_cams, ci, n_ci, out, out4);
}

template <int S, int NV>
__global__ __launch_bounds__(kBlock) void triangulate_all_views_kernel(
    const float* __restrict__ kpts, int64_t n, int V, const double* __restrict__ cams, int n_cams, CamIdx ci,
    float* __restrict__ out, double* __restrict__ out4) {
    triangulate_all_views_body<S, NV>(kpts, n, V, cams, n_cams, ci, out, out4);
}

// utils.triangulate_points (utils.py:1277-1336) on float64 keypoints, as the extrinsic
// branch calls it on its Gaussian samples (pose_refinement.py:811): cv.undistortPoints keeps
// CV_64F (no f32 rounding of the undistorted points), cv.triangulatePoints builds the same
// fp64 A and writes a CV_64F points4D, cv.convertPointsFromHomogeneous divides in double
// (scale = w != 0 ? 1./w : 1.).  kpts: (n, 2 views, 2) [point][view][x, y]; cams: the two
// views' records (camera 1 first).  Exact Jacobi restatement for every point.
__global__ __launch_bounds__(kBlock) void triangulate_pairs_f64_kernel(const double* __restrict__ kpts, int64_t n,
                                                                       const double* __restrict__ cams,
                                                                       double* __restrict__ out,
                                                                       double* __restrict__ out4) {
    __shared__ double scam[2][MVP_CAM_DOUBLES];
    for (int i = threadIdx.x; i < 2 * MVP_CAM_DOUBLES; i += blockDim.x) scam[i / MVP_CAM_DOUBLES][i % MVP_CAM_DOUBLES] = cams[i];
    __syncthreads();
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    const double* k = kpts + 4 * p;
    double E[4][4];
#pragma unroll
    for (int q = 0; q < 2; q++) {
        double ex, ey;
        undistort_point_f64(k[2 * q], k[2 * q + 1], scam[q], ex, ey);
        add_view_rows(E, 2 * q, ex, ey, scam[q] + 26);
    }
    double nv[4];
    dlt_null_vector<true, 4>(E, nv);
    const double w = nv[3];
    const double s = (w != 0.) ? 1. / w : 1.;
    out[3 * p + 0] = nv[0] * s;
    out[3 * p + 1] = nv[1] * s;
    out[3 * p + 2] = nv[2] * s;
    if (out4) {
#pragma unroll
        for (int q = 0; q < 4; q++) out4[4 * p + q] = nv[q];
    }
}

}  // namespace

extern "C" int mvp_triangulate(const float* kpts, int64_t n_points, int V, const double* cams, int n_cams,
                               const int* cam_idx, int n_cam_idx, int mode, float* out_xyz, double* out_xyzw,
                               void* stream) {
    MVP_ABI_BEGIN
    const char* fn = "mvp_triangulate";
    const CamIdx ci = tri_parse_args(fn, n_points, V, n_cams, cam_idx, n_cam_idx);
    if (n_points == 0) return MVP_OK;
    MVP_REQUIRE(kpts && cams && out_xyz, "mvp_triangulate: null device pointer");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const unsigned blocks = tri_grid(fn, n_points);
    const bool exact = (mode & MVP_TRI_EXACT_JACOBI) != 0;
    const bool tol = (mode & MVP_TRI_TOLERANCE) != 0;
    MVP_REQUIRE(!(exact && tol), "mvp_triangulate: MVP_TRI_EXACT_JACOBI and MVP_TRI_TOLERANCE exclude each other");
    mode &= ~(MVP_TRI_EXACT_JACOBI | MVP_TRI_TOLERANCE);
    const dim3 grid(blocks), block(kBlock);
    if (mode == MVP_TRI_REFERENCE) {
        MVP_REQUIRE(n_cam_idx <= n_cams, "mvp_triangulate: reference mode keys params by position: need "
                    "n_cam_idx <= n_cams");
        if (tol && n_cam_idx == 2 && n_points < (1LL << 32))
            mvp::launch_triangulate_tol2(kpts, n_points, V, cams, n_cams, ci.v, blocks, out_xyz, out_xyzw, s);
        else if (exact)
            hipLaunchKernelGGL(triangulate_reference_kernel<kExact>, grid, block, 0, s, kpts, n_points, V, cams,
                               n_cams, ci, n_cam_idx, out_xyz, out_xyzw);
        else
            hipLaunchKernelGGL(triangulate_reference_kernel<kFast>, grid, block, 0, s, kpts, n_points, V, cams,
                               n_cams, ci, n_cam_idx, out_xyz, out_xyzw);
    } else if (mode == MVP_TRI_ALL_VIEWS) {
        tri_dispatch_views(n_cam_idx, [&](auto nv) {
            constexpr int NV = decltype(nv)::value;
            if (exact)
                hipLaunchKernelGGL((triangulate_all_views_kernel<kExact, NV>), grid, block, 0, s, kpts, n_points, V,
                                   cams, n_cams, ci, out_xyz, out_xyzw);
            else
                hipLaunchKernelGGL((triangulate_all_views_kernel<kFast, NV>), grid, block, 0, s, kpts, n_points, V,
                                   cams, n_cams, ci, out_xyz, out_xyzw);
        });
    } else {
        mvp::fail(MVP_ERR_ARG, "mvp_triangulate: unknown mode %d", mode);
    }
    MVP_HIP(hipGetLastError());
    MVP_ABI_END
}

extern "C" int mvp_triangulate_points_f64(const double* kpts_2d, int64_t n_points, const double* cams,
                                          double* out_xyz, double* out_xyzw, void* stream) {
    MVP_ABI_BEGIN
    MVP_REQUIRE(n_points >= 0, "mvp_triangulate_points_f64: n_points < 0");
    if (n_points == 0) return MVP_OK;
    MVP_REQUIRE(kpts_2d && cams && out_xyz, "mvp_triangulate_points_f64: null device pointer");
    const unsigned blocks = tri_grid("mvp_triangulate_points_f64", n_points);
    hipLaunchKernelGGL(triangulate_pairs_f64_kernel, dim3(blocks), dim3(kBlock), 0,
                       reinterpret_cast<hipStream_t>(stream), kpts_2d, n_points, cams, out_xyz, out_xyzw);
    MVP_HIP(hipGetLastError());
    MVP_ABI_END
}
