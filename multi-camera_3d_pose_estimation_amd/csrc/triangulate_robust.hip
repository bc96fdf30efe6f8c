// mvp_triangulate_robust: N-view triangulation with outlier-view rejection (numerics contract and
// shared device code in tri_common.h; map of the triangulation files in triangulate.hip).
#pragma clang fp contract(off)

#include "tri_common.h"

namespace {

// ----------------------------------------------------------------- robust N-view mode
// mvp_triangulate_robust: the all-views DLT with per-point outlier-view rejection, an inlier
// mask and a reprojection-error read-out (no reference counterpart; algorithm in mvpose.h).
// Per lane:
//   * every listed view is undistorted once (f32 result, as in the all-views kernel) and parked in
//     LDS, [view][lane] (bank-conflict free), with its confidence: the pair loop of step B indexes
//     views at run time, which a per-lane register array cannot do without going to scratch, and
//     the DLT's A (2·NV x 4 fp64) is rebuilt from these values whenever a solve needs it;
//   * step A and the final solve of step B are ONE copy of the all-views solver (QR + inverse
//     iteration, certified, else the Jacobi restatement) inside a two-trip loop over a view mask:
//     rows of the views outside the mask are exact zeros, which leaves the Jacobi result's bits
//     those of the compacted system (x + 0·y is exact), so the float32 point equals the oracle's
//     over exactly the masked views;
//   * step B (the 4x4 DLT of every pair of valid views, one-sided Jacobi: accurate whatever the
//     pair's conditioning; only selects, no bit contract) is entered under a wave ballot: a wave
//     whose points all pass step A never runs it.
// Reprojection error of a view against a homogeneous X: reprojection_error (tri_common.h).

// NV = 8 left to the compiler takes 256 VGPRs + 17 AGPRs = 1 wave per SIMD; held at 2 waves
// (256 VGPRs, 80 B/lane of scratch) it measured 0.199 against 0.285 ms per 1 M clean points.
template <int NV>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(NV == 8 ? 2 : 1))) void triangulate_robust_kernel(
    const float* __restrict__ kpts, int64_t n, int V, const double* __restrict__ cams, int n_cams, CamIdx ci,
    float inlier_px, float min_conf, float* __restrict__ out, uint8_t* __restrict__ out_mask,
    float* __restrict__ out_err) {
    __shared__ double scam[kMaxCams][MVP_CAM_DOUBLES];
    __shared__ CamFast sfast[kMaxCams];
    __shared__ int scol[kMaxCams];
    __shared__ float s_ux[NV][kBlock], s_uy[NV][kBlock], s_conf[NV][kBlock];
#pragma unroll
    for (int j = 0; j < NV; j++)
        if ((int)threadIdx.x == j) scol[j] = ci.v[j];
    load_cams(scam, sfast, cams, n_cams);  // ends in the block's barrier
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    const int tid = threadIdx.x;
    const float* __restrict__ kp = kpts + p * 3 * V;
    const double inl = (double)inlier_px;
    unsigned valid = 0;
#pragma unroll
    for (int j = 0; j < NV; j++) {
        const int col = ci.v[j];
        const float x = kp[col], y = kp[V + col], c = kp[2 * V + col];
        float ux, uy;
        undistort_point_fast(x, y, scam[col], sfast[col], ux, uy);
        const bool ok = view_usable(x, y, c, min_conf) && isfinite(ux) && isfinite(uy);
        valid |= (ok ? 1u : 0u) << j;
        s_ux[j][tid] = ux;
        s_uy[j][tid] = uy;
        s_conf[j][tid] = c;
    }
    const float qnan = __builtin_nanf("");
    unsigned mask = valid;                  // the views of the next solve
    bool active = __popc(valid) >= 2;       // this lane takes part in the next solve
    bool failed = !active;                  // NaN point, empty mask
    float xyz[3] = {qnan, qnan, qnan};
    float err[NV];
#pragma unroll
    for (int j = 0; j < NV; j++) err[j] = qnan;
#pragma unroll 1
    for (int pass = 0; pass < 2; pass++) {
        bool all_in = true;
        if (active) {
            double nv[4];
            {
                double A[2 * NV][4];
#pragma unroll
                for (int j = 0; j < NV; j++) {
                    if ((mask >> j) & 1u) {
                        add_view_rows(A, 2 * j, s_ux[j][tid], s_uy[j][tid], scam[ci.v[j]] + 26);
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; k++) A[2 * j][k] = A[2 * j + 1][k] = 0.0;
                    }
                }
                dlt_null_vector<false, 2 * NV>(A, nv);
            }
            dehomogenize_f32(nv, xyz);
            const double X[4] = {(double)xyz[0], (double)xyz[1], (double)xyz[2], 1.0};
#pragma unroll
            for (int j = 0; j < NV; j++)
                if ((valid >> j) & 1u) {
                    const double e = reprojection_error(scam[ci.v[j]] + 26, X, s_ux[j][tid], s_uy[j][tid]);
                    err[j] = (float)e;
                    all_in = all_in && (e <= inl);
                }
        }
        if (pass == 1) break;
        const bool need_b = active && !all_in;
        if (__ballot(need_b) == 0) break;  // every point of the wave accepted in step A (or has < 2 views)
        active = need_b;
        if (need_b) {
            int best_cnt = -1;
            float best_sum = 0.f;
            unsigned best_mask = 0;
#pragma unroll 1
            for (int a = 0; a < NV - 1; a++) {
#pragma unroll 1
                for (int b = a + 1; b < NV; b++) {
                    if (((valid >> a) & 1u) && ((valid >> b) & 1u)) {
                        const double* __restrict__ Pa = scam[scol[a]] + 26;
                        const double* __restrict__ Pb = scam[scol[b]] + 26;
                        const double xa = s_ux[a][tid], ya = s_uy[a][tid], xb = s_ux[b][tid], yb = s_uy[b][tid];
                        double At[4][4];
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            At[k][0] = xa * Pa[8 + k] - Pa[0 + k];
                            At[k][1] = ya * Pa[8 + k] - Pa[4 + k];
                            At[k][2] = xb * Pb[8 + k] - Pb[0 + k];
                            At[k][3] = yb * Pb[8 + k] - Pb[4 + k];
                        }
                        double X[4];
                        jacobi_null_vector<4>(At, X);
                        int cnt = 0;
                        float sum = 0.f;  // f32, ascending view position
                        unsigned m = 0;
#pragma unroll
                        for (int j = 0; j < NV; j++)
                            if ((valid >> j) & 1u) {
                                const double e = reprojection_error(scam[ci.v[j]] + 26, X, s_ux[j][tid], s_uy[j][tid]);
                                if (e <= inl) {
                                    cnt++;
                                    sum = __fadd_rn(sum, s_conf[j][tid]);
                                    m |= 1u << j;
                                }
                            }
                        if (cnt > best_cnt || (cnt == best_cnt && sum > best_sum)) {
                            best_cnt = cnt;
                            best_sum = sum;
                            best_mask = m;
                        }
                    }
                }
            }
            if (best_cnt < 2) {
                failed = true;
                active = false;
            } else {
                mask = best_mask;
            }
        }
    }
    if (failed) {
        mask = 0;
#pragma unroll
        for (int k = 0; k < 3; k++) xyz[k] = qnan;
#pragma unroll
        for (int j = 0; j < NV; j++) err[j] = qnan;
    }
    out[3 * p + 0] = xyz[0];
    out[3 * p + 1] = xyz[1];
    out[3 * p + 2] = xyz[2];
    out_mask[p] = (uint8_t)mask;
    if (out_err) {
#pragma unroll
        for (int j = 0; j < NV; j++) out_err[p * NV + j] = err[j];
    }
}

}  // namespace

extern "C" int mvp_triangulate_robust(const float* kpts, int64_t n_points, int V, const double* cams, int n_cams,
                                      const int* cam_idx, int n_cam_idx, float inlier_px, float min_conf,
                                      float* out_xyz, uint8_t* out_mask, float* out_err, void* stream) {
    MVP_ABI_BEGIN
    const char* fn = "mvp_triangulate_robust";
    const CamIdx ci = tri_parse_args(fn, n_points, V, n_cams, cam_idx, n_cam_idx);
    MVP_REQUIRE(std::isfinite(inlier_px) && inlier_px > 0.f, "mvp_triangulate_robust: inlier_px=%g (finite, > 0)",
                (double)inlier_px);
    MVP_REQUIRE(!std::isnan(min_conf), "mvp_triangulate_robust: min_conf is NaN");
    if (n_points == 0) return MVP_OK;
    MVP_REQUIRE(kpts && cams && out_xyz && out_mask, "mvp_triangulate_robust: null device pointer");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(tri_grid(fn, n_points)), block(kBlock);
    tri_dispatch_views(n_cam_idx, [&](auto nv) {
        hipLaunchKernelGGL((triangulate_robust_kernel<decltype(nv)::value>), grid, block, 0, s, kpts, n_points, V, cams,
                           n_cams, ci, inlier_px, min_conf, out_xyz, out_mask, out_err);
    });
    MVP_HIP(hipGetLastError());
    MVP_ABI_END
}
