// mvp_triangulate_refine: maximum-likelihood refinement of triangulated points with a 3D covariance
// (shared device code in tri_common.h; map of the triangulation files in triangulate.hip).
#pragma clang fp contract(off)

#include "refine_common.h"

namespace {

// ----------------------------------------------------------------- maximum-likelihood refinement
// mvp_triangulate_refine: Levenberg-Marquardt on the weighted reprojection error through the full
// distortion model, from any triangulator's seed; the inverse Gauss-Newton Hessian is the point's
// covariance (no reference counterpart; algorithm in mvpose.h).  Per lane, fp64, FMA contraction on
// (no bit contract here):
//   * the used views' observation (2) and weight (3 numbers) are parked in LDS, [view][lane]
//     (bank-conflict free), as the robust kernel parks its views: the trial loop walks the views
//     in a rolled loop, which a per-lane register array cannot serve without going to scratch
//     (unrolled, the compiler hoists every view's camera record out of the trial loop: 256 VGPRs
//     + 150 AGPRs at NV = 8);
//   * the camera records are read through wave-uniform addresses straight from the parameter block
//     (scalar loads, one view's record at a time);
//   * ONE copy of the cost / gradient / Hessian evaluation inside the trial loop (trip 0 evaluates
//     the seed); accept / reject is selects, and the loop is left on a wave ballot once every lane
//     has converged, failed or used up max_iter — the pattern of triangulate_tol2_kernel.
//   (The observation rule, the forward model and the 3x3 Cholesky: refine_common.h, shared.)

template <int NV>
__global__ __launch_bounds__(kBlock) void triangulate_refine_kernel(
    ReprojObs o, ViewList vl, const double* __restrict__ cams, const float* __restrict__ xyz0, int max_iter, double tol,
    float* __restrict__ out_xyz, float* __restrict__ out_cov, float* __restrict__ out_cost,
    uint8_t* __restrict__ out_status) {
#pragma clang fp contract(fast)
    __shared__ double s_zx[NV][kBlock], s_zy[NV][kBlock], s_wxx[NV][kBlock], s_wxy[NV][kBlock], s_wyy[NV][kBlock];
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= o.n) return;
    const int tid = threadIdx.x;
    const unsigned allowed = reproj_allowed(o, p);
    int64_t gt;
    int gj;
    reproj_frame_joint(o, p, gt, gj);
    unsigned used = 0;
#pragma unroll
    for (int j = 0; j < NV; j++) {
        double ox, oy, a, b, d;
        const bool ok = reproj_observe(o, p, gt, gj, vl.col(j), (allowed >> j) & 1u, ox, oy, a, b, d);
        used |= (ok ? 1u : 0u) << j;
        s_zx[j][tid] = ok ? ox : 0.0;
        s_zy[j][tid] = ok ? oy : 0.0;
        s_wxx[j][tid] = ok ? a : 0.0;
        s_wxy[j][tid] = ok ? b : 0.0;
        s_wyy[j][tid] = ok ? d : 0.0;
    }
    const float s0 = xyz0[3 * p + 0], s1 = xyz0[3 * p + 1], s2 = xyz0[3 * p + 2];
    const double dinf = (double)INFINITY;
    bool alive = __popc(used) >= 2 && isfinite(s0) && isfinite(s1) && isfinite(s2);
    bool failed = !alive, conv = false, conv_step = false;
    double X[3] = {(double)s0, (double)s1, (double)s2};
    double delta[3] = {0.0, 0.0, 0.0};
    double f = dinf, g[3] = {0, 0, 0}, H[6] = {0, 0, 0, 0, 0, 0};
    double lambda = 1e-3;
    int trials = 0;
#pragma unroll 1
    for (int it = 0;; it++) {
        // trip 0: the seed itself (delta = 0); trip it > 0: trial `it`
        const double Xn[3] = {X[0] + delta[0], X[1] + delta[1], X[2] + delta[2]};
        double fn = 0, gn[3] = {0, 0, 0}, Hn[6] = {0, 0, 0, 0, 0, 0};
        bool front = true;
#pragma unroll 1
        for (int j = 0; j < NV; j++) {
            const RefineCam c = refine_cam(cams + vl.col(j) * MVP_CAM_DOUBLES);
            double fj = 0, gj3[3] = {0, 0, 0}, Hj[6] = {0, 0, 0, 0, 0, 0};
            const bool infront = refine_view_terms(c, Xn, s_zx[j][tid], s_zy[j][tid], s_wxx[j][tid], s_wxy[j][tid],
                                                   s_wyy[j][tid], fj, gj3, Hj);
            const bool u = (used >> j) & 1u;
            front = front && (infront || !u);
            const bool add = u && infront;
            fn += add ? fj : 0.0;
#pragma unroll
            for (int k = 0; k < 3; k++) gn[k] += add ? gj3[k] : 0.0;
#pragma unroll
            for (int k = 0; k < 6; k++) Hn[k] += add ? Hj[k] : 0.0;
        }
        fn = front ? fn : dinf;
        const bool fin = isfinite(fn);
        bool accept;
        if (it == 0) {
            failed = failed || !fin;
            alive = alive && fin;
            accept = alive;
        } else {
            accept = alive && fin && fn <= f;
            lambda = !alive ? lambda : (accept ? fmax(lambda * 0.1, 1e-12) : lambda * 10.0);
            trials += alive ? 1 : 0;
            conv = conv || (alive && conv_step);
        }
        f = accept ? fn : f;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            X[k] = accept ? Xn[k] : X[k];
            g[k] = accept ? gn[k] : g[k];
        }
#pragma unroll
        for (int k = 0; k < 6; k++) H[k] = accept ? Hn[k] : H[k];
        alive = alive && !conv;
        if (it >= max_iter) break;
        if (__ballot(alive) == 0) break;
        // propose: (H + lambda·diag H) delta = -g
        const double damp = 1.0 + lambda;
        const double A[6] = {H[0] * damp, H[1], H[2], H[3] * damp, H[4], H[5] * damp};
        const double mg[3] = {-g[0], -g[1], -g[2]};
        double L[6];
        const bool pd = chol3(A, L);
        chol3_solve(L, mg, delta);
        failed = failed || (alive && !pd);
        alive = alive && pd;
#pragma unroll
        for (int k = 0; k < 3; k++) delta[k] = alive ? delta[k] : 0.0;
        const double dn = sqrt(delta[0] * delta[0] + delta[1] * delta[1] + delta[2] * delta[2]);
        const double xn = sqrt(X[0] * X[0] + X[1] * X[1] + X[2] * X[2]);
        conv_step = dn <= tol * (xn + tol);
    }
    const float qnan = __builtin_nanf("");
    float cov[6] = {qnan, qnan, qnan, qnan, qnan, qnan};
    if (!failed) {
        double L[6];
        if (chol3(H, L)) {
            // columns of H⁻¹
            const double e0[3] = {1, 0, 0}, e1[3] = {0, 1, 0}, e2[3] = {0, 0, 1};
            double c0[3], c1[3], c2[3];
            chol3_solve(L, e0, c0);
            chol3_solve(L, e1, c1);
            chol3_solve(L, e2, c2);
            cov[0] = (float)c0[0], cov[1] = (float)c0[1], cov[2] = (float)c0[2];
            cov[3] = (float)c1[1], cov[4] = (float)c1[2], cov[5] = (float)c2[2];
        }
    }
    out_xyz[3 * p + 0] = failed ? s0 : (float)X[0];
    out_xyz[3 * p + 1] = failed ? s1 : (float)X[1];
    out_xyz[3 * p + 2] = failed ? s2 : (float)X[2];
    if (out_cov) {
#pragma unroll
        for (int k = 0; k < 6; k++) out_cov[6 * p + k] = cov[k];
    }
    if (out_cost) out_cost[p] = failed ? qnan : (float)f;
    if (out_status) out_status[p] = failed ? (uint8_t)0x80 : (uint8_t)(trials | (conv ? 0 : 0x40));
}

}  // namespace

extern "C" int mvp_triangulate_refine(const float* kpts, int64_t n_points, int V, const double* cams, int n_cams,
                                      const int* cam_idx, int n_cam_idx, const float* xyz0, const uint8_t* mask,
                                      int weights, const double* gauss, int J, float min_conf, float cov_floor,
                                      int max_iter, double tol, float* out_xyz, float* out_cov, float* out_cost,
                                      uint8_t* out_status, void* stream) {
    MVP_ABI_BEGIN
    const char* fn = "mvp_triangulate_refine";
    const CamIdx ci = tri_parse_args(fn, n_points, V, n_cams, cam_idx, n_cam_idx);
    const ReprojObs o = reproj_parse_obs(fn, kpts, n_points, V, mask, weights, gauss, J, min_conf, cov_floor, 0.0);
    MVP_REQUIRE(max_iter >= 0 && max_iter <= 63, "%s: max_iter=%d (0..63)", fn, max_iter);
    MVP_REQUIRE(std::isfinite(tol) && tol > 0, "%s: tol=%g (finite, > 0)", fn, tol);
    if (n_points == 0) return MVP_OK;
    MVP_REQUIRE(kpts && cams && xyz0 && out_xyz, "%s: null device pointer", fn);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(tri_grid(fn, n_points)), block(kBlock);
    tri_dispatch_views(n_cam_idx, [&](auto nv) {
        hipLaunchKernelGGL((triangulate_refine_kernel<decltype(nv)::value>), grid, block, 0, s, o, view_list(ci, n_cam_idx),
                           cams, xyz0, max_iter, tol, out_xyz, out_cov, out_cost, out_status);
    });
    MVP_HIP(hipGetLastError());
    MVP_ABI_END
}
