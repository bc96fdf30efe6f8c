// The one observation and view model of the reprojection-error solvers: the maximum-likelihood
// point refinement (triangulate_refine.hip), the bundle adjustment of the extrinsics
// (bundle_adjust.hip) and the trajectory and skeleton fits (trajectory_fit_terms.h).  All of them
// score raw, distorted pixels against the full forward model of include/mvpose.h, with the same
// rule for which view is used and what its observation and weight are.  Sections: the observation,
// the view model, the 3x3 Cholesky; the last two compile for the host too (tools/reproj_host_check.cpp).
#pragma once
#pragma clang fp contract(off)

#include "tri_common.h"

namespace {

struct RefineCam {  // what one view's forward model reads of a camera record
    double fx, skew, cx, fy, cy, k1, k2, p1, p2, k3, R[9], T[3];
};

__host__ __device__ __forceinline__ RefineCam refine_cam(const double* __restrict__ c) {
    RefineCam r;
    r.fx = c[0], r.skew = c[1], r.cx = c[2], r.fy = c[4], r.cy = c[5];
    r.k1 = c[9], r.k2 = c[10], r.p1 = c[11], r.p2 = c[12], r.k3 = c[13];
#pragma unroll
    for (int k = 0; k < 9; k++) r.R[k] = c[14 + k];
#pragma unroll
    for (int k = 0; k < 3; k++) r.T[k] = c[23 + k];
    return r;
}

// ------------------------------------------------------------------------------- the observation
// What a kernel reads of the caller's observations.  Point e's frame and joint are e / stride and
// e % stride: the refinement and the bundle adjustment pass J, the fits P.  reproj_allowed: bit j
// says whether the caller's mask allows view j of point e.
struct ReprojObs {
    const float* kpts;      // [n][3][V]
    const uint8_t* mask;    // [n] or null
    const double* gauss;    // [n / stride][V][stride][6] or null
    int64_t n;
    int V, stride, weights;
    float min_conf, cov_floor;
    double hub;             // Huber delta on the whitened residual; <= 0: off
};

// The listed cameras (each < kMaxCams = 8) as nibbles of one scalar: a rolled view loop's index.
struct ViewList {
    unsigned cols;
    int nv;
    __host__ __device__ __forceinline__ int col(int j) const { return (int)((cols >> (4 * j)) & 15u); }
};

inline ViewList view_list(const CamIdx& ci, int nv) {
    ViewList vl{0u, nv};
    for (int j = 0; j < nv; j++) vl.cols |= (unsigned)ci.v[j] << (4 * j);
    return vl;
}

__device__ __forceinline__ unsigned reproj_allowed(const ReprojObs& o, int64_t e) {
    return o.mask ? (unsigned)o.mask[e] : 0xFFu;
}

// Point e's frame and joint, read with MVP_REFINE_W_GAUSS only (else 0, and no division); the
// second reproj_observe below is for a caller that has only e.
__device__ __forceinline__ void reproj_frame_joint(const ReprojObs& o, int64_t e, int64_t& gt, int& gj) {
    const bool gs = o.weights == MVP_REFINE_W_GAUSS;
    gt = gs ? e / o.stride : 0;
    gj = gs ? (int)(e % o.stride) : 0;
}

// Whether view `col` of point e = gt·stride + gj is used (`allowed`: its bit of the caller's mask),
// with its observation (ox, oy) and weight [[a, b], [b, d]] — the rule of mvp_triangulate_refine
// (mvpose.h).  Not used: the outputs are whatever the arithmetic gave; the caller selects them away.
__device__ __forceinline__ bool reproj_observe(const ReprojObs& o, int64_t e, int64_t gt, int gj, int col, bool allowed,
                                               double& ox, double& oy, double& a, double& b, double& d) {
    const float* __restrict__ kp = o.kpts + e * 3 * o.V;
    const float x = kp[col], y = kp[o.V + col], c = kp[2 * o.V + col];
    bool ok = allowed && view_usable(x, y, c, o.min_conf);
    ox = (double)x, oy = (double)y, a = 1.0, b = 0.0, d = 1.0;
    if (o.weights == MVP_REFINE_W_CONF) {
        a = d = (double)c;
    } else if (o.weights == MVP_REFINE_W_GAUSS) {
        const double* __restrict__ gq = o.gauss + ((gt * o.V + col) * (int64_t)o.stride + gj) * 6;
        const double g0 = gq[0], g1 = gq[1], g2 = gq[2], g3 = gq[3], g4 = gq[4], g5 = gq[5];
        const bool fin = isfinite(g0) && isfinite(g1) && isfinite(g2) && isfinite(g3) && isfinite(g4) && isfinite(g5);
        const bool zero = g0 == 0 && g1 == 0 && g2 == 0 && g3 == 0 && g4 == 0 && g5 == 0;
        const double sa = g2 + (double)o.cov_floor, sb = g3, sd = g5 + (double)o.cov_floor;
        const double det = sa * sd - sb * sb;
        ok = ok && fin && !zero && sa > 0 && det > 0;
        const double idet = 1.0 / det;
        ox = g0, oy = g1;
        a = sd * idet, b = -sb * idet, d = sa * idet;
    }
    return ok;
}

__device__ __forceinline__ bool reproj_observe(const ReprojObs& o, int64_t e, int col, bool allowed, double& ox,
                                               double& oy, double& a, double& b, double& d) {
    int64_t gt;
    int gj;
    reproj_frame_joint(o, e, gt, gj);
    return reproj_observe(o, e, gt, gj, col, allowed, ox, oy, a, b, d);
}

// The observation arguments' checks, after tri_parse_args; `fn`, the entry point's name, prefixes
// each message.  An entry point without a Huber loss passes huber_delta = 0.
inline ReprojObs reproj_parse_obs(const char* fn, const float* kpts, int64_t n, int V, const uint8_t* mask, int weights,
                                  const double* gauss, int stride, float min_conf, float cov_floor,
                                  double huber_delta) {
    MVP_REQUIRE(weights >= MVP_REFINE_W_UNIT && weights <= MVP_REFINE_W_GAUSS, "%s: weights=%d (0..2)", fn, weights);
    if (weights == MVP_REFINE_W_GAUSS) {
        MVP_REQUIRE(gauss != nullptr, "%s: MVP_REFINE_W_GAUSS needs gauss_dev", fn);
        MVP_REQUIRE(stride > 0 && n % stride == 0, "%s: J=%d (> 0, dividing n_points=%lld)", fn, stride, (long long)n);
    }
    MVP_REQUIRE(!std::isnan(min_conf), "%s: min_conf is NaN", fn);
    MVP_REQUIRE(cov_floor >= 0.f, "%s: cov_floor=%g (not NaN, >= 0)", fn, (double)cov_floor);
    MVP_REQUIRE(!std::isnan(huber_delta), "%s: huber_delta is NaN", fn);
    return ReprojObs{kpts, mask, gauss, n, V, stride, weights, min_conf, cov_floor, huber_delta > 0 ? huber_delta : 0.0};
}

// ------------------------------------------------------------------------------- the view model
// One view's forward model at X: the camera-frame point P, 1/P_z, the normalised (x, y), the pixel
// (u, v) and A = d pixel / d(x, y) (a00 a01; a10 a11).  Branch-free; P_z <= 0 gives Inf / NaN that
// the caller drops.
struct RefineFwd {
    double Px, Py, Pz, iz, x, y, u, v, a00, a01, a10, a11;
};

__host__ __device__ __forceinline__ RefineFwd refine_forward(const RefineCam& c, const double (&X)[3]) {
#pragma clang fp contract(fast)
    RefineFwd w;
    w.Px = c.R[0] * X[0] + c.R[1] * X[1] + c.R[2] * X[2] + c.T[0];
    w.Py = c.R[3] * X[0] + c.R[4] * X[1] + c.R[5] * X[2] + c.T[1];
    w.Pz = c.R[6] * X[0] + c.R[7] * X[1] + c.R[8] * X[2] + c.T[2];
    w.iz = 1.0 / w.Pz;
    const double x = w.Px * w.iz, y = w.Py * w.iz;
    w.x = x, w.y = y;
    const double r2 = x * x + y * y;
    const double radial = 1 + r2 * (c.k1 + r2 * (c.k2 + r2 * c.k3));
    const double drad = c.k1 + r2 * (2 * c.k2 + 3 * c.k3 * r2);  // d radial / d r2
    const double xd = x * radial + 2 * c.p1 * x * y + c.p2 * (r2 + 2 * x * x);
    const double yd = y * radial + c.p1 * (r2 + 2 * y * y) + 2 * c.p2 * x * y;
    w.u = c.fx * xd + c.skew * yd + c.cx;
    w.v = c.fy * yd + c.cy;
    // d(xd, yd) / d(x, y): symmetric off-diagonal
    const double dxx = radial + 2 * x * x * drad + 2 * c.p1 * y + 6 * c.p2 * x;
    const double dxy = 2 * x * y * drad + 2 * c.p1 * x + 2 * c.p2 * y;
    const double dyy = radial + 2 * y * y * drad + 6 * c.p1 * y + 2 * c.p2 * x;
    w.a00 = c.fx * dxx + c.skew * dxy, w.a01 = c.fx * dxy + c.skew * dyy;
    w.a10 = c.fy * dxy, w.a11 = c.fy * dyy;
    return w;
}

// One view's term of f, g (3) and H (xx, xy, xz, yy, yz, zz) at X, branch-free; false when the
// point is not in front of the camera (the caller then drops the terms, which may be Inf / NaN).
// The refinement kernel's own statements: through reproj_view and reproj_add_normal W·r fuses its
// other product, a last-place change that float32 outputs hide from a hash but that decides a
// rank-deficient H's last pivot (test_pipeline_refine_outputs).
__device__ __forceinline__ bool refine_view_terms(const RefineCam& c, const double (&X)[3], double zx, double zy,
                                                  double wxx, double wxy, double wyy, double& f, double (&g)[3],
                                                  double (&H)[6]) {
#pragma clang fp contract(fast)
    const RefineFwd w = refine_forward(c, X);
    const double r0 = w.u - zx;
    const double r1 = w.v - zy;
    double J0[3], J1[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double m0 = (c.R[k] - w.x * c.R[6 + k]) * w.iz;  // d x / d X_k
        const double m1 = (c.R[3 + k] - w.y * c.R[6 + k]) * w.iz;
        J0[k] = w.a00 * m0 + w.a01 * m1;
        J1[k] = w.a10 * m0 + w.a11 * m1;
    }
    const double wr0 = wxx * r0 + wxy * r1, wr1 = wxy * r0 + wyy * r1;
    f += 0.5 * (r0 * wr0 + r1 * wr1);
    double wj0[3], wj1[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        wj0[k] = wxx * J0[k] + wxy * J1[k];
        wj1[k] = wxy * J0[k] + wyy * J1[k];
        g[k] += J0[k] * wr0 + J1[k] * wr1;
    }
    H[0] += J0[0] * wj0[0] + J1[0] * wj1[0];
    H[1] += J0[0] * wj0[1] + J1[0] * wj1[1];
    H[2] += J0[0] * wj0[2] + J1[0] * wj1[2];
    H[3] += J0[1] * wj0[1] + J1[1] * wj1[1];
    H[4] += J0[1] * wj0[2] + J1[1] * wj1[2];
    H[5] += J0[2] * wj0[2] + J1[2] * wj1[2];
    return w.Pz > 0;
}

// One view at X against the observation (zx, zy) of weight W = [[wxx, wxy], [wxy, wyy]]: the forward
// model, the residual r, s² = rᵀ·W·r, front = P_z > 0, and under mvp_bundle_adjust's Huber loss on the
// whitened residual s (hub <= 0: off) its value rho and W̃ = omega·W, omega the IRLS weight.  Branch-free.
struct ReprojView {
    RefineFwd w;
    double r0, r1, s2, rho, w00, w01, w11;
    bool front;
};

__host__ __device__ __forceinline__ ReprojView reproj_view(const RefineCam& c, const double (&X)[3], double zx,
                                                           double zy, double wxx, double wxy, double wyy, double hub) {
#pragma clang fp contract(fast)
    ReprojView v;
    v.w = refine_forward(c, X);
    v.front = v.w.Pz > 0;
    v.r0 = v.w.u - zx;
    v.r1 = v.w.v - zy;
    v.s2 = v.r0 * (wxx * v.r0 + wxy * v.r1) + v.r1 * (wxy * v.r0 + wyy * v.r1);
    const double s = sqrt(v.s2);
    const bool quad = !(hub > 0) || !(s > hub);
    const double om = quad ? 1.0 : hub / s;
    v.rho = quad ? 0.5 * v.s2 : hub * (s - 0.5 * hub);
    v.w00 = om * wxx, v.w01 = om * wxy, v.w11 = om * wyy;
    return v;
}

// J_X = d pixel / dX has two forms, equal in exact arithmetic and different in rounding.  Each
// solver's output bits depend on its own, so both stay; do not convert a solver to the other's.
// The refinement's and the fits': m = d(x, y) / dX_k = (R_k − x·R_{6+k})·iz, then A·m.
__host__ __device__ __forceinline__ void reproj_jx(const RefineCam& c, const RefineFwd& w, double (&J0)[3],
                                                   double (&J1)[3]) {
#pragma clang fp contract(fast)
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double m0 = (c.R[k] - w.x * c.R[6 + k]) * w.iz;  // d x / d X_k
        const double m1 = (c.R[3 + k] - w.y * c.R[6 + k]) * w.iz;
        J0[k] = w.a00 * m0 + w.a01 * m1;
        J1[k] = w.a10 * m0 + w.a11 * m1;
    }
}

// The bundle adjustment's: p = d pixel / dP = A·[[iz, 0, −x·iz], [0, iz, −y·iz]], then p·R; p also
// gives J_c = p·[−[P−T]×, I], the view's rotation (3) and translation (3).
__host__ __device__ __forceinline__ void reproj_jx_jc(const RefineCam& c, const RefineFwd& w, double (&jx0)[3],
                                                      double (&jx1)[3], double (&jc0)[6], double (&jc1)[6]) {
#pragma clang fp contract(fast)
    const double p00 = w.a00 * w.iz, p01 = w.a01 * w.iz, p02 = -(w.a00 * w.x + w.a01 * w.y) * w.iz;
    const double p10 = w.a10 * w.iz, p11 = w.a11 * w.iz, p12 = -(w.a10 * w.x + w.a11 * w.y) * w.iz;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        jx0[k] = p00 * c.R[k] + p01 * c.R[3 + k] + p02 * c.R[6 + k];
        jx1[k] = p10 * c.R[k] + p11 * c.R[3 + k] + p12 * c.R[6 + k];
    }
    const double qx = w.Px - c.T[0], qy = w.Py - c.T[1], qz = w.Pz - c.T[2];
    jc0[0] = p02 * qy - p01 * qz, jc0[1] = p00 * qz - p02 * qx, jc0[2] = p01 * qx - p00 * qy;
    jc1[0] = p12 * qy - p11 * qz, jc1[1] = p10 * qz - p12 * qx, jc1[2] = p11 * qx - p10 * qy;
    jc0[3] = p00, jc0[4] = p01, jc0[5] = p02;
    jc1[3] = p10, jc1[4] = p11, jc1[5] = p12;
}

// Where u: g += Jᵀ·W̃·r and H (xx, xy, xz, yy, yz, zz) += Jᵀ·W̃·J; else both += 0.  Which product of
// each a·b + c·d the compiler's contraction fuses changes with the code around it, and with it the
// output bits: so the fused multiply-adds are written out, as the fits and the bundle adjustment
// have always rounded.  Terms before selects: as branches ba_linearise_kernel takes 12 more VGPRs.
__host__ __device__ __forceinline__ void reproj_add_normal(const double (&J0)[3], const double (&J1)[3], double w00,
                                                           double w01, double w11, double r0, double r1, bool u,
                                                           double (&g)[3], double (&H)[6]) {
    const double wr0 = __builtin_fma(w00, r0, w01 * r1), wr1 = __builtin_fma(w01, r0, w11 * r1);
    double wj0[3], wj1[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        wj0[k] = __builtin_fma(w00, J0[k], w01 * J1[k]);
        wj1[k] = __builtin_fma(w01, J0[k], w11 * J1[k]);
        const double gk = __builtin_fma(J0[k], wr0, J1[k] * wr1);
        g[k] += u ? gk : 0.0;
    }
    int k = 0;
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = a; b < 3; b++, k++) {
            const double h = __builtin_fma(J1[a], wj1[b], J0[a] * wj0[b]);
            H[k] += u ? h : 0.0;
        }
}

// One view's term of rho and Σ s², added to their sums, and with JAC g += Jᵀ·W̃·r (3),
// H += Jᵀ·W̃·J at X, by reproj_view, reproj_jx and reproj_add_normal (the fits); branch-free; false
// when the point is not in front of the camera (the caller then drops the terms, which may be
// Inf / NaN).
template <bool JAC>
__host__ __device__ __forceinline__ bool refine_view_terms_huber(const RefineCam& c, const double (&X)[3], double zx,
                                                                 double zy, double wxx, double wxy, double wyy,
                                                                 double hub, double& rho, double& s2sum,
                                                                 double (&g)[3], double (&H)[6]) {
#pragma clang fp contract(fast)
    const ReprojView v = reproj_view(c, X, zx, zy, wxx, wxy, wyy, hub);
    rho += v.rho;
    s2sum += v.s2;
    if (JAC) {
        double J0[3], J1[3];
        reproj_jx(c, v.w, J0, J1);
        reproj_add_normal(J0, J1, v.w00, v.w01, v.w11, v.r0, v.r1, true, g, H);
    }
    return v.front;
}

// ------------------------------------------------------------------------------- 3x3 Cholesky
// Cholesky A = L·Lᵀ of the symmetric 3x3 (xx, xy, xz, yy, yz, zz); false on a non-positive (or
// NaN) pivot.  L: l00, l10, l20, l11, l21, l22.
__host__ __device__ __forceinline__ bool chol3(const double (&A)[6], double (&L)[6]) {
#pragma clang fp contract(fast)
    const double d0 = A[0];
    L[0] = sqrt(d0);
    L[1] = A[1] / L[0];
    L[2] = A[2] / L[0];
    const double d1 = A[3] - L[1] * L[1];
    L[3] = sqrt(d1);
    L[4] = (A[4] - L[2] * L[1]) / L[3];
    const double d2 = A[5] - L[2] * L[2] - L[4] * L[4];
    L[5] = sqrt(d2);
    return (d0 > 0) && (d1 > 0) && (d2 > 0);
}

// x = A⁻¹ b from A's Cholesky factor.
__host__ __device__ __forceinline__ void chol3_solve(const double (&L)[6], const double (&b)[3], double (&x)[3]) {
#pragma clang fp contract(fast)
    const double y0 = b[0] / L[0];
    const double y1 = (b[1] - L[1] * y0) / L[3];
    const double y2 = (b[2] - L[2] * y0 - L[4] * y1) / L[5];
    x[2] = y2 / L[5];
    x[1] = (y1 - L[4] * x[2]) / L[3];
    x[0] = (y0 - L[1] * x[1] - L[2] * x[2]) / L[0];
}

}  // namespace
