// Shared device code of the reprojection-error solvers: the maximum-likelihood point refinement
// (triangulate_refine.hip) and the bundle adjustment of the extrinsics (bundle_adjust.hip).  Both
// score raw, distorted pixels against the full forward model of include/mvpose.h, with the same
// rule for which view is used and what its observation and weight are.
#pragma once
#pragma clang fp contract(off)

#include "tri_common.h"

namespace {

struct RefineCam {  // what one view's forward model reads of a camera record
    double fx, skew, cx, fy, cy, k1, k2, p1, p2, k3, R[9], T[3];
};

__device__ __forceinline__ RefineCam refine_cam(const double* __restrict__ c) {
    RefineCam r;
    r.fx = c[0], r.skew = c[1], r.cx = c[2], r.fy = c[4], r.cy = c[5];
    r.k1 = c[9], r.k2 = c[10], r.p1 = c[11], r.p2 = c[12], r.k3 = c[13];
#pragma unroll
    for (int k = 0; k < 9; k++) r.R[k] = c[14 + k];
#pragma unroll
    for (int k = 0; k < 3; k++) r.T[k] = c[23 + k];
    return r;
}

// Whether view `col` of the point whose keypoints start at kp is used (`allowed`: its bit of the
// caller's mask), with its observation (ox, oy) and weight [[a, b], [b, d]] — the rule of
// mvp_triangulate_refine (mvpose.h).  gt, gj: the point's frame and joint, read with
// MVP_REFINE_W_GAUSS only.  Not used: the outputs are whatever the arithmetic gave; the caller
// selects them away.
__device__ __forceinline__ bool refine_observation(const float* __restrict__ kp, int V, int col, bool allowed,
                                                   int weights, const double* __restrict__ gauss, int64_t gt, int gj,
                                                   int J, float min_conf, float cov_floor, double& ox, double& oy,
                                                   double& a, double& b, double& d) {
    const float x = kp[col], y = kp[V + col], c = kp[2 * V + col];
    bool ok = allowed && view_usable(x, y, c, min_conf);
    ox = (double)x, oy = (double)y, a = 1.0, b = 0.0, d = 1.0;
    if (weights == MVP_REFINE_W_CONF) {
        a = d = (double)c;
    } else if (weights == MVP_REFINE_W_GAUSS) {
        const double* __restrict__ gq = gauss + ((gt * V + col) * (int64_t)J + gj) * 6;
        const double g0 = gq[0], g1 = gq[1], g2 = gq[2], g3 = gq[3], g4 = gq[4], g5 = gq[5];
        const bool fin = isfinite(g0) && isfinite(g1) && isfinite(g2) && isfinite(g3) && isfinite(g4) && isfinite(g5);
        const bool zero = g0 == 0 && g1 == 0 && g2 == 0 && g3 == 0 && g4 == 0 && g5 == 0;
        const double sa = g2 + (double)cov_floor, sb = g3, sd = g5 + (double)cov_floor;
        const double det = sa * sd - sb * sb;
        ok = ok && fin && !zero && sa > 0 && det > 0;
        const double idet = 1.0 / det;
        ox = g0, oy = g1;
        a = sd * idet, b = -sb * idet, d = sa * idet;
    }
    return ok;
}

// One view's forward model at X: the camera-frame point P, 1/P_z, the normalised (x, y), the pixel
// (u, v) and A = d pixel / d(x, y) (a00 a01; a10 a11).  Branch-free; P_z <= 0 gives Inf / NaN that
// the caller drops.
struct RefineFwd {
    double Px, Py, Pz, iz, x, y, u, v, a00, a01, a10, a11;
};

__device__ __forceinline__ RefineFwd refine_forward(const RefineCam& c, const double (&X)[3]) {
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

// refine_view_terms with a Huber loss on the whitened residual s = sqrt(rᵀ·W·r), the rho and the
// IRLS weight omega of mvp_bundle_adjust (hub <= 0: off): rho and s² are added to their sums, and
// with JAC g += Jᵀ·W̃·r, H += Jᵀ·W̃·J, W̃ = omega·W.  Branch-free; false when the point is not in
// front of the camera.
template <bool JAC>
__device__ __forceinline__ bool refine_view_terms_huber(const RefineCam& c, const double (&X)[3], double zx, double zy,
                                                        double wxx, double wxy, double wyy, double hub, double& rho,
                                                        double& s2sum, double (&g)[3], double (&H)[6]) {
#pragma clang fp contract(fast)
    const RefineFwd w = refine_forward(c, X);
    const double r0 = w.u - zx;
    const double r1 = w.v - zy;
    const double s2 = r0 * (wxx * r0 + wxy * r1) + r1 * (wxy * r0 + wyy * r1);
    const double s = sqrt(s2);
    const bool quad = !(hub > 0) || !(s > hub);
    const double om = quad ? 1.0 : hub / s;
    rho += quad ? 0.5 * s2 : hub * (s - 0.5 * hub);
    s2sum += s2;
    if (JAC) {
        const double oxx = om * wxx, oxy = om * wxy, oyy = om * wyy;
        double J0[3], J1[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double m0 = (c.R[k] - w.x * c.R[6 + k]) * w.iz;  // d x / d X_k
            const double m1 = (c.R[3 + k] - w.y * c.R[6 + k]) * w.iz;
            J0[k] = w.a00 * m0 + w.a01 * m1;
            J1[k] = w.a10 * m0 + w.a11 * m1;
        }
        const double wr0 = oxx * r0 + oxy * r1, wr1 = oxy * r0 + oyy * r1;
        double wj0[3], wj1[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            wj0[k] = oxx * J0[k] + oxy * J1[k];
            wj1[k] = oxy * J0[k] + oyy * J1[k];
            g[k] += J0[k] * wr0 + J1[k] * wr1;
        }
        H[0] += J0[0] * wj0[0] + J1[0] * wj1[0];
        H[1] += J0[0] * wj0[1] + J1[0] * wj1[1];
        H[2] += J0[0] * wj0[2] + J1[0] * wj1[2];
        H[3] += J0[1] * wj0[1] + J1[1] * wj1[1];
        H[4] += J0[1] * wj0[2] + J1[1] * wj1[2];
        H[5] += J0[2] * wj0[2] + J1[2] * wj1[2];
    }
    return w.Pz > 0;
}

// Cholesky A = L·Lᵀ of the symmetric 3x3 (xx, xy, xz, yy, yz, zz); false on a non-positive (or
// NaN) pivot.  L: l00, l10, l20, l11, l21, l22.
__device__ __forceinline__ bool chol3(const double (&A)[6], double (&L)[6]) {
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
__device__ __forceinline__ void chol3_solve(const double (&L)[6], const double (&b)[3], double (&x)[3]) {
#pragma clang fp contract(fast)
    const double y0 = b[0] / L[0];
    const double y1 = (b[1] - L[1] * y0) / L[3];
    const double y2 = (b[2] - L[2] * y0 - L[4] * y1) / L[5];
    x[2] = y2 / L[5];
    x[1] = (y1 - L[4] * x[2]) / L[3];
    x[0] = (y0 - L[1] * x[1] - L[2] * x[2]) / L[0];
}

}  // namespace
