// Shared pieces of the batched multi-view triangulation for gfx950 — one (frame, joint) problem
// per lane (triangulate.hip has the map of which file holds which solver).
//
// Replaces the reference's T*J Python-level calls of utils.triangulate_points
// (pose_estimation.py:27-53 -> utils.py:1277-1336), whose numerics live in
// OpenCV 4.9 (cv.undistortPoints, cv.triangulatePoints,
// cv.convertPointsFromHomogeneous).  Per lane, in fp64 with no FMA contraction
// so the rounding sequence is OpenCV's:
//   1. undistort each view's (x, y) with its own K/dist: 5 fixed iterations,
//      icdist<0 fallback, RR = K, rounded to f32 (cvUndistortPointsInternal);
//   2. A (2V x 4): rows x·P[2]-P[0], y·P[2]-P[1] per view (icvTriangulatePoints);
//   3. null vector = Vt row 3 of cv::SVD (JacobiSVDImpl_): by default computed by
//      Householder QR + inverse iteration to the fp64 noise floor (qr_inverse_iteration,
//      ~1/4 of the FP64 work), falling back per lane to the exact restatement —
//      one-sided Hestenes Jacobi on the rows of Aᵀ, eps = 10·DBL_EPSILON,
//      descending selection sort — when that iteration has not provably
//      converged; MVP_TRI_EXACT_JACOBI forces the restatement for every lane;
//   4. f32 homogeneous divide: s = w != 0 ? 1.f/w : 1.f (convertPointsFromHomogeneous).
// The reference's camera selection (top-2 by confidence, ascending; parameters
// keyed by selection position; pose_estimation.py:32-45) is reproduced in
// MVP_TRI_REFERENCE mode.
//
// Roofline: HBM-bound by design at 12·(V+1) B per point (read x,y,conf per view,
// write xyz) but FP64-issue-heavy (Jacobi ≈ 2-3 kFLOP/point); see DESIGN.md.
//
// Every translation unit that includes this header opens with the same pragma: the bit contract
// with OpenCV holds only without FMA contraction, and the functions that may contract say so
// themselves (contract(fast) in their body).
#pragma once
#pragma clang fp contract(off)

#include "mvp_common.h"

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <type_traits>

namespace {

constexpr int kMaxCams = 8;
constexpr int kBlock = 256;

struct CamIdx {
    int v[kMaxCams];
};

// cvUndistortPointsInternal (OpenCV 4.9), R = I, P = K, 5 iterations, 5 coefficients.
// The k4..k6 / thin-prism terms are zero and contribute exact zeros; they are
// omitted (sign-of-zero differences cannot change the result).  OpenCV computes in
// double and stores into the source's depth: undistort_point rounds to f32 (CV_32FC2
// keypoints, the pipeline), undistort_point_f64 keeps the double (CV_64FC2).
__device__ __forceinline__ void undistort_point_f64(double u, double v, const double* __restrict__ c,
                                                    double& ox, double& oy) {
    const double fx = c[0], fy = c[4];
    const double ifx = 1. / fx, ify = 1. / fy;
    const double cx = c[2], cy = c[5];
    const double k0 = c[9], k1 = c[10], k2 = c[11], k3 = c[12], k4 = c[13];
    double x = (u - cx) * ifx;
    double y = (v - cy) * ify;
    const double x0 = x, y0 = y;
#pragma unroll
    for (int j = 0; j < 5; j++) {
        double r2 = x * x + y * y;
        double icdist = 1. / (1 + ((k4 * r2 + k1) * r2 + k0) * r2);
        if (icdist < 0) {
            x = (u - cx) * ifx;
            y = (v - cy) * ify;
            break;
        }
        double deltaX = 2 * k2 * x * y + k3 * (r2 + 2 * x * x);
        double deltaY = k2 * (r2 + 2 * y * y) + 2 * k3 * x * y;
        x = (x0 - deltaX) * icdist;
        y = (y0 - deltaY) * icdist;
    }
    double xx = c[0] * x + c[1] * y + c[2];
    double yy = c[3] * x + c[4] * y + c[5];
    double ww = 1. / (c[6] * x + c[7] * y + c[8]);
    ox = xx * ww;
    oy = yy * ww;
}

__device__ __forceinline__ void undistort_point(float uf, float vf, const double* __restrict__ c,
                                                float& ox, float& oy) {
    double x, y;
    undistort_point_f64(uf, vf, c, x, y);
    ox = (float)x;
    oy = (float)y;
}

// Reciprocals and square roots built on v_rcp_f64 / v_rsq_f64.  They differ in the number of
// refinement steps, hence in accuracy: recip_rn is the IEEE division's bits (bit-exact paths may
// use it), rcp_nr is ~1 ulp, rcp_nr1 ~11 ulp; sqrt_fast and rsqrt_fast are ~1 ulp.  Only recip_rn
// may stand where OpenCV's rounding sequence is restated; the others serve the certified
// approximations, whose error bounds account for them.

// 1/b with the arithmetic of the compiler's IEEE fp64 division (v_div_scale,
// v_rcp_f64, two Newton steps, one quotient correction, v_div_fmas, v_div_fixup)
// minus the scale / fixup instructions, which are identities for finite, normal
// b away from the exponent limits: bit-identical there, 7 instructions not 11.
// Used for every reciprocal of the fast path; every b here is O(1) to O(1e6).
__device__ __forceinline__ double recip_rn(double b) {
    double r = __builtin_amdgcn_rcp(b);
    double e = __builtin_fma(-b, r, 1.0);
    r = __builtin_fma(r, e, r);
    e = __builtin_fma(-b, r, 1.0);
    r = __builtin_fma(r, e, r);
    e = __builtin_fma(-b, r, 1.0);
    return __builtin_fma(e, r, r);
}

// r = 1/b to ~1 ulp: v_rcp_f64 + two Newton steps (no IEEE-division scaling)
__device__ __forceinline__ double rcp_nr(double b) {
    double r = __builtin_amdgcn_rcp(b);
    double e = __builtin_fma(-b, r, 1.0);
    r = __builtin_fma(r, e, r);
    e = __builtin_fma(-b, r, 1.0);
    return __builtin_fma(r, e, r);
}

// r = 1/b to ~11 ulp: v_rcp_f64 (~2^-24) + one Newton step (profiles/r03p_rcp_probe.log).
// For the undistortion's fp64 steps: 11 ulp of fp64 is ~1e-15 relative, inside the bound's
// fp64 term.
__device__ __forceinline__ double rcp_nr1(double b) {
    const double r = __builtin_amdgcn_rcp(b);
    return __builtin_fma(r, __builtin_fma(-b, r, 1.0), r);
}

// sqrt(s) for s > 0 by v_rsq_f64 + two Goldschmidt steps + one residual
// correction (~1 ulp); the fast solver's norms only.
__device__ __forceinline__ double sqrt_fast(double s) {
    const double y = __builtin_amdgcn_rsq(s);
    double g = s * y, h = 0.5 * y;
    double r = __builtin_fma(-g, h, 0.5);
    g = __builtin_fma(g, r, g);
    h = __builtin_fma(h, r, h);
    r = __builtin_fma(-g, h, 0.5);
    g = __builtin_fma(g, r, g);
    h = __builtin_fma(h, r, h);
    const double d = __builtin_fma(-g, g, s);
    return s > 0 ? __builtin_fma(d, h, g) : 0.0;
}

// 1/sqrt(s), s > 0, to ~1 ulp: v_rsq_f64 + two Newton steps.
__device__ __forceinline__ double rsqrt_fast(double s) {
    double y = __builtin_amdgcn_rsq(s);
    double t = s * y;
    double e = __builtin_fma(-t, y, 1.0);
    y = __builtin_fma(0.5 * y, e, y);
    t = s * y;
    e = __builtin_fma(-t, y, 1.0);
    return __builtin_fma(0.5 * y, e, y);
}

// Per-camera constants of the fast undistortion, computed once per block with
// the same IEEE operations the per-point code would do (1./fx, 1./fy).
struct CamFast {
    double ifx, ify;
};

// undistort_point with the loop-invariant reciprocals from CamFast and every
// division as recip_rn; branch-free, so the two views of a point interleave.
// Same operation sequence and rounding as undistort_point for finite input.
__device__ __forceinline__ void undistort_point_fast(float uf, float vf, const double* __restrict__ c,
                                                     const CamFast& cf, float& ox, float& oy) {
    const double cx = c[2], cy = c[5];
    const double k0 = c[9], k1 = c[10], k2 = c[11], k3 = c[12], k4 = c[13];
    const double u = uf, v = vf;
    double x = (u - cx) * cf.ifx;
    double y = (v - cy) * cf.ify;
    const double x0 = x, y0 = y;
    bool neg = false;
#pragma unroll
    for (int j = 0; j < 5; j++) {
        double r2 = x * x + y * y;
        double icdist = recip_rn(1 + ((k4 * r2 + k1) * r2 + k0) * r2);
        neg = neg || (icdist < 0);
        double deltaX = 2 * k2 * x * y + k3 * (r2 + 2 * x * x);
        double deltaY = k2 * (r2 + 2 * y * y) + 2 * k3 * x * y;
        x = (x0 - deltaX) * icdist;
        y = (y0 - deltaY) * icdist;
    }
    // OpenCV breaks out with the initial guess on icdist < 0: the iterates after
    // such a step are discarded here instead — selects, not a branch, so both
    // views' chains stay in one basic block for the scheduler to interleave
    // (the branch form measured 0.081 vs 0.058 ms per 1.7 M points)
    x = neg ? x0 : x;
    y = neg ? y0 : y;
    double xx = c[0] * x + c[1] * y + c[2];
    double yy = c[3] * x + c[4] * y + c[5];
    const double ww = recip_rn(c[6] * x + c[7] * y + c[8]);
    ox = (float)(xx * ww);
    oy = (float)(yy * ww);
}

// std::hypot as OpenCV's JacobiSVDImpl_ gets it from libm on Linux: glibc 2.35's __ieee754_hypot
// (sysdeps/ieee754/dbl-64/e_hypot.c, the non-FMA kernel x86-64 builds; verified bit-identical to
// this image's libm on 5e7 random pairs, tests/test_oracle_triangulate.py).  The compiler's
// hypot (ocml) rounds differently in the last bit, which made ~60 % of the exact path's float64
// outputs differ from the restatement's in round 4.
__device__ __forceinline__ double hypot_kernel(double ax, double ay) {
    double h = sqrt(ax * ax + ay * ay);
    double t1, t2;
    if (h <= 2.0 * ay) {
        const double delta = h - ay;
        t1 = ax * (2.0 * delta - ax);
        t2 = (delta - 2.0 * (ax - ay)) * delta;
    } else {
        const double delta = h - ax;
        t1 = 2.0 * delta * (ax - 2.0 * ay);
        t2 = (4.0 * delta - ay) * ay + delta * delta;
    }
    h -= (t1 + t2) / (2.0 * h);
    return h;
}

__device__ __noinline__ double hypot_glibc(double x, double y) {
    if (!isfinite(x) || !isfinite(y)) {
        if (isinf(x) || isinf(y)) return INFINITY;
        return x + y;
    }
    x = fabs(x);
    y = fabs(y);
    const double ax = x < y ? y : x, ay = x < y ? x : y;
    if (ax > 0x1p+511) {
        if (ay <= ax * 0x1p-54) return ax + ay;
        return hypot_kernel(ax * 0x1p-600, ay * 0x1p-600) / 0x1p-600;
    }
    if (ay < 0x1p-511) {
        if (ax >= ay / 0x1p-54) return ax + ay;
        return hypot_kernel(ax / 0x1p-600, ay / 0x1p-600) * 0x1p-600;
    }
    if (ay <= ax * 0x1p-54) return ax + ay;
    return hypot_kernel(ax, ay);
}

// JacobiSVDImpl_<double> on At (4 rows of length M); returns Vt row of the
// smallest singular value after OpenCV's descending selection sort.
template <int M>
__device__ __forceinline__ void jacobi_null_vector(double (&At)[4][M], double (&nv)[4]) {
    double W[4];
    double Vt[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        double sd = 0;
#pragma unroll
        for (int k = 0; k < M; k++) sd += At[i][k] * At[i][k];
        W[i] = sd;
#pragma unroll
        for (int k = 0; k < 4; k++) Vt[i][k] = (i == k) ? 1.0 : 0.0;
    }
    const double eps = DBL_EPSILON * 10;
    const int max_iter = M > 30 ? M : 30;
    for (int iter = 0; iter < max_iter; iter++) {
        bool changed = false;
#pragma unroll
        for (int i = 0; i < 3; i++) {
#pragma unroll
            for (int j = i + 1; j < 4; j++) {
                double a = W[i], b = W[j], p = 0;
#pragma unroll
                for (int k = 0; k < M; k++) p += At[i][k] * At[j][k];
                if (!(fabs(p) <= eps * sqrt(a * b))) {
                    p *= 2;
                    double beta = a - b, gamma = hypot_glibc(p, beta);
                    double c, s;
                    if (beta < 0) {
                        double delta = (gamma - beta) * 0.5;
                        s = sqrt(delta / gamma);
                        c = p / (gamma * s * 2);
                    } else {
                        c = sqrt((gamma + beta) / (gamma * 2));
                        s = p / (gamma * c * 2);
                    }
                    a = 0;
                    b = 0;
#pragma unroll
                    for (int k = 0; k < M; k++) {
                        double t0 = c * At[i][k] + s * At[j][k];
                        double t1 = -s * At[i][k] + c * At[j][k];
                        At[i][k] = t0;
                        At[j][k] = t1;
                        a += t0 * t0;
                        b += t1 * t1;
                    }
                    W[i] = a;
                    W[j] = b;
                    changed = true;
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        double t0 = c * Vt[i][k] + s * Vt[j][k];
                        double t1 = -s * Vt[i][k] + c * Vt[j][k];
                        Vt[i][k] = t0;
                        Vt[j][k] = t1;
                    }
                }
            }
        }
        if (!changed) break;
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        double sd = 0;
#pragma unroll
        for (int k = 0; k < M; k++) sd += At[i][k] * At[i][k];
        W[i] = sqrt(sd);
    }
    // descending selection sort (only the Vt rows matter), compile-time row indices
#pragma unroll
    for (int i = 0; i < 3; i++) {
        int j = i;
        double wj = W[i];
#pragma unroll
        for (int k = i + 1; k < 4; k++)
            if (wj < W[k]) {
                wj = W[k];
                j = k;
            }
#pragma unroll
        for (int k = i + 1; k < 4; k++)
            if (j == k) {
                double t = W[i];
                W[i] = W[k];
                W[k] = t;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    double tv = Vt[i][q];
                    Vt[i][q] = Vt[k][q];
                    Vt[k][q] = tv;
                }
            }
    }
#pragma unroll
    for (int q = 0; q < 4; q++) nv[q] = Vt[3][q];
}

// Certification of the throughput solvers against the exact path (OpenCV's rounding sequence).
// A float64 value c that the exact path rounds to float32 (cvmSet into the f32 points4D, the f32
// undistorted points) is computed here with an error |e| <= delta.  If c lies farther than
// 2·delta from the f32 rounding midpoint nearest it, float(c + e) == float(c): both paths store
// the same bits.  That midpoint has c's sign, exponent and upper 23 mantissa bits and mantissa bit
// 28 set (one v_and_or_b32); c - m is exact (Sterbenz).  The factor 2 covers the finer f32 grid
// just below a power of two.  NaN / Inf / 0 / f32-subnormal c never pass (|c - m| is NaN or
// below any delta used here).
__device__ __forceinline__ bool f32_rounding_stable(double c, double delta2) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(c);
    const unsigned long long mb = (b & 0xFFFFFFFFE0000000ull) | 0x10000000ull;
    return fabs(c - __longlong_as_double((long long)mb)) > delta2;
}

// Error bound of a certified null vector (unit vector, absolute per component):
//   8 · (remaining inverse-iteration error, estimated as step² / previous step: the iterate's
//        off-null component shrinks by the same factor λ₄/λ₃ each step; sqrt(dd) once the
//        steps stop contracting, i.e. at the rounding floor)
// + 0.2 · eps · sqrt(tr M / D₂) (rounding floor of both solvers; eps·σ₁/σ₃ with D₂ the third
//        LDLᵀ pivot of M = AᵀA standing in for λ₃: the exact Jacobi's own error measured
//        <= 0.025 of it, the normal equations' floor <= 0.0033, D₂/λ₃ <= 1.4, on 1.4 M synthetic
//        and random points: tools/tri_cert_emu.c — an EMPIRICAL bound, not a proof; the GPU
//        tests add adversarial rigs: tiny baselines, points near the epipoles)
// + 2^-50 (normalisation).  Returned doubled for f32_rounding_stable.
__device__ __forceinline__ double null_vector_delta2(double dd, double prev, double cond2) {
    const float d = (float)dd, pv = (float)prev;
    const float it_err = d * __builtin_amdgcn_rsqf(fmaxf(fmaxf(d, pv), 1e-37f));
    return (double)(16.f * it_err + 0.4f * 2.220446e-16f * __builtin_sqrtf((float)cond2) + 0x1p-49f);
}

__device__ __forceinline__ bool null_vector_certified(const double (&nv)[4], double delta2) {
    return f32_rounding_stable(nv[0], delta2) && f32_rounding_stable(nv[1], delta2) &&
           f32_rounding_stable(nv[2], delta2) && f32_rounding_stable(nv[3], delta2);
}

// Fast null vector of A (M x 4): Householder QR (A = QR; R is 4x4 upper
// triangular with A's right singular vectors), then inverse iteration on RᵀR
// started from R⁻¹e₄.  Each step shrinks the component off the smallest right
// singular vector by (σ₄/σ₃)² (~1e-6 on real rigs), so two or three steps reach
// the fp64 noise floor, where the unit vector agrees with JacobiSVDImpl_'s Vt
// row 3 to ~1e-13 (its own rounding error) at a fraction of the FP64 work.
// Returns false unless the iteration has provably converged (ill-conditioned
// geometry with σ₄ ≈ σ₃, NaN/Inf input) AND its f32-rounded components are certified equal
// to the Jacobi restatement's (null_vector_certified): the caller then runs the exact Jacobi
// restatement, so the default solver's outputs are bit-identical to the exact path's.  FMA contraction is allowed here: this is an approximation of the
// Jacobi result, checked by its own convergence test, not a restatement of
// OpenCV's rounding sequence.
template <int M>
__device__ __forceinline__ bool qr_inverse_iteration(const double (&A0)[M][4], double (&nv)[4]) {
#pragma clang fp contract(fast)
    double A[M][4];
#pragma unroll
    for (int r = 0; r < M; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) A[r][c] = A0[r][c];
    double R[4][4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        double s = 0;
#pragma unroll
        for (int r = k; r < M; r++) s += A[r][k] * A[r][k];
        const double nrm = sqrt_fast(s);
        if (k == 3) {
            R[3][3] = nrm;
            break;
        }
        const double akk = A[k][k];
        const double alpha = akk >= 0 ? -nrm : nrm;
        // reflector v = a - alpha·e_k; vᵀv / 2 = nrm (nrm + |akk|)
        const double half_vtv = nrm * (nrm + fabs(akk));
        const double inv = half_vtv > 0 ? recip_rn(half_vtv) : 0.0;
        A[k][k] = akk - alpha;
        R[k][k] = alpha;
#pragma unroll
        for (int j = k + 1; j < 4; j++) {
            double d = 0;
#pragma unroll
            for (int r = k; r < M; r++) d += A[r][k] * A[r][j];
            const double t = d * inv;
#pragma unroll
            for (int r = k; r < M; r++) A[r][j] -= t * A[r][k];
            R[k][j] = A[k][j];
        }
    }
    // an exactly singular R (noise-free data): a perturbation far below the QR
    // rounding error keeps R⁻¹ finite and changes nothing else
    const double scale = fmax(fmax(fabs(R[0][0]), fabs(R[1][1])), fabs(R[2][2]));
    if (fabs(R[3][3]) < 1e-18 * scale) R[3][3] = 1e-18 * scale;
    double d[4];
#pragma unroll
    for (int k = 0; k < 4; k++) d[k] = recip_rn(R[k][k]);
    auto back = [&](double (&x)[4]) {  // x <- R⁻¹ x
        x[3] = x[3] * d[3];
        x[2] = (x[2] - R[2][3] * x[3]) * d[2];
        x[1] = (x[1] - R[1][2] * x[2] - R[1][3] * x[3]) * d[1];
        x[0] = (x[0] - R[0][1] * x[1] - R[0][2] * x[2] - R[0][3] * x[3]) * d[0];
    };
    auto fwd = [&](double (&x)[4]) {  // x <- R⁻ᵀ x
        x[0] = x[0] * d[0];
        x[1] = (x[1] - R[0][1] * x[0]) * d[1];
        x[2] = (x[2] - R[0][2] * x[0] - R[1][2] * x[1]) * d[2];
        x[3] = (x[3] - R[0][3] * x[0] - R[1][3] * x[1] - R[2][3] * x[2]) * d[3];
    };
    auto normalize = [&](double (&x)[4]) {
        const double is = rsqrt_fast(x[0] * x[0] + x[1] * x[1] + x[2] * x[2] + x[3] * x[3]);
#pragma unroll
        for (int q = 0; q < 4; q++) x[q] *= is;
    };
    double x[4] = {0.0, 0.0, 0.0, 1.0};
    back(x);
    normalize(x);
    double prev = 1.0;  // squared step length of the previous iteration
    for (int it = 0; it < 12; it++) {
        double y[4] = {x[0], x[1], x[2], x[3]};
        fwd(y);
        back(y);
        normalize(y);  // (RᵀR)⁻¹ is positive definite: no sign flip between iterates
        double dd = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const double e = y[q] - x[q];
            dd += e * e;
            x[q] = y[q];
        }
        // squared step dd; geometric convergence: remaining error ≈ step · (step / prev),
        // i.e. step <= 4e-16, or step <= 1e-6 and step² <= 1e-14 · prev
        if (dd <= 1.6e-31 || (dd <= 1e-12 && dd * dd <= 1e-28 * prev)) {
#pragma unroll
            for (int q = 0; q < 4; q++) nv[q] = x[q];
            // certified against the exact path, else its Jacobi: RᵀR = AᵀA, so tr M = ‖R‖²_F
            // and the third LDLᵀ pivot is R₂₂²
            double trm = 0;
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = i; j < 4; j++) trm += R[i][j] * R[i][j];
            return null_vector_certified(nv, null_vector_delta2(dd, prev, trm * d[2] * d[2]));
        }
        if (it >= 2 && !(dd < 0.25 * prev)) return false;  // not contracting (or NaN)
        prev = dd;
    }
    return false;
}

// The DLT's null vector, the one place that decides between the two solvers: the exact Jacobi
// restatement (on Aᵀ) for every lane when EXACT, else only for the lanes whose QR / inverse
// iteration is not certified equal to it — bit-identical either way.  Returns whether the fast
// solver's vector stood.  No caller reads that, but it stays: written as a void function the fast
// kernels compile to different code (triangulate_reference_kernel<kFast>: 134 VGPRs against 118).
template <bool EXACT, int M>
__device__ __forceinline__ bool dlt_null_vector(const double (&A)[M][4], double (&nv)[4]) {
    const bool fast = !EXACT && qr_inverse_iteration<M>(A, nv);
    if (!fast) {
        double At[4][M];
#pragma unroll
        for (int c = 0; c < 4; c++)
#pragma unroll
            for (int r = 0; r < M; r++) At[c][r] = A[r][c];
        jacobi_null_vector<M>(At, nv);
    }
    return fast;
}

// cvmSet into the f32 points4D, then convertPointsFromHomogeneous in f32; xyz: 3 floats.
__device__ __forceinline__ void dehomogenize_f32(const double (&nv)[4], float* __restrict__ xyz) {
    const float X = (float)nv[0], Y = (float)nv[1], Z = (float)nv[2], w = (float)nv[3];
    const float s = (w != 0.f) ? __frcp_rn(w) : 1.f;
    xyz[0] = __fmul_rn(X, s);
    xyz[1] = __fmul_rn(Y, s);
    xyz[2] = __fmul_rn(Z, s);
}

__device__ __forceinline__ void write_result(const double (&nv)[4], int64_t p, float* __restrict__ out,
                                             double* __restrict__ out4) {
    dehomogenize_f32(nv, out + 3 * p);
    if (out4) {
        out4[4 * p + 0] = nv[0];
        out4[4 * p + 1] = nv[1];
        out4[4 * p + 2] = nv[2];
        out4[4 * p + 3] = nv[3];
    }
}

__device__ __forceinline__ void add_view_rows(double (*A)[4], int r, double x, double y,
                                              const double* __restrict__ P) {
#pragma unroll
    for (int k = 0; k < 4; k++) {
        A[r][k] = x * P[8 + k] - P[0 + k];
        A[r + 1][k] = y * P[8 + k] - P[4 + k];
    }
}

__device__ __forceinline__ void load_cams(double (*scam)[MVP_CAM_DOUBLES], CamFast* sfast,
                                          const double* __restrict__ cams, int n_cams) {
    const int total = n_cams * MVP_CAM_DOUBLES;
    for (int i = threadIdx.x; i < total; i += blockDim.x) scam[i / MVP_CAM_DOUBLES][i % MVP_CAM_DOUBLES] = cams[i];
    if (threadIdx.x < n_cams) {
        const double* c = cams + threadIdx.x * MVP_CAM_DOUBLES;
        sfast[threadIdx.x].ifx = 1. / c[0];
        sfast[threadIdx.x].ify = 1. / c[4];
    }
    __syncthreads();
}

// A view's keypoint may enter a solve: finite coordinates, a confidence that is no NaN and
// reaches min_conf (the robust and the refinement kernels' rule, mvpose.h).
__device__ __forceinline__ bool view_usable(float x, float y, float conf, float min_conf) {
    return isfinite(x) && isfinite(y) && !isnan(conf) && conf >= min_conf;
}

// Reprojection error of view i against homogeneous X (the robust and the peak-selecting kernels'
// rule, mvpose.h): q = P_i·X in fp64; +inf unless q2·X3 > 0 (in front of the camera), else the
// distance of (q0/q2, q1/q2) to the f32 undistorted point.
__device__ __forceinline__ double reprojection_error(const double* __restrict__ P, const double (&X)[4], float ux,
                                                     float uy) {
    const double q0 = P[0] * X[0] + P[1] * X[1] + P[2] * X[2] + P[3] * X[3];
    const double q1 = P[4] * X[0] + P[5] * X[1] + P[6] * X[2] + P[7] * X[3];
    const double q2 = P[8] * X[0] + P[9] * X[1] + P[10] * X[2] + P[11] * X[3];
    if (!(q2 * X[3] > 0)) return (double)INFINITY;
    const double dx = q0 / q2 - (double)ux, dy = q1 / q2 - (double)uy;
    return sqrt(dx * dx + dy * dy);
}

// ----------------------------------------------------------------- host side
// The argument checks every N-view entry point opens with; `fn`, the entry point's name, prefixes
// each message.  Returns the listed cameras.  No device call: the callers' n_points == 0 return
// and their null-pointer check come after it.
inline CamIdx tri_parse_args(const char* fn, int64_t n_points, int V, int n_cams, const int* cam_idx,
                             int n_cam_idx) {
    MVP_REQUIRE(n_points >= 0, "%s: n_points < 0", fn);
    MVP_REQUIRE(V >= 2 && V <= 64, "%s: V=%d out of range", fn, V);
    MVP_REQUIRE(n_cams >= 1 && n_cams <= kMaxCams, "%s: n_cams=%d (1..%d)", fn, n_cams, kMaxCams);
    MVP_REQUIRE(cam_idx != nullptr, "%s: cam_idx is NULL", fn);
    MVP_REQUIRE(n_cam_idx >= 2 && n_cam_idx <= kMaxCams, "%s: n_cam_idx=%d (2..%d)", fn, n_cam_idx, kMaxCams);
    CamIdx ci{};
    for (int i = 0; i < n_cam_idx; i++) {
        MVP_REQUIRE(cam_idx[i] >= 0 && cam_idx[i] < V && cam_idx[i] < n_cams,
                    "%s: cam_idx[%d]=%d out of range (V=%d, n_cams=%d)", fn, i, cam_idx[i], V, n_cams);
        ci.v[i] = cam_idx[i];
    }
    return ci;
}

// Blocks of kBlock lanes, one point per lane.
inline unsigned tri_grid(const char* fn, int64_t n_points) {
    const int64_t blocks = (n_points + kBlock - 1) / kBlock;
    MVP_REQUIRE(blocks < (1LL << 31), "%s: too many points", fn);
    return (unsigned)blocks;
}

// f(std::integral_constant<int, NV>) for the run-time view count NV = n_cam_idx (2..kMaxCams,
// checked by tri_parse_args): the kernels take the view count as a template argument.
template <class F>
inline void tri_dispatch_views(int n_cam_idx, F&& f) {
    switch (n_cam_idx) {
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 3: f(std::integral_constant<int, 3>{}); break;
        case 4: f(std::integral_constant<int, 4>{}); break;
        case 5: f(std::integral_constant<int, 5>{}); break;
        case 6: f(std::integral_constant<int, 6>{}); break;
        case 7: f(std::integral_constant<int, 7>{}); break;
        case 8: f(std::integral_constant<int, 8>{}); break;
    }
}

}  // namespace

namespace mvp {

// triangulate_tol.hip: the two launches of the certified tolerance solver (MVP_TRI_REFERENCE |
// MVP_TRI_TOLERANCE with two listed cameras) for mvp_triangulate.  cam_idx: CamIdx::v (the kernels'
// parameter type is local to each translation unit); blocks: tri_grid's count.
__attribute__((visibility("hidden"))) void launch_triangulate_tol2(
    const float* kpts, int64_t n_points, int V, const double* cams, int n_cams, const int (&cam_idx)[kMaxCams],
    unsigned blocks, float* out_xyz, double* out_xyzw, hipStream_t s);

}  // namespace mvp
