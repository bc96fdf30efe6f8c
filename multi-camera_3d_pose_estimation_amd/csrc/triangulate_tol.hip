// MVP_TRI_TOLERANCE: the certified two-camera triangulation solver (numerics contract and shared
// device code in tri_common.h; map of the triangulation files in triangulate.hip).
#pragma clang fp contract(off)

#include "tri_common.h"

#include <algorithm>
#include <cstdlib>
#include <map>
#include <mutex>
#include <utility>

namespace {

// ----------------------------------------------------------------- tolerance mode
// MVP_TRI_TOLERANCE: the reference-mode two-camera problem solved for throughput, with every
// output CERTIFIED bit-identical to the exact path (OpenCV's rounding sequence); a point that
// cannot be certified is re-solved on the exact path by a second launch.
//   * undistortion: OpenCV's 5 fixed iterations.  The first NF32 run in f32 (both views packed
//     in v_pk_* instructions) on the distortion correction c = x - x0 rather than on x, so the
//     f32 rounding error scales with |c| ~ |k1| r² |x| instead of |x|; the rest run in fp64 from
//     x0 + c.  Bound: the f32 iterates' error <= kappa · 2^-24 · (the terms' magnitudes), carried
//     through each fp64 iteration by L, a bound on the iteration map's Jacobian at the last f32
//     iterate (the distortion polynomial's derivative and the tangential terms), plus the fp64
//     rounding; the f64 undistorted pixel is certified when it lies farther than that bound from
//     an f32 rounding midpoint (f32_rounding_stable): its f32 rounding is then the exact path's;
//   * null vector: normal equations M = AᵀA (fp64), LDLᵀ, inverse iteration from M⁻¹e₄ to a
//     geometric convergence test (2-5 steps; each shrinks the off-null component by
//     λ₄/λ₃ = (σ₄/σ₃)², median 4e-7 on the synthetic rigs); certified by null_vector_delta2;
//   * the camera at the world origin (P = [K | 0], the reference's camera 0,
//     setup_camera_configuration.py:392-393) contributes 6 non-zero entries to M, 3 of them per-
//     camera constants: M is formed from its two rows in closed form (21 fewer fp64 operations);
//   * not certified, not contracting (σ₄ ≈ σ₃ geometry), Inf input, a distortion denominator
//     near zero (OpenCV's icdist < 0 branch): the exact path (fallback launch).  NaN input is
//     answered inline (the exact path gives NaN for every output).
// The certified result is dehomogenised through OpenCV's f32 chain (write_result, shared).
// Measured rates (tests/test_triangulate_gpu.py prints them): see DESIGN.md §4.2.

typedef float f2v __attribute__((ext_vector_type(2)));

struct CamTol {              // per-camera constants of the f32 iterations and the error bound
    float k1, k2, k3;        // radial
    float p1, p2, p1x2, p2x2;  // tangential, and doubled
    float a1, a2, a3, b;     // Jacobian bound: 2|k1|, 4|k2|, 6|k3|, 8(|p1| + |p2|)
    float kn;                // |fx| + |skew| + |fy|: pixels per normalised unit
    float floor2;            // 2 · 2^-45 (|cx| + |cy|): the K application's rounding near cx, cy
    int ok;                  // K's last row is (0, 0, 1) and fx, fy != 0: the pixel bound holds
    int origin;              // P = [K | 0] with K's last row (0, 0, 1) and K[1][0] == 0
};

__device__ __forceinline__ CamTol make_cam_tol(const double* __restrict__ c) {
    CamTol t;
    const double k1 = c[9], k2 = c[10], p1 = c[11], p2 = c[12], k3 = c[13];
    t.k1 = (float)k1;
    t.k2 = (float)k2;
    t.k3 = (float)k3;
    t.p1 = (float)p1;
    t.p2 = (float)p2;
    t.p1x2 = (float)(2 * p1);
    t.p2x2 = (float)(2 * p2);
    t.a1 = (float)(2 * fabs(k1)) * 1.0001f;
    t.a2 = (float)(4 * fabs(k2)) * 1.0001f;
    t.a3 = (float)(6 * fabs(k3)) * 1.0001f;
    t.b = (float)(8 * (fabs(p1) + fabs(p2))) * 1.0001f;
    t.kn = (float)(fabs(c[0]) + fabs(c[1]) + fabs(c[4])) * 1.0001f;
    t.floor2 = (float)(0x1p-44 * (fabs(c[2]) + fabs(c[5])));
    t.ok = c[6] == 0 && c[7] == 0 && c[8] == 1 && c[0] != 0 && c[4] != 0;
    const double* P = c + 26;
    t.origin = t.ok && c[3] == 0 && P[3] == 0 && P[7] == 0 && P[11] == 0 && P[8] == 0 && P[9] == 0 && P[10] == 1 &&
               P[4] == 0 && P[0] == c[0] && P[1] == c[1] && P[2] == c[2] && P[5] == c[4] && P[6] == c[5];
    return t;
}

// Both views of a point: (u, v) pixels -> undistorted pixels (P = K), OpenCV's iteration, the
// first NF32 of the 5 in f32 on the correction, the rest in fp64.  ox / oy: the f32 values;
// certified &= both views' values provably equal the exact path's.
template <int NF32>
__device__ __forceinline__ void undistort_pair_tol(const float (&u)[2], const float (&v)[2],
                                                   const double* __restrict__ c0, const double* __restrict__ c1,
                                                   const CamFast& f0, const CamFast& f1, const CamTol& t0,
                                                   const CamTol& t1, float (&ox)[2], float (&oy)[2],
                                                   bool& certified) {
#pragma clang fp contract(fast)
    constexpr int NF64 = 5 - NF32;
    const double* cc[2] = {c0, c1};
    double x0[2], y0[2];
    x0[0] = ((double)u[0] - c0[2]) * f0.ifx;
    y0[0] = ((double)v[0] - c0[5]) * f0.ify;
    x0[1] = ((double)u[1] - c1[2]) * f1.ifx;
    y0[1] = ((double)v[1] - c1[5]) * f1.ify;
    const f2v X0 = {(float)x0[0], (float)x0[1]}, Y0 = {(float)y0[0], (float)y0[1]};
    const f2v K1 = {t0.k1, t1.k1}, K2 = {t0.k2, t1.k2}, K3 = {t0.k3, t1.k3};
    const f2v P1 = {t0.p1, t1.p1}, P2 = {t0.p2, t1.p2}, P1x2 = {t0.p1x2, t1.p1x2}, P2x2 = {t0.p2x2, t1.p2x2};
    const f2v one = {1.f, 1.f}, two = {2.f, 2.f};
    f2v cx = {0.f, 0.f}, cy = {0.f, 0.f}, x = X0, y = Y0, r2 = {0.f, 0.f}, poly = {0.f, 0.f};
    f2v ic = {1.f, 1.f}, dX = {0.f, 0.f}, dY = {0.f, 0.f};
    f2v den_min = {1.f, 1.f};
#pragma unroll
    for (int j = 0; j < NF32; j++) {
        x = X0 + cx;
        y = Y0 + cy;
        r2 = __builtin_elementwise_fma(x, x, y * y);
        poly = r2 * __builtin_elementwise_fma(__builtin_elementwise_fma(K3, r2, K2), r2, K1);
        const f2v den = poly + one;
        den_min = __builtin_elementwise_min(den_min, den);
        ic.x = __builtin_amdgcn_rcpf(den.x);
        ic.y = __builtin_amdgcn_rcpf(den.y);
        const f2v xy = x * y;
        dX = __builtin_elementwise_fma(P1x2, xy, P2 * __builtin_elementwise_fma(two * x, x, r2));
        dY = __builtin_elementwise_fma(P1, __builtin_elementwise_fma(two * y, y, r2), P2x2 * xy);
        cx = -(__builtin_elementwise_fma(X0, poly, dX) * ic);
        cy = -(__builtin_elementwise_fma(Y0, poly, dY) * ic);
    }
    // error of the f32 correction: kappa = 8 roundings of the terms it is built from (X0 and the
    // iterate x rounded to f32, poly, the tangential terms, the approximate reciprocal),
    // propagated through each later iteration by L.  Scalar f32 (|.| is a free source modifier
    // there; packed instructions would need an and-mask per absolute value).  |x| + |y| <=
    // 0.5 + r² bounds the tangential Jacobian's (|x| + |y|) factor without absolute values.
    const CamTol* tt[2] = {&t0, &t1};
    float errq[2];
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const float r2q = q ? r2.y : r2.x, icq = q ? ic.y : ic.x, pq = q ? poly.y : poly.x;
        const float L = icq * __builtin_fmaf(r2q, __builtin_fmaf(__builtin_fmaf(tt[q]->a3, r2q, tt[q]->a2), r2q, tt[q]->a1),
                                             tt[q]->b * (0.5f + r2q));
        const float terms = __builtin_fmaf(fabsf(q ? X0.y : X0.x) + fabsf(q ? Y0.y : Y0.x), fabsf(pq),
                                           fabsf(q ? dX.y : dX.x) + fabsf(q ? dY.y : dY.x));
        float e = (8.f * 0x1p-24f) * terms * icq;
#pragma unroll
        for (int j = 0; j < NF64; j++) e *= L;
        errq[q] = e;
    }
    double xd[2] = {x0[0] + (double)cx.x, x0[1] + (double)cx.y};
    double yd[2] = {y0[0] + (double)cy.x, y0[1] + (double)cy.y};
    double dmin[2] = {(double)den_min.x, (double)den_min.y};
#pragma unroll
    for (int j = NF32; j < 5; j++) {
#pragma unroll
        for (int q = 0; q < 2; q++) {
            const double* c = cc[q];
            const double k1 = c[9], k2 = c[10], p1 = c[11], p2 = c[12], k3 = c[13];
            const double rr = xd[q] * xd[q] + yd[q] * yd[q];
            const double den = 1 + ((k3 * rr + k2) * rr + k1) * rr;
            dmin[q] = fmin(dmin[q], den);
            const double icd = rcp_nr1(den);
            const double ddX = 2 * p1 * xd[q] * yd[q] + p2 * (rr + 2 * xd[q] * xd[q]);
            const double ddY = p1 * (rr + 2 * yd[q] * yd[q]) + 2 * p2 * xd[q] * yd[q];
            xd[q] = (x0[q] - ddX) * icd;
            yd[q] = (y0[q] - ddY) * icd;
        }
    }
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const double* c = cc[q];
        const double ww = rcp_nr1(c[6] * xd[q] + c[7] * yd[q] + c[8]);
        const double oxd = (c[0] * xd[q] + c[1] * yd[q] + c[2]) * ww;
        const double oyd = (c[3] * xd[q] + c[4] * yd[q] + c[5]) * ww;
        ox[q] = (float)oxd;
        oy[q] = (float)oyd;
        // pixel error bound, doubled: kn · (the f32 error carried through) + 2^-44 (|ox| + |oy|)
        // + floor2 (2^-44 (|cx| + |cy|)): the fp64 iterations' and the K application's rounding
        // (kn |x| <= |ox| + |cx|, so this covers 2^-46 kn |x| with a factor 4)
        const double d2 = __builtin_fma(0x1p-44, fabs(oxd) + fabs(oyd), (double)(2.f * tt[q]->kn * errq[q] + tt[q]->floor2));
        // OpenCV's icdist < 0 branch (keep the initial guess) and a near-zero denominator are left
        // to the exact path: the f32 and fp64 denominators could disagree on the sign
        certified = certified && tt[q]->ok && dmin[q] > 0x1p-10 && f32_rounding_stable(oxd, d2) &&
                    f32_rounding_stable(oyd, d2);
    }
}

// Null vector of M = AᵀA (lower triangle m[i][j], j <= i) by LDLᵀ inverse iteration; false = not
// provably converged or not certified against the exact path.
__device__ __forceinline__ bool normal_eq_null_vector(const double (&m)[4][4], double (&nv)[4]) {
#pragma clang fp contract(fast)
    // LDLᵀ (lower triangle of m)
    const double D0 = m[0][0], r0 = rcp_nr(D0);
    const double l10 = m[1][0] * r0, l20 = m[2][0] * r0, l30 = m[3][0] * r0;
    const double a11 = m[1][1] - l10 * m[1][0], a21 = m[2][1] - l20 * m[1][0], a31 = m[3][1] - l30 * m[1][0];
    const double a22 = m[2][2] - l20 * m[2][0], a32 = m[3][2] - l30 * m[2][0], a33 = m[3][3] - l30 * m[3][0];
    const double r1 = rcp_nr(a11);
    const double l21 = a21 * r1, l31 = a31 * r1;
    const double b22 = a22 - l21 * a21, b32 = a32 - l31 * a21, b33 = a33 - l31 * a31;
    const double r2 = rcp_nr(b22);
    const double l32 = b32 * r2;
    double D3 = b33 - l32 * b32;
    // an exactly singular M (noise-free data): the last pivot is rounding noise of either sign;
    // a positive pivot far below the factorisation's rounding keeps the solves finite and M⁻¹
    // positive definite (a negative one flipped the iterate's sign every step, so 27 % of the
    // noise-free points never converged) and changes nothing else
    if (!(D3 >= 1e-30 * D0)) D3 = 1e-30 * D0;
    const double r3 = rcp_nr(D3);
    auto solve = [&](double (&y)[4]) {  // y <- M⁻¹ y
        const double z1 = y[1] - l10 * y[0];
        const double z2 = y[2] - l20 * y[0] - l21 * z1;
        const double z3 = y[3] - l30 * y[0] - l31 * z1 - l32 * z2;
        y[3] = z3 * r3;
        y[2] = z2 * r2 - l32 * y[3];
        y[1] = z1 * r1 - l21 * y[2] - l31 * y[3];
        y[0] = y[0] * r0 - l10 * y[1] - l20 * y[2] - l30 * y[3];
    };
    double x[4];
    x[3] = r3;  // M⁻¹ e₄
    x[2] = -l32 * x[3];
    x[1] = -l21 * x[2] - l31 * x[3];
    x[0] = -l10 * x[1] - l20 * x[2] - l30 * x[3];
    {
        const double is = rsqrt_fast(x[0] * x[0] + x[1] * x[1] + x[2] * x[2] + x[3] * x[3]);
#pragma unroll
        for (int q = 0; q < 4; q++) x[q] *= is;
    }
    // e₄ is a poor start (the null vector is (X, Y, Z, 1)/|.| with |X, Y, Z| ~ 1e2-1e3 world
    // units, so its e₄ component is ~1/350) and λ₄/λ₃ reaches ~2e-5 on the synthetic rigs:
    // iterate to a geometric convergence test (remaining error ≈ step · step / previous step
    // <= 1e-13).  Branch-free per lane: every lane takes the same steps (a converged lane stays
    // converged), two unconditionally, more only while some lane of the wave is still
    // contracting — the per-lane early exits compiled to ~40 register copies per step.
    auto step = [&](double& dd) {
        double y[4] = {x[0], x[1], x[2], x[3]};
        solve(y);
        const double is = rsqrt_fast(y[0] * y[0] + y[1] * y[1] + y[2] * y[2] + y[3] * y[3]);
        dd = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            y[q] *= is;  // M⁻¹ is positive definite (up to the pivot clamp): no sign flip
            const double e = y[q] - x[q];
            dd += e * e;
            x[q] = y[q];
        }
    };
    auto converged = [](double dd, double prev) { return dd <= 1e-26 || (dd <= 1e-16 && dd * dd <= 1e-26 * prev); };
    double d0, d1;
    step(d0);
    step(d1);
    bool ok = converged(d1, d0) || converged(d0, 1.0);
    bool failed = false;
    double prev = d0, last = d1;
#pragma unroll 1
    for (int it = 2; it < 8 && __builtin_amdgcn_ballot_w64(!ok && !failed) != 0; it++) {
        double dd;
        step(dd);
        const bool now = converged(dd, last);
        failed = failed || (!ok && !now && !(dd < 0.25 * last));  // not contracting (or NaN)
        ok = ok || now;
        prev = last;
        last = dd;
    }
#pragma unroll
    for (int q = 0; q < 4; q++) nv[q] = x[q];
    // certification: the rounding floor uses tr M / D₂ (D₂ = b22, the third pivot)
    const double cond2 = (m[0][0] + m[1][1] + (m[2][2] + m[3][3])) * r2;
    return ok && !failed && null_vector_certified(nv, null_vector_delta2(last, prev, cond2));
}

// MVP_TRI_REFERENCE | MVP_TRI_TOLERANCE with camera_indices of length 2 (the reference's
// hard-coded [0, 1]): the top-2 rule reduces to one comparison (np.argsort of two values:
// [0, 1] unless conf[1] < conf[0], NaN sorts last).
struct Tol2Sel {
    int pos0, pos1;
    float u[2], v[2];
};
__device__ __forceinline__ Tol2Sel tol2_select(const float* __restrict__ kp, int V, const CamIdx& ci) {
    const int ca = ci.v[0], cb = ci.v[1];
    const float conf_a = kp[2 * V + ca], conf_b = kp[2 * V + cb];
    // stable ascending argsort of (conf_a, conf_b), NaN last: swapped iff conf_b sorts before conf_a
    const bool swap = isnan(conf_a) ? !isnan(conf_b) : (conf_b < conf_a);
    // rows of the lower-confidence camera first; each view's point comes from its column
    // ci.v[pos] and its parameters from camera key = its position pos in camera_indices
    Tol2Sel r;
    r.pos0 = swap ? 1 : 0;
    r.pos1 = swap ? 0 : 1;
    const int col0 = ci.v[r.pos0], col1 = ci.v[r.pos1];
    r.u[0] = kp[col0];
    r.u[1] = kp[col1];
    r.v[0] = kp[V + col0];
    r.v[1] = kp[V + col1];
    return r;
}

// Points the tolerance kernel could not certify are re-solved on the exact path by a second
// launch, so the exact path's registers (Jacobi on A^T and V^T: the inline fallback held the
// kernel at 150 VGPRs = 3 waves per SIMD) never limit the occupancy of the throughput kernel.
// The tolerance kernel marks such a point's x output with a signalling-NaN sentinel (arithmetic
// never produces it) and appends its index to a per-stream list (one atomic per wave); past the
// list's capacity the fallback sweeps the outputs for the sentinel instead.  The fallback grid
// (kFbBlocks workgroups, one exact point per lane at a time) adds its count to a running total
// (mvp_triangulate_fallback_total) and its last workgroup resets the list for the next launch.
constexpr int kFbCap = 1 << 16;
constexpr int kFbBlocks = 128;
constexpr uint32_t kFbSentinel = 0x7FA5A5A5u;

struct FbHeader {
    unsigned count;            // entries appended by the current launch
    unsigned done;             // fallback workgroups finished (the last one resets)
    unsigned long long total;  // points re-solved on this stream since the list was created
};

struct FbList {
    FbHeader* hdr;
    unsigned* idx;  // [kFbCap]
    int force;      // tests: send every finite point to the fallback (MVPOSE_TRI_FORCE_FALLBACK=1)
};

// M = AᵀA (lower triangle) of the two views' DLT rows x·P₂ - P₀, y·P₂ - P₁ (FMA-contracted:
// any rounding is inside the certification's floor).  ORIGIN = 1: view 0's camera has P = [K | 0]
// with K's last row (0, 0, 1): its rows are (-fx, -s, du, 0) and (0, -fy, dv, 0) with du = x - cx,
// dv = y - cy (the values the generic rows hold) and its part of M is fx², fx·s, s² + fy²
// (constants), -fx·du, -(s·du + fy·dv), du² + dv².
template <bool ORIGIN>
__device__ __forceinline__ void normal_matrix_2v(const double (&x)[2], const double (&y)[2],
                                                 const double* __restrict__ c0, const double* __restrict__ c1,
                                                 double (&m)[4][4]) {
#pragma clang fp contract(fast)
    double a[2][4], b[2][4];
#pragma unroll
    for (int q = ORIGIN ? 1 : 0; q < 2; q++) {
        const double* P = (q == 0 ? c0 : c1) + 26;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            a[q][k] = __builtin_fma(x[q], P[8 + k], -P[0 + k]);
            b[q][k] = __builtin_fma(y[q], P[8 + k], -P[4 + k]);
        }
    }
    if constexpr (ORIGIN) {
        const double fx = c0[0], s = c0[1], fy = c0[4];
        const double du = x[0] - c0[2], dv = y[0] - c0[5];
        double m0[4][4] = {};
        m0[0][0] = fx * fx;
        m0[1][0] = fx * s;
        m0[1][1] = s * s + fy * fy;
        m0[2][0] = -fx * du;
        m0[2][1] = -(s * du + fy * dv);
        m0[2][2] = du * du + dv * dv;
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j <= i; j++)
                m[i][j] = __builtin_fma(a[1][i], a[1][j], __builtin_fma(b[1][i], b[1][j], m0[i][j]));
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j <= i; j++) {
                double t = a[0][i] * a[0][j];
                t = __builtin_fma(b[0][i], b[0][j], t);
                t = __builtin_fma(a[1][i], a[1][j], t);
                m[i][j] = __builtin_fma(b[1][i], b[1][j], t);
            }
    }
}

// Grid-stride: a grid of (CUs x resident blocks per CU) blocks loops over the points, so the
// per-block set-up (camera records into LDS, their reciprocals and bound constants) is paid once
// per resident block instead of once per 256 points.  The point's live state is ~100 VGPRs; 5
// waves per SIMD (96 VGPRs, 4 spilled) measured 0.500 ms per 1 M frames against 0.525 for one
// point per thread at 5 waves and 0.556 at 4 (same box, gpurun_out/r05b).
template <int NF32>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(5))) void triangulate_tol2_kernel(
    const float* __restrict__ kpts, int64_t n, int V, const double* __restrict__ cams, int n_cams, CamIdx ci,
    float* __restrict__ out, double* __restrict__ out4, FbList fb) {
    __shared__ double scam[kMaxCams][MVP_CAM_DOUBLES];
    __shared__ CamFast sfast[kMaxCams];
    __shared__ CamTol stol[2];
    load_cams(scam, sfast, cams, n_cams);
    if (threadIdx.x < 2) stol[threadIdx.x] = make_cam_tol(cams + threadIdx.x * MVP_CAM_DOUBLES);
    __syncthreads();
    // the camera at the world origin (block-uniform): its rows in closed form, whichever order
    // the confidences put the two views in (the order only changes M's rounding)
    const int origin = stol[0].origin ? 0 : (stol[1].origin ? 1 : -1);
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < n; p += stride) {
        const Tol2Sel sel = tol2_select(kpts + p * 3 * V, V, ci);
        const double* cp[2] = {scam[sel.pos0], scam[sel.pos1]};
        bool ok;
        if (isnan(sel.u[0]) || isnan(sel.u[1]) || isnan(sel.v[0]) || isnan(sel.v[1])) {
            // a NaN coordinate makes every entry of its view's rows, hence the whole SVD, NaN on
            // the exact path: all outputs NaN
            const double qn = __builtin_nan("");
            const double nv[4] = {qn, qn, qn, qn};
            write_result(nv, p, out, out4);
            ok = true;
        } else {
            float ux[2], uy[2];
            bool cert = !fb.force;
            undistort_pair_tol<NF32>(sel.u, sel.v, cp[0], cp[1], sfast[sel.pos0], sfast[sel.pos1], stol[sel.pos0],
                                     stol[sel.pos1], ux, uy, cert);
            double m[4][4];
            if (origin >= 0) {
                const int io = sel.pos0 == origin ? 0 : 1;  // the origin camera's view slot
                const double xs[2] = {(double)(io == 0 ? ux[0] : ux[1]), (double)(io == 0 ? ux[1] : ux[0])};
                const double ys[2] = {(double)(io == 0 ? uy[0] : uy[1]), (double)(io == 0 ? uy[1] : uy[0])};
                normal_matrix_2v<true>(xs, ys, scam[origin], scam[1 - origin], m);
            } else {
                const double xs[2] = {(double)ux[0], (double)ux[1]}, ys[2] = {(double)uy[0], (double)uy[1]};
                normal_matrix_2v<false>(xs, ys, cp[0], cp[1], m);
            }
            double nv[4];
            ok = normal_eq_null_vector(m, nv) && cert;
            if (ok) write_result(nv, p, out, out4);
            else reinterpret_cast<unsigned*>(out)[3 * p] = kFbSentinel;
        }
        // wave-aggregated append of the uncertified points
        const unsigned long long msk = __ballot(!ok);
        if (msk) {
            const int lane = __lane_id();
            const int leader = __ffsll((long long)msk) - 1;
            unsigned base = 0;
            if (lane == leader) base = atomicAdd(&fb.hdr->count, (unsigned)__popcll(msk));
            base = __shfl(base, leader);
            if (!ok) {
                const unsigned slot = base + (unsigned)__popcll(msk & ((1ull << lane) - 1));
                if (slot < (unsigned)kFbCap) fb.idx[slot] = (unsigned)p;
            }
        }
    }
}

// The exact path (OpenCV undistortion with IEEE divisions, Jacobi SVD) for one point.
__device__ __forceinline__ void tol2_exact_point(const float* __restrict__ kpts, int64_t p, int V,
                                              const double (*scam)[MVP_CAM_DOUBLES], const CamIdx& ci,
                                              float* __restrict__ out, double* __restrict__ out4) {
    const Tol2Sel sel = tol2_select(kpts + p * 3 * V, V, ci);
    const double* cp[2] = {scam[sel.pos0], scam[sel.pos1]};
    float e0x, e0y, e1x, e1y;
    undistort_point(sel.u[0], sel.v[0], cp[0], e0x, e0y);
    undistort_point(sel.u[1], sel.v[1], cp[1], e1x, e1y);
    double E[4][4];
    add_view_rows(E, 0, e0x, e0y, cp[0] + 26);
    add_view_rows(E, 2, e1x, e1y, cp[1] + 26);
    double nv[4];
    dlt_null_vector<true, 4>(E, nv);
    write_result(nv, p, out, out4);
}

// kFbBlocks workgroups: the listed points (or, past the list's capacity, every point whose x
// output carries the sentinel), strided over the grid; the last workgroup to finish adds the
// count to the running total and resets the list for the next launch on the stream.  Every
// workgroup reads the count before it signals `done`, so the reset cannot race a reader.
__global__ __launch_bounds__(kBlock) void triangulate_tol2_fallback_kernel(
    const float* __restrict__ kpts, int64_t n, int V, const double* __restrict__ cams, int n_cams, CamIdx ci,
    float* __restrict__ out, double* __restrict__ out4, FbList fb) {
    __shared__ double scam[kMaxCams][MVP_CAM_DOUBLES];
    __shared__ CamFast sfast[kMaxCams];
    const unsigned cnt = __atomic_load_n(&fb.hdr->count, __ATOMIC_RELAXED);
    if (cnt == 0) return;  // the usual case: nothing to re-solve, the count is already 0
    load_cams(scam, sfast, cams, n_cams);
    const unsigned stride = gridDim.x * kBlock;
    if (cnt <= (unsigned)kFbCap) {
        for (unsigned i = blockIdx.x * kBlock + threadIdx.x; i < cnt; i += stride) {
            const unsigned p = fb.idx[i];
            if ((int64_t)p < n) tol2_exact_point(kpts, p, V, scam, ci, out, out4);  // never write past this call's n
        }
    } else {
        const unsigned* ob = reinterpret_cast<const unsigned*>(out);
        for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < n; p += stride)
            if (ob[3 * p] == kFbSentinel) tol2_exact_point(kpts, p, V, scam, ci, out, out4);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        if (atomicAdd(&fb.hdr->done, 1u) == gridDim.x - 1) {
            fb.hdr->total += cnt;
            fb.hdr->count = 0u;
            fb.hdr->done = 0u;
            __threadfence();
        }
    }
}

// The tolerance kernel's fallback list, one per (device, stream), allocated on first use
// (a stream-captured launch needs one uncaptured call on that stream first).  The list is
// shared by every call on its stream, so a call holds the list's own mutex from the first
// launch to the second: two host threads on one stream (PyTorch's default stream is shared)
// then enqueue tol A, fallback A, tol B, fallback B, never tol A, tol B, fallback A, ...
struct FbSlot {
    FbList fb;
    std::mutex* mu;
};

FbSlot tol_fallback_list(hipStream_t s) {
    static std::mutex mu;
    static std::map<std::pair<int, hipStream_t>, FbSlot> lists;
    int dev = 0;
    MVP_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    auto it = lists.find({dev, s});
    if (it != lists.end()) return it->second;
    void* buf = nullptr;
    MVP_HIP(hipMalloc(&buf, sizeof(FbHeader) + (size_t)kFbCap * sizeof(unsigned)));
    MVP_HIP(hipMemsetAsync(buf, 0, sizeof(FbHeader), s));
    FbHeader* hdr = static_cast<FbHeader*>(buf);
    const FbSlot slot{FbList{hdr, reinterpret_cast<unsigned*>(hdr + 1), 0}, new std::mutex};  // lives as long as the process
    lists[{dev, s}] = slot;
    return slot;
}

}  // namespace

void mvp::launch_triangulate_tol2(const float* kpts, int64_t n_points, int V, const double* cams, int n_cams,
                                  const int (&cam_idx)[kMaxCams], unsigned blocks, float* out_xyz,
                                  double* out_xyzw, hipStream_t s) {
    CamIdx ci;
    std::copy(cam_idx, cam_idx + kMaxCams, ci.v);
    const FbSlot slot = tol_fallback_list(s);
    std::lock_guard<std::mutex> call_lock(*slot.mu);
    FbList fb = slot.fb;
    const char* ff = getenv("MVPOSE_TRI_FORCE_FALLBACK");  // tests: exercise the fallback list / sweep
    // the float64 null vectors (out_xyzw, a diagnostic output) are the exact path's only
    // when it solves every point; the certification covers the f32 outputs
    fb.force = (ff && ff[0] == '1') || out_xyzw != nullptr;
    // 3 f32 + 2 fp64 undistortion iterations: 4 + 1 sends ~0.6 % of the synthetic rigs'
    // points to the exact path (0.013 % with 3 + 2, tools/tri_cert_emu.c)
    // 5 blocks of 4 waves per CU = the kernel's 5 waves per SIMD (88 VGPRs)
    const dim3 tgrid((unsigned)std::min<int64_t>(blocks, (int64_t)cu_count() * 5)), block(kBlock);
    hipLaunchKernelGGL(triangulate_tol2_kernel<3>, tgrid, block, 0, s, kpts, n_points, V, cams, n_cams, ci,
                       out_xyz, out_xyzw, fb);
    hipLaunchKernelGGL(triangulate_tol2_fallback_kernel, dim3(kFbBlocks), block, 0, s, kpts, n_points, V, cams,
                       n_cams, ci, out_xyz, out_xyzw, fb);
}

extern "C" int mvp_triangulate_fallback_total(void* stream, unsigned long long* out_total) {
    MVP_ABI_BEGIN
    MVP_REQUIRE(out_total != nullptr, "mvp_triangulate_fallback_total: out_total is NULL");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const FbSlot slot = tol_fallback_list(s);
    std::lock_guard<std::mutex> call_lock(*slot.mu);
    MVP_HIP(hipStreamSynchronize(s));
    MVP_HIP(hipMemcpy(out_total, &slot.fb.hdr->total, sizeof(unsigned long long), hipMemcpyDeviceToHost));
    MVP_ABI_END
}
