// The partition solver of the block-pentadiagonal chain systems (3x3 blocks), shared by the
// trajectory smoother (smooth.hip) and the trajectory fit (trajectory_fit.hip).  The algorithm,
// the workspace layout and the three sweeps (eliminate, reduce, backsub) are described at the top
// of smooth.hip; this header holds the per-lane code, templated on the frame source A:
//
//   A has the fields of SolveCore (by derivation or by name) and adds
//     Raw / Out                     what load_raw / load_out return (requested one step ahead)
//     kInfoForm                     false: frame_weight gives (W, z) and the rhs is W z;
//                                   true: it gives (W, b) in information form, the rhs is b
//     damp(p)                       the Marquardt factor (1 + mu_p) of the diagonal entries, or NoDamp
//     skip(p)                       the chain takes no part in this call (its lanes return)
//     load_raw(t, p), frame_weight(raw, W, z)     the eliminate sweep's frame
//     load_out(t, p), write_frame(t, p, out, x0, x1, x2), failed(p), write_failed(t, p)   backsub
//     finish(p, cnt, bad)           the end of the reduce: per-chain status
//
// A source that sets kKeepPivot = true and has the fields of CovCore gets the posterior covariance
// instead of the solution: eliminate_lane then also stores each frame's inverse pivot, and
// reduce_cov_chain / cov_lane (below) run the Takahashi recursion back over the same factors to
// the diagonal and lag-1 blocks of A⁻¹.  Such a source needs failed(p) and none of the backsub
// members.
//
// A source that sets kHasCross = true has a symmetric 3x3 data block between neighbouring frames
// as well (the trajectory fit with sub-frame camera offsets): cross(raw, C) gives the block between
// the frame before raw's and raw's own, zero for frame 0.  It belongs to the lane that owns the
// later frame of the pair, as a second-difference row belongs to the lane that owns its last frame,
// so every pair enters exactly one window, whether it lies inside a chunk, inside a separator or
// across the edge of one.  The other sources compile to what they were.
//
// The three kernels of a source are solve_eliminate_kernel<A>, solve_reduce_kernel<A> and
// solve_backsub_kernel<A> (below the per-lane code); bind_core fills a source's SolveCore fields
// from the plan.  The per-lane functions also compile for the host, where a CPU build can step
// through them.
#pragma once
// FMA contraction is allowed in everything below, whatever an earlier header left in force
// (refine_common.h turns it off at file scope).
#pragma clang fp contract(fast)
#include "mvp_common.h"

#include <cmath>
#include <cstdint>
#include <type_traits>
#include <utility>

#define MVP_SMOOTH_HD __host__ __device__ __forceinline__

namespace {

constexpr int kSmBlock = 64;         // threads per block: few lanes exist (P·n_chunks), spread them over CUs
constexpr int kFacDoubles = 39;      // per eliminated frame: G (12x3) | q (3)
constexpr int kSchurDoubles = 90;    // per lane: lower triangle of the 12x12 Schur complement (78) | rhs (12)
constexpr int kRedDoubles = 63;      // per separator and chain: C (21, lower, 1/diagonal) | Y (36) | y (6)
constexpr int kPivDoubles = 6;       // per eliminated frame of a covariance call: the inverse pivot (xx, xy, xz, yy, yz, zz)
constexpr int kCovRedDoubles = 57;   // per separator and chain: Σ_jj (21, lower) | Σ_j,j+1 (36, row: coordinate of j)
constexpr int kMinChunk = 4, kMaxChunk = 4096;

// What the three sweeps need whatever the frames come from.
struct SolveCore {
    int T, P, chunk, n_chunks, n_seps;
    int64_t n_lanes, n_blocks;
    double lambda;
    double* fac;    // [step][block][39][64]
    double* schur;  // [block][90][64]
    double* red;    // [sep][63][P]
    double* usol;   // [sep][6][P]
    int* cnt;       // [P] observed frames (zeroed before the eliminate launch)
    int* bad;       // [P] a pivot was not > 0 (zeroed likewise)
};

// What a covariance source adds to SolveCore.
struct CovCore {
    double* piv;        // [step][block][6][64]
    double* covred;     // [sep][57][P]
    float* out_cov;     // [T][P][6]
    float* out_cross;   // [T][P][9] or null
};

// A::kKeepPivot, false where the source has no such member.
template <class A, class = void>
struct keeps_pivot : std::false_type {};
template <class A>
struct keeps_pivot<A, std::enable_if_t<A::kKeepPivot>> : std::true_type {};

// A::kHasCross, likewise.
template <class A, class = void>
struct has_cross : std::false_type {};
template <class A>
struct has_cross<A, std::enable_if_t<A::kHasCross>> : std::true_type {};

MVP_SMOOTH_HD constexpr int tri(int i, int j) { return i * (i + 1) / 2 + j; }  // i >= j
MVP_SMOOTH_HD constexpr int sym(int i, int j) { return i >= j ? tri(i, j) : tri(j, i); }
// index of (d, e), d >= e, in a 3x3 kept as (xx, xy, xz, yy, yz, zz)
MVP_SMOOTH_HD constexpr int sym3(int d, int e) { return e == 0 ? d : e == 1 ? 2 + d : 5; }

// 1/sqrt(s), s > 0 and normal, to ~1 ulp: v_rsq_f64 + two Newton steps on the device (a sixth of
// the instructions of an fp64 sqrt followed by an fp64 division; every sweep step has six of them
// on its critical path).
MVP_SMOOTH_HD double inv_sqrt(double s) {
#ifdef __HIP_DEVICE_COMPILE__
    double y = __builtin_amdgcn_rsq(s);
    double t = s * y;
    double e = __builtin_fma(-t, y, 1.0);
    y = __builtin_fma(0.5 * y, e, y);
    t = s * y;
    e = __builtin_fma(-t, y, 1.0);
    return __builtin_fma(0.5 * y, e, y);
#else
    return 1.0 / sqrt(s);
#endif
}

// Inverse of the symmetric 3x3 s = (xx, xy, xz, yy, yz, zz) by Cholesky; false unless all three
// pivots are > 0 (NaN included).
MVP_SMOOTH_HD bool spd3_inverse(const double (&s)[6], double (&w)[6]) {
    const double d0 = s[0];
    const bool ok0 = d0 > 0;
    const double i00 = inv_sqrt(ok0 ? d0 : 1.0);
    const double l10 = s[1] * i00, l20 = s[2] * i00;
    const double d1 = s[3] - l10 * l10;
    const bool ok1 = d1 > 0;
    const double i11 = inv_sqrt(ok1 ? d1 : 1.0);
    const double l21 = (s[4] - l20 * l10) * i11;
    const double d2 = s[5] - l20 * l20 - l21 * l21;
    const bool ok2 = d2 > 0;
    const double i22 = inv_sqrt(ok2 ? d2 : 1.0);
    // L⁻¹, then W = L⁻ᵀ L⁻¹
    const double i10 = -l10 * i00 * i11;
    const double i21 = -l21 * i11 * i22;
    const double i20 = -(l20 * i00 + l21 * i10) * i22;
    w[0] = i00 * i00 + i10 * i10 + i20 * i20;
    w[1] = i10 * i11 + i20 * i21;
    w[2] = i20 * i22;
    w[3] = i11 * i11 + i21 * i21;
    w[4] = i21 * i22;
    w[5] = i22 * i22;
    return ok0 && ok1 && ok2;
}

// Workspace addressing: lanes in blocks of kSmBlock (one wave), [element][lane of the block] inside.
template <class A>
MVP_SMOOTH_HD int64_t fac_index(const A& a, int step, int64_t lane) {
    return (((int64_t)step * a.n_blocks + lane / kSmBlock) * kFacDoubles) * kSmBlock + lane % kSmBlock;
}
template <class A>
MVP_SMOOTH_HD int64_t piv_index(const A& a, int step, int64_t lane) {
    return (((int64_t)step * a.n_blocks + lane / kSmBlock) * kPivDoubles) * kSmBlock + lane % kSmBlock;
}
MVP_SMOOTH_HD int64_t schur_index(int64_t lane) {
    return (lane / kSmBlock) * kSchurDoubles * kSmBlock + lane % kSmBlock;
}

// The Marquardt factor of a diagonal entry: a compile-time 1 for a source that has none.
struct NoDamp {};
MVP_SMOOTH_HD double damped(double v, NoDamp) { return v; }
MVP_SMOOTH_HD double damped(double v, double damp) { return v * damp; }

// Data term of the frame in window block B: W onto its diagonal block (its diagonal entries times
// the Marquardt factor), and onto its rhs W z, or z itself when the source is in information form.
template <int B, bool INFO, class D>
MVP_SMOOTH_HD void add_data(double (&M)[120], double (&r)[15], const double (&W)[6], const double (&z)[3], D damp) {
    constexpr int o = 3 * B;
    M[tri(o, o)] += damped(W[0], damp);
    M[tri(o + 1, o)] += W[1];
    M[tri(o + 2, o)] += W[2];
    M[tri(o + 1, o + 1)] += damped(W[3], damp);
    M[tri(o + 2, o + 1)] += W[4];
    M[tri(o + 2, o + 2)] += damped(W[5], damp);
    if (INFO) {
        r[o] += z[0];
        r[o + 1] += z[1];
        r[o + 2] += z[2];
    } else {
        r[o] += W[0] * z[0] + W[1] * z[1] + W[2] * z[2];
        r[o + 1] += W[1] * z[0] + W[3] * z[1] + W[4] * z[2];
        r[o + 2] += W[2] * z[0] + W[4] * z[1] + W[5] * z[2];
    }
}

// λ v vᵀ ⊗ I₃ with v = (1, −2, 1) on window blocks B, B+1, B+2: one second-difference row (its
// diagonal entries times the Marquardt factor).
template <int B, class D>
MVP_SMOOTH_HD void add_element(double (&M)[120], double lam, D damp) {
    constexpr double v[3] = {1.0, -2.0, 1.0};
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j <= i; j++)
#pragma unroll
            for (int d = 0; d < 3; d++)
                M[tri(3 * (B + i) + d, 3 * (B + j) + d)] += i == j ? damped(lam * v[i] * v[j], damp) : lam * v[i] * v[j];
}

// The symmetric 3x3 data block C = (xx, xy, xz, yy, yz, zz) between window blocks B-1 and B (rows:
// the later frame).  Off the diagonal: no Marquardt factor.
template <int B>
MVP_SMOOTH_HD void add_cross(double (&M)[120], const double (&C)[6]) {
    constexpr int o = 3 * B;
#pragma unroll
    for (int d = 0; d < 3; d++)
#pragma unroll
        for (int e = 0; e < 3; e++) M[tri(o + d, o - 3 + e)] += C[d >= e ? sym3(d, e) : sym3(e, d)];
}

// The frames lane (chain p, chunk k) works on.
struct LaneRange {
    int p, k;
    int g0;  // first interior frame
    int n;   // interior frames (>= 1)
    int hi;  // end of the owned frames: interior + right separator (0, 1 or 2 frames)
};

template <class A>
MVP_SMOOTH_HD LaneRange lane_range(const A& a, int64_t lane) {
    LaneRange r;
    r.k = (int)(lane / a.P);
    r.p = (int)(lane - (int64_t)r.k * a.P);
    r.g0 = r.k * (a.chunk + 2);
    const int left = a.T - r.g0;
    r.n = left < a.chunk ? left : a.chunk;
    const int own = left < a.chunk + 2 ? left : a.chunk + 2;
    r.hi = r.g0 + own;
    return r;
}

// Window rows: 0..5 left separator (frames g0-2, g0-1), 6..8 frame a, 9..11 frame b, 12..14 frame c.
template <class A>
MVP_SMOOTH_HD void eliminate_lane(const A& a, int64_t lane) {
    const LaneRange R = lane_range(a, lane);
    if (a.skip(R.p)) return;
    const auto damp = a.damp(R.p);
    double M[120], r[15];
#pragma unroll
    for (int i = 0; i < 120; i++) M[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 15; i++) r[i] = 0.0;
    int cnt = 0;
    bool bad = false;
    double W[6], z[3];
    const bool has_b = R.g0 + 1 < R.hi;
    const typename A::Raw fa = a.load_raw(R.g0, R.p);
    const typename A::Raw fb = a.load_raw(has_b ? R.g0 + 1 : R.g0, R.p);
    typename A::Raw nxt = a.load_raw(R.g0 + 2 < R.hi ? R.g0 + 2 : R.g0, R.p);
    cnt += a.frame_weight(fa, W, z);
    add_data<2, A::kInfoForm>(M, r, W, z, damp);
    if (has_b) {
        cnt += a.frame_weight(fb, W, z);
        add_data<3, A::kInfoForm>(M, r, W, z, damp);
    }
    if constexpr (has_cross<A>::value) {
        // the pairs that end in frames a and b: (left separator, a) and (a, b)
        double X[6];
        if (R.k > 0) {
            a.cross(fa, X);
            add_cross<2>(M, X);
        }
        if (has_b) {
            a.cross(fb, X);
            add_cross<3>(M, X);
        }
    }
    if (R.k > 0) {
        add_element<0>(M, a.lambda, damp);
        if (has_b) add_element<1>(M, a.lambda, damp);
    }
    for (int i = 0; i < R.n; i++) {
        // frame c enters; the frame after it is requested now
        const int c = R.g0 + i + 2;
        const typename A::Raw fc = nxt;
        if (c + 1 < R.hi) nxt = a.load_raw(c + 1, R.p);
#pragma unroll
        for (int j = tri(12, 0); j < 120; j++) M[j] = 0.0;
        r[12] = r[13] = r[14] = 0.0;
        if (c < R.hi) {
            cnt += a.frame_weight(fc, W, z);
            add_data<4, A::kInfoForm>(M, r, W, z, damp);
            add_element<2>(M, a.lambda, damp);
            if constexpr (has_cross<A>::value) {
                double X[6];
                a.cross(fc, X);
                add_cross<4>(M, X);
            }
        }
        // frame a leaves: pivot P = M[a][a]
        const double s[6] = {M[tri(6, 6)], M[tri(7, 6)], M[tri(8, 6)], M[tri(7, 7)], M[tri(8, 7)], M[tri(8, 8)]};
        double Pi[6];
        bad = !spd3_inverse(s, Pi) || bad;
        const double q0 = Pi[0] * r[6] + Pi[1] * r[7] + Pi[2] * r[8];
        const double q1 = Pi[1] * r[6] + Pi[3] * r[7] + Pi[4] * r[8];
        const double q2 = Pi[2] * r[6] + Pi[4] * r[7] + Pi[5] * r[8];
        double* f = a.fac + fac_index(a, i, lane);
        double C[12][3], G[12][3];
#pragma unroll
        for (int o = 0; o < 12; o++) {
            const int row = o < 6 ? o : o + 3;
#pragma unroll
            for (int d = 0; d < 3; d++) C[o][d] = row < 6 ? M[tri(6 + d, row)] : M[tri(row, 6 + d)];
            G[o][0] = C[o][0] * Pi[0] + C[o][1] * Pi[1] + C[o][2] * Pi[2];
            G[o][1] = C[o][0] * Pi[1] + C[o][1] * Pi[3] + C[o][2] * Pi[4];
            G[o][2] = C[o][0] * Pi[2] + C[o][1] * Pi[4] + C[o][2] * Pi[5];
#pragma unroll
            for (int d = 0; d < 3; d++) f[(3 * o + d) * kSmBlock] = G[o][d];
        }
        f[36 * kSmBlock] = q0;
        f[37 * kSmBlock] = q1;
        f[38 * kSmBlock] = q2;
        if constexpr (keeps_pivot<A>::value) {
            double* pv = a.piv + piv_index(a, i, lane);
#pragma unroll
            for (int k = 0; k < kPivDoubles; k++) pv[k * kSmBlock] = Pi[k];
        }
        // Schur update of the 12 remaining rows, shifted into place: rows 9..14 move to 6..11
#pragma unroll
        for (int o = 0; o < 12; o++) {
            const int row = o < 6 ? o : o + 3;
#pragma unroll
            for (int u = 0; u <= o; u++) {
                const int col = u < 6 ? u : u + 3;
                M[tri(o, u)] = M[tri(row, col)] - (G[o][0] * C[u][0] + G[o][1] * C[u][1] + G[o][2] * C[u][2]);
            }
            r[o] = r[row] - (C[o][0] * q0 + C[o][1] * q1 + C[o][2] * q2);
        }
    }
    // the window's first 12 rows are now (left separator, right separator); a separator frame past
    // the end of the recording is decoupled: give it a unit diagonal so the reduced block stays SPD
#pragma unroll
    for (int q = 0; q < 2; q++)
        if (R.g0 + R.n + q >= a.T)
#pragma unroll
            for (int d = 0; d < 3; d++) M[tri(6 + 3 * q + d, 6 + 3 * q + d)] = 1.0;
    double* sc = a.schur + schur_index(lane);
#pragma unroll
    for (int i = 0; i < 78; i++) sc[i * kSmBlock] = M[i];
#pragma unroll
    for (int i = 0; i < 12; i++) sc[(78 + i) * kSmBlock] = r[i];
#ifdef __HIP_DEVICE_COMPILE__
    if (cnt) atomicAdd(&a.cnt[R.p], cnt);
    if (bad) atomicOr(&a.bad[R.p], 1);
#else
    a.cnt[R.p] += cnt;
    a.bad[R.p] |= bad ? 1 : 0;
#endif
}

// What the reduce phase reads for separator j of chain p, 90 doubles: the right-separator corner
// of chunk j's Schur complement (21) and rhs (6), the left-separator corner of chunk j+1's (21)
// and rhs (6), and E (36), the coupling to separator j+1 (row: coordinate of j, column: of j+1).
constexpr int kInRR = 0, kInGR = 21, kInLL = 27, kInGL = 48, kInE = 54, kInDoubles = 90;

template <class A>
MVP_SMOOTH_HD void load_reduce_in(const A& a, int p, int j, double (&v)[kInDoubles]) {
    const double* s0 = a.schur + schur_index((int64_t)j * a.P + p);
    const bool has_next = j + 1 < a.n_chunks, has_e = j + 1 < a.n_seps;
    const double* s1 = a.schur + schur_index((int64_t)(has_next ? j + 1 : j) * a.P + p);
#pragma unroll
    for (int i = 0; i < 6; i++) {
#pragma unroll
        for (int u = 0; u <= i; u++) {
            v[kInRR + tri(i, u)] = s0[tri(6 + i, 6 + u) * kSmBlock];
            v[kInLL + tri(i, u)] = has_next ? s1[tri(i, u) * kSmBlock] : 0.0;
        }
        v[kInGR + i] = s0[(78 + 6 + i) * kSmBlock];
        v[kInGL + i] = has_next ? s1[(78 + i) * kSmBlock] : 0.0;
#pragma unroll
        for (int u = 0; u < 6; u++) v[kInE + 6 * i + u] = has_e ? s1[tri(6 + u, i) * kSmBlock] : 0.0;
    }
}

// One chain's reduced system, forward then back, everything in registers (fully unrolled; the
// 6x6 blocks are packed lower triangles).
template <class A>
MVP_SMOOTH_HD void reduce_chain(const A& a, int p) {
    if (a.skip(p)) return;
    int bad = a.bad[p];
    const int ns = a.n_seps;
    double in[kInDoubles];
    double Yp[36], yp[6];   // Y, y of separator j-1 (0 in front of the first)
#pragma unroll
    for (int i = 0; i < 36; i++) Yp[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 6; i++) yp[i] = 0.0;
    if (ns > 0) load_reduce_in(a, p, 0, in);
    for (int j = 0; j < ns; j++) {
        // D = right-separator part of chunk j + left-separator part of chunk j+1 - Yᵀ Y of separator j-1
        double D[21], g[6], Y[36];
#pragma unroll
        for (int i = 0; i < 6; i++) {
#pragma unroll
            for (int u = 0; u <= i; u++) {
                double d = in[kInRR + tri(i, u)] + in[kInLL + tri(i, u)];
#pragma unroll
                for (int m = 0; m < 6; m++) d -= Yp[6 * m + i] * Yp[6 * m + u];
                D[tri(i, u)] = d;
            }
            double e = in[kInGR + i] + in[kInGL + i];
#pragma unroll
            for (int m = 0; m < 6; m++) e -= Yp[6 * m + i] * yp[m];
            g[i] = e;
        }
#pragma unroll
        for (int i = 0; i < 36; i++) Y[i] = in[kInE + i];
        if (j + 1 < ns) load_reduce_in(a, p, j + 1, in);   // requested now, used in the next step
        // Cholesky D = C Cᵀ in place; the diagonal keeps 1 / C_ii
#pragma unroll
        for (int i = 0; i < 6; i++) {
#pragma unroll
            for (int u = 0; u <= i; u++) {
                double d = D[tri(i, u)];
#pragma unroll
                for (int m = 0; m < u; m++) d -= D[tri(i, m)] * D[tri(u, m)];
                if (u < i) {
                    D[tri(i, u)] = d * D[tri(u, u)];
                } else {
                    const bool ok = d > 0;
                    bad = ok ? bad : 1;
                    D[tri(i, i)] = inv_sqrt(ok ? d : 1.0);
                }
            }
        }
        // Y = C⁻¹ E, y = C⁻¹ g
#pragma unroll
        for (int i = 0; i < 6; i++) {
#pragma unroll
            for (int u = 0; u < 6; u++) {
                double d = Y[6 * i + u];
#pragma unroll
                for (int m = 0; m < i; m++) d -= D[tri(i, m)] * Y[6 * m + u];
                Y[6 * i + u] = d * D[tri(i, i)];
            }
            double e = g[i];
#pragma unroll
            for (int m = 0; m < i; m++) e -= D[tri(i, m)] * g[m];
            g[i] = e * D[tri(i, i)];
        }
        double* rd = a.red + ((int64_t)j * kRedDoubles) * a.P + p;
#pragma unroll
        for (int i = 0; i < 21; i++) rd[(int64_t)i * a.P] = D[i];
#pragma unroll
        for (int i = 0; i < 36; i++) {
            rd[(int64_t)(21 + i) * a.P] = Y[i];
            Yp[i] = Y[i];
        }
#pragma unroll
        for (int i = 0; i < 6; i++) {
            rd[(int64_t)(57 + i) * a.P] = g[i];
            yp[i] = g[i];
        }
    }
    // back: u_j = C⁻ᵀ (y − Y u_{j+1}), in registers, separator j-1's factor requested while j is solved
    double u[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double cur[kRedDoubles], nxt[kRedDoubles];
    if (ns > 0) {
        const double* rd = a.red + ((int64_t)(ns - 1) * kRedDoubles) * a.P + p;
#pragma unroll
        for (int i = 0; i < kRedDoubles; i++) cur[i] = rd[(int64_t)i * a.P];
    }
    for (int j = ns - 1; j >= 0; j--) {
        if (j > 0) {
            const double* rd = a.red + ((int64_t)(j - 1) * kRedDoubles) * a.P + p;
#pragma unroll
            for (int i = 0; i < kRedDoubles; i++) nxt[i] = rd[(int64_t)i * a.P];
        }
        double v[6];
#pragma unroll
        for (int i = 0; i < 6; i++) {
            double d = cur[57 + i];
#pragma unroll
            for (int m = 0; m < 6; m++) d -= cur[21 + 6 * i + m] * u[m];
            v[i] = d;
        }
#pragma unroll
        for (int i = 5; i >= 0; i--) {
            double d = v[i];
#pragma unroll
            for (int m = i + 1; m < 6; m++) d -= cur[tri(m, i)] * u[m];
            u[i] = d * cur[tri(i, i)];
        }
        double* us = a.usol + ((int64_t)j * 6) * a.P + p;
#pragma unroll
        for (int i = 0; i < 6; i++) us[(int64_t)i * a.P] = u[i];
        if (j > 0) {
#pragma unroll
            for (int i = 0; i < kRedDoubles; i++) cur[i] = nxt[i];
        }
    }
    a.finish(p, a.cnt[p], bad);
}

template <class A>
MVP_SMOOTH_HD void backsub_lane(const A& a, int64_t lane) {
    const LaneRange R = lane_range(a, lane);
    if (a.skip(R.p)) return;
    if (a.failed(R.p)) {
        for (int t = R.g0; t < R.hi; t++) a.write_failed(t, R.p);
        return;
    }
    // x: 0..5 left separator, 6..11 frames b, c (the right separator to start with)
    double x[12];
#pragma unroll
    for (int i = 0; i < 12; i++) x[i] = 0.0;
    if (R.k > 0) {
        const double* us = a.usol + ((int64_t)(R.k - 1) * 6) * a.P + R.p;
#pragma unroll
        for (int i = 0; i < 6; i++) x[i] = us[(int64_t)i * a.P];
    }
    if (R.k < a.n_seps) {
        const double* us = a.usol + ((int64_t)R.k * 6) * a.P + R.p;
#pragma unroll
        for (int i = 0; i < 6; i++) x[6 + i] = us[(int64_t)i * a.P];
    }
    for (int q = 0; q < 2; q++)
        if (R.g0 + R.n + q < R.hi)
            a.write_frame(R.g0 + R.n + q, R.p, a.load_out(R.g0 + R.n + q, R.p), x[6 + 3 * q], x[7 + 3 * q], x[8 + 3 * q]);
    // the factor and the input frame of step i-1 are requested while step i is solved
    double fc[kFacDoubles], fn[kFacDoubles];
    typename A::Out rc = a.load_out(R.g0 + R.n - 1, R.p), rn = rc;
    {
        const double* f = a.fac + fac_index(a, R.n - 1, lane);
#pragma unroll
        for (int k = 0; k < kFacDoubles; k++) fc[k] = f[k * kSmBlock];
    }
    for (int i = R.n - 1; i >= 0; i--) {
        if (i > 0) {
            const double* f = a.fac + fac_index(a, i - 1, lane);
#pragma unroll
            for (int k = 0; k < kFacDoubles; k++) fn[k] = f[k * kSmBlock];
            rn = a.load_out(R.g0 + i - 1, R.p);
        }
        double xa[3];
#pragma unroll
        for (int d = 0; d < 3; d++) xa[d] = fc[36 + d];
#pragma unroll
        for (int o = 0; o < 12; o++)
#pragma unroll
            for (int d = 0; d < 3; d++) xa[d] -= fc[3 * o + d] * x[o];
        a.write_frame(R.g0 + i, R.p, rc, xa[0], xa[1], xa[2]);
#pragma unroll
        for (int d = 0; d < 3; d++) {
            x[9 + d] = x[6 + d];
            x[6 + d] = xa[d];
        }
        if (i > 0) {
#pragma unroll
            for (int k = 0; k < kFacDoubles; k++) fc[k] = fn[k];
            rc = rn;
        }
    }
}

// ----------------------------------------------------------------- posterior covariance
// Σ = A⁻¹ by the Takahashi recursion over the factors of eliminate_lane and reduce_chain, in their
// elimination order backwards: the separators first (reduce_cov_chain), then every chunk's
// interior (cov_lane).  Every symmetric block is a packed lower triangle from the moment it is
// formed: a 3x3 Π + GᵀΣG kept as a full matrix carries an antisymmetric rounding residue that the
// recursion doubles per frame.

// The selected inverse of chain p's reduced system: with D_j = C_j C_jᵀ, Y_j = C_j⁻¹ E_j and
// Z_j = C_j⁻ᵀ Y_j,  Σ_last,last = C⁻ᵀ C⁻¹,  Σ_j,j+1 = −Z_j Σ_j+1,j+1,
// Σ_j,j = C_j⁻ᵀ C_j⁻¹ + Z_j Σ_j+1,j+1 Z_jᵀ.  Runs behind reduce_chain (same lane: it reads red and
// the chain's status).
template <class A>
MVP_SMOOTH_HD void reduce_cov_chain(const A& a, int p) {
    const int ns = a.n_seps;
    if (ns == 0 || a.failed(p)) return;
    constexpr int kIn = 57;   // C | Y of red
    double S[21], cur[kIn], nxt[kIn];
    {
        const double* rd = a.red + ((int64_t)(ns - 1) * kRedDoubles) * a.P + p;
#pragma unroll
        for (int i = 0; i < kIn; i++) cur[i] = rd[(int64_t)i * a.P];
    }
#pragma unroll
    for (int i = 0; i < 21; i++) S[i] = 0.0;
    for (int j = ns - 1; j >= 0; j--) {
        if (j > 0) {
            const double* rd = a.red + ((int64_t)(j - 1) * kRedDoubles) * a.P + p;
#pragma unroll
            for (int i = 0; i < kIn; i++) nxt[i] = rd[(int64_t)i * a.P];
        }
        // Ci = C⁻¹ (lower), W = Ciᵀ Ci
        double Ci[21], W[21];
#pragma unroll
        for (int i = 0; i < 6; i++) {
            Ci[tri(i, i)] = cur[tri(i, i)];
#pragma unroll
            for (int u = 0; u < i; u++) {
                double d = 0.0;
#pragma unroll
                for (int m = u; m < i; m++) d += cur[tri(i, m)] * Ci[tri(m, u)];
                Ci[tri(i, u)] = -d * cur[tri(i, i)];
            }
        }
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int u = 0; u <= i; u++) {
                double d = 0.0;
#pragma unroll
                for (int m = i; m < 6; m++) d += Ci[tri(m, i)] * Ci[tri(m, u)];
                W[tri(i, u)] = d;
            }
        double* cr = a.covred + ((int64_t)j * kCovRedDoubles) * a.P + p;
        if (j + 1 < ns) {
            double Z[36], X[36];
#pragma unroll
            for (int i = 0; i < 6; i++)
#pragma unroll
                for (int u = 0; u < 6; u++) {
                    double d = 0.0;
#pragma unroll
                    for (int m = i; m < 6; m++) d += Ci[tri(m, i)] * cur[21 + 6 * m + u];
                    Z[6 * i + u] = d;
                }
#pragma unroll
            for (int i = 0; i < 6; i++)
#pragma unroll
                for (int u = 0; u < 6; u++) {
                    double d = 0.0;
#pragma unroll
                    for (int m = 0; m < 6; m++) d += Z[6 * i + m] * S[sym(m, u)];
                    X[6 * i + u] = d;
                    cr[(int64_t)(21 + 6 * i + u) * a.P] = -d;
                }
#pragma unroll
            for (int i = 0; i < 6; i++)
#pragma unroll
                for (int u = 0; u <= i; u++) {
                    double d = W[tri(i, u)];
#pragma unroll
                    for (int m = 0; m < 6; m++) d += X[6 * i + m] * Z[6 * u + m];
                    W[tri(i, u)] = d;
                }
        }
#pragma unroll
        for (int i = 0; i < 21; i++) {
            S[i] = W[i];
            cr[(int64_t)i * a.P] = W[i];
        }
        if (j > 0) {
#pragma unroll
            for (int i = 0; i < kIn; i++) cur[i] = nxt[i];
        }
    }
}

// Σ_t,t of frame (t, p) from a packed block; rows o.. of S, or the 3x3 form of the pivot.
template <class A>
MVP_SMOOTH_HD void put_cov(const A& a, int t, int p, double xx, double xy, double xz, double yy, double yz, double zz) {
    float* o = a.out_cov + 6 * ((int64_t)t * a.P + p);
    o[0] = (float)xx, o[1] = (float)xy, o[2] = (float)xz, o[3] = (float)yy, o[4] = (float)yz, o[5] = (float)zz;
}

// Σ_t,t+1 of frame (t, p), row-major (row: coordinate of X_t); NaN for the last frame.
template <class A>
MVP_SMOOTH_HD void put_cross(const A& a, int t, int p, const double (&c)[9]) {
    if (!a.out_cross) return;
    float* o = a.out_cross + 9 * ((int64_t)t * a.P + p);
    const bool last = t == a.T - 1;
#pragma unroll
    for (int k = 0; k < 9; k++) o[k] = last ? NAN : (float)c[k];
}

// One lane per (chain, chunk), as backsub_lane: where that carries the solution on (left
// separator, b, c), this carries Σ on them, a packed 12x12.  Per frame a, from the last interior
// frame back:  Σ_N,a = −Σ_N,N G,  Σ_a,a = Π + Gᵀ Σ_N,N G,  then the window shifts to (L, a, b).
// The lane writes Σ_t,t of the frames it owns and Σ_t,t+1 of every pair it holds in one window:
// its interior frames, the first frame of its right separator, and the frame in front of its first
// interior frame; the second separator frame's only when it ends the recording (NaN).
template <class A>
MVP_SMOOTH_HD void cov_lane(const A& a, int64_t lane) {
    const LaneRange R = lane_range(a, lane);
    const int p = R.p;
    if (a.failed(p)) {
        const double nan9[9] = {NAN, NAN, NAN, NAN, NAN, NAN, NAN, NAN, NAN};
        for (int t = R.g0; t < R.hi; t++) put_cov(a, t, p, NAN, NAN, NAN, NAN, NAN, NAN);
        for (int t = R.k > 0 ? R.g0 - 1 : R.g0; t < R.hi; t++)
            if (t != R.g0 + R.n + 1 || t == a.T - 1) put_cross(a, t, p, nan9);
        return;
    }
    // S: 0..5 left separator, 6..11 frames b, c (the right separator to start with)
    double S[78];
#pragma unroll
    for (int i = 0; i < 78; i++) S[i] = 0.0;
    const bool has_l = R.k > 0, has_r = R.k < a.n_seps;
    if (has_l) {
        const double* cr = a.covred + ((int64_t)(R.k - 1) * kCovRedDoubles) * a.P + p;
#pragma unroll
        for (int i = 0; i < 21; i++) S[i] = cr[(int64_t)i * a.P];
        if (has_r) {
#pragma unroll
            for (int i = 0; i < 6; i++)
#pragma unroll
                for (int u = 0; u < 6; u++) S[tri(6 + i, u)] = cr[(int64_t)(21 + 6 * u + i) * a.P];
        }
    }
    if (has_r) {
        const double* cr = a.covred + ((int64_t)R.k * kCovRedDoubles) * a.P + p;
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int u = 0; u <= i; u++) S[tri(6 + i, 6 + u)] = cr[(int64_t)tri(i, u) * a.P];
    }
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const int t = R.g0 + R.n + q;
        if (t < R.hi) {
            const int o = 6 + 3 * q;
            put_cov(a, t, p, S[tri(o, o)], S[tri(o + 1, o)], S[tri(o + 2, o)], S[tri(o + 1, o + 1)], S[tri(o + 2, o + 1)],
                    S[tri(o + 2, o + 2)]);
            if (q == 0 || t == a.T - 1) {
                double c[9];
#pragma unroll
                for (int r = 0; r < 3; r++)
#pragma unroll
                    for (int u = 0; u < 3; u++) c[3 * r + u] = S[tri(9 + u, 6 + r)];
                put_cross(a, t, p, c);
            }
        }
    }
    // the factor and the pivot of step i-1 are requested while step i is worked on
    double G[36], Pi[kPivDoubles], Gn[36], Pn[kPivDoubles];
    {
        const double* f = a.fac + fac_index(a, R.n - 1, lane);
        const double* pv = a.piv + piv_index(a, R.n - 1, lane);
#pragma unroll
        for (int k = 0; k < 36; k++) G[k] = f[k * kSmBlock];
#pragma unroll
        for (int k = 0; k < kPivDoubles; k++) Pi[k] = pv[k * kSmBlock];
    }
    for (int i = R.n - 1; i >= 0; i--) {
        if (i > 0) {
            const double* f = a.fac + fac_index(a, i - 1, lane);
            const double* pv = a.piv + piv_index(a, i - 1, lane);
#pragma unroll
            for (int k = 0; k < 36; k++) Gn[k] = f[k * kSmBlock];
#pragma unroll
            for (int k = 0; k < kPivDoubles; k++) Pn[k] = pv[k * kSmBlock];
        }
        // V = Σ_N,N G  (= −Σ_N,a)
        double V[36];
#pragma unroll
        for (int o = 0; o < 12; o++)
#pragma unroll
            for (int d = 0; d < 3; d++) {
                double v = 0.0;
#pragma unroll
                for (int u = 0; u < 12; u++) v += S[sym(o, u)] * G[3 * u + d];
                V[3 * o + d] = v;
            }
        double Saa[6];
#pragma unroll
        for (int d = 0; d < 3; d++)
#pragma unroll
            for (int e = 0; e <= d; e++) {
                double v = Pi[sym3(d, e)];
#pragma unroll
                for (int o = 0; o < 12; o++) v += G[3 * o + d] * V[3 * o + e];
                Saa[sym3(d, e)] = v;
            }
        const int t = R.g0 + i;
        put_cov(a, t, p, Saa[0], Saa[1], Saa[2], Saa[3], Saa[4], Saa[5]);
        {
            double c[9];
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int u = 0; u < 3; u++) c[3 * r + u] = -V[3 * (6 + u) + r];
            put_cross(a, t, p, c);
        }
        if (i == 0 && has_l) {
            double c[9];
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int u = 0; u < 3; u++) c[3 * r + u] = -V[3 * (3 + r) + u];
            put_cross(a, t - 1, p, c);
        }
        // the window shifts to (L, a, b): rows 6..8 move to 9..11, frame a takes 6..8
#pragma unroll
        for (int d = 0; d < 3; d++) {
#pragma unroll
            for (int u = 0; u < 6; u++) S[tri(9 + d, u)] = S[tri(6 + d, u)];
#pragma unroll
            for (int e = 0; e <= d; e++) S[tri(9 + d, 9 + e)] = S[tri(6 + d, 6 + e)];
        }
#pragma unroll
        for (int d = 0; d < 3; d++) {
#pragma unroll
            for (int u = 0; u < 6; u++) S[tri(6 + d, u)] = -V[3 * u + d];
#pragma unroll
            for (int e = 0; e <= d; e++) S[tri(6 + d, 6 + e)] = Saa[sym3(d, e)];
#pragma unroll
            for (int e = 0; e < 3; e++) S[tri(9 + d, 6 + e)] = -V[3 * (6 + d) + e];
        }
        if (i > 0) {
#pragma unroll
            for (int k = 0; k < 36; k++) G[k] = Gn[k];
#pragma unroll
            for (int k = 0; k < kPivDoubles; k++) Pi[k] = Pn[k];
        }
    }
}

// ----------------------------------------------------------------- kernels
// The three launches of a source A: one lane per (chain, chunk), per chain, per (chain, chunk).  A
// source that keeps its pivots has the reduced system's selected inverse behind its reduce and the
// covariance sweep for its third launch.
template <class A>
__global__ __launch_bounds__(kSmBlock) void solve_eliminate_kernel(A a) {
    const int64_t lane = (int64_t)blockIdx.x * kSmBlock + threadIdx.x;
    if (lane < a.n_lanes) eliminate_lane(a, lane);
}

template <class A>
__global__ __launch_bounds__(kSmBlock) void solve_reduce_kernel(A a) {
    const int p = blockIdx.x * kSmBlock + threadIdx.x;
    if (p < a.P) {
        reduce_chain(a, p);
        if constexpr (keeps_pivot<A>::value) reduce_cov_chain(a, p);
    }
}

template <class A>
__global__ __launch_bounds__(kSmBlock) void solve_backsub_kernel(A a) {
    const int64_t lane = (int64_t)blockIdx.x * kSmBlock + threadIdx.x;
    if (lane < a.n_lanes) {
        if constexpr (keeps_pivot<A>::value)
            cov_lane(a, lane);
        else
            backsub_lane(a, lane);
    }
}

// ----------------------------------------------------------------- host side
struct SmoothPlan {
    int chunk, n_chunks, n_seps, steps;
    int64_t n_lanes, n_blocks;
    int64_t off_fac, off_schur, off_red, off_usol, off_cnt, off_bad, off_fail, bytes;
};

inline int64_t align256(int64_t b) { return (b + 255) / 256 * 256; }

// chunk = 0: the automatic rule ("Trajectory smoothing": the sweep it comes from).
// A lane's two sweeps cost about 2·chunk steps, the serial reduce one longer step per separator,
// T / chunk of them: the minimum lies at a multiple of sqrt(T), 1.25 on the MI355X.
inline int auto_chunk(int T) {
    int c = (int)lround(1.25 * sqrt((double)T));
    return c < kMinChunk ? kMinChunk : c > kMaxChunk ? kMaxChunk : c;
}

inline SmoothPlan smooth_plan(const char* fn, int T, int P, int chunk) {
    MVP_REQUIRE(T >= 1, "%s: T=%d < 1", fn, T);
    MVP_REQUIRE(P >= 1, "%s: P=%d < 1", fn, P);
    MVP_REQUIRE(chunk == 0 || (chunk >= kMinChunk && chunk <= kMaxChunk), "%s: chunk=%d (0 = automatic, or %d..%d)", fn,
                chunk, kMinChunk, kMaxChunk);
    SmoothPlan pl;
    pl.chunk = chunk == 0 ? auto_chunk(T) : chunk;
    const int period = pl.chunk + 2;
    pl.n_chunks = (T + period - 1) / period;
    pl.n_seps = T > pl.chunk ? (T - pl.chunk - 1) / period + 1 : 0;
    pl.steps = T < pl.chunk ? T : pl.chunk;
    pl.n_lanes = (int64_t)P * pl.n_chunks;
    pl.n_blocks = (pl.n_lanes + kSmBlock - 1) / kSmBlock;
    MVP_REQUIRE(pl.n_blocks < (1LL << 31), "%s: too many lanes (T=%d, P=%d)", fn, T, P);
    int64_t b = 0;
    pl.off_fac = b;
    b = align256(b + (int64_t)pl.steps * pl.n_blocks * kFacDoubles * kSmBlock * 8);
    pl.off_schur = b;
    b = align256(b + pl.n_blocks * kSchurDoubles * kSmBlock * 8);
    pl.off_red = b;
    b = align256(b + (int64_t)pl.n_seps * kRedDoubles * P * 8);
    pl.off_usol = b;
    b = align256(b + (int64_t)pl.n_seps * 6 * P * 8);
    pl.off_cnt = b;   // cnt and bad lie together: one memset zeroes both
    b += (int64_t)P * 4;
    pl.off_bad = b;
    b = align256(b + (int64_t)P * 4);
    pl.off_fail = b;
    b = align256(b + (int64_t)P * 4);
    pl.bytes = b;
    return pl;
}

// What a covariance call adds behind `base` bytes of its solver's workspace.
struct CovPlan {
    int64_t off_piv, off_covred, bytes;
};

inline CovPlan cov_plan(const SmoothPlan& sp, int P, int64_t base) {
    CovPlan cp;
    int64_t b = base;
    cp.off_piv = b;
    b = align256(b + (int64_t)sp.steps * sp.n_blocks * kPivDoubles * kSmBlock * 8);
    cp.off_covred = b;
    b = align256(b + (int64_t)sp.n_seps * kCovRedDoubles * P * 8);
    cp.bytes = b;
    return cp;
}

template <class A, class = void>
struct has_fail : std::false_type {};
template <class A>
struct has_fail<A, std::void_t<decltype(std::declval<A&>().fail)>> : std::true_type {};

// The fields of SolveCore in a source, over the workspace ws of plan sp; with them the source's
// fail, where it has one.
template <class A>
inline void bind_core(A& a, char* ws, const SmoothPlan& sp, int T, int P, double lambda) {
    a.T = T, a.P = P, a.chunk = sp.chunk, a.n_chunks = sp.n_chunks, a.n_seps = sp.n_seps;
    a.n_lanes = sp.n_lanes, a.n_blocks = sp.n_blocks;
    a.lambda = lambda;
    a.fac = reinterpret_cast<double*>(ws + sp.off_fac);
    a.schur = reinterpret_cast<double*>(ws + sp.off_schur);
    a.red = reinterpret_cast<double*>(ws + sp.off_red);
    a.usol = reinterpret_cast<double*>(ws + sp.off_usol);
    a.cnt = reinterpret_cast<int*>(ws + sp.off_cnt);
    a.bad = reinterpret_cast<int*>(ws + sp.off_bad);
    if constexpr (has_fail<A>::value) a.fail = reinterpret_cast<int*>(ws + sp.off_fail);
}

// What a covariance source adds, over the same workspace.
inline void bind_cov(CovCore& a, char* ws, const CovPlan& cp, float* out_cov, float* out_cross) {
    a.piv = reinterpret_cast<double*>(ws + cp.off_piv);
    a.covred = reinterpret_cast<double*>(ws + cp.off_covred);
    a.out_cov = out_cov;
    a.out_cross = out_cross;
}

}  // namespace
