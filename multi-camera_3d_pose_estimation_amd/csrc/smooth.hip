// Covariance-weighted trajectory smoothing with gap filling (mvp_trajectory_smooth; the problem
// is stated in include/mvpose.h; no reference counterpart) for gfx950.
//
// Per chain p the minimiser of
//   ½ Σ_t (X_t − z_t)ᵀ W_t (X_t − z_t) + ½ λ Σ_t |X_t − 2 X_{t−1} + X_{t−2}|²
// solves a symmetric block-pentadiagonal system (3x3 blocks) in T unknowns.  A recording has
// only P = 17 chains, so the solve is parallel in time by the partition (substructuring)
// method: the frames are cut into chunks of `chunk` interior frames with 2-frame separators
// between them (period chunk + 2).  The matrix couples t only with t±1, t±2, so a separator
// decouples its two sides.  Three stream-ordered launches, everything fp64:
//
//   eliminate  one lane per (chain, chunk).  The lane owns its interior frames, the separator
//              to its right (its data terms) and every second-difference row that touches its
//              interior.  It keeps a window [left separator (6) | frames a, b, c (9)] of the
//              matrix, 15x15 symmetric plus right-hand side, in registers; per step frame c
//              enters (its W built on the fly from the covariance, the second-difference row
//              (a, b, c) added), frame a is eliminated by its 3x3 Cholesky pivot, and the
//              window shifts.  The left separator stays in the window for the whole sweep,
//              so when the interior is used up the window IS the chunk's Schur complement on
//              (left separator, right separator): the four corner blocks of the interior
//              inverse come out of the one sweep, no extra right-hand sides.  Per eliminated
//              frame 39 doubles go to the workspace: the 12x3 multipliers and P⁻¹·rhs.
//   reduce     one lane per chain: assembles the block-tridiagonal (6x6) separator system
//              from the chunks' Schur complements, solves it by block Cholesky (in registers,
//              fully unrolled; the next separator's 90 inputs are requested while this one is
//              factorised), and writes the per-chain status from the
//              observed-frame counts and pivot flags the eliminate lanes have added up.
//   backsub    one lane per (chain, chunk): x_a = P⁻¹ rhs − Gᵀ x_window, from the last interior
//              frame back to the first, then xyz / resid / observed; failed chains get their
//              input bits back.
//
// Lanes run along p first, then along chunks.  The per-lane workspace arrays are [step][wave]
// [element][lane of the wave], so a wave-instruction touches 512 contiguous aligned bytes and a
// wave's whole sweep step one contiguous piece.  Every sweep loads what its next step needs
// (input frame, factor) one step ahead.  FMA contraction is allowed (no bit contract).
// Register / LDS / scratch figures and the measurements are in DESIGN.md.
#include "mvp_common.h"

#include <cmath>
#include <cstdint>

// The per-lane functions also compile for the host, where a CPU build can step through them.
#define MVP_SMOOTH_HD __host__ __device__ __forceinline__

namespace {

constexpr int kSmBlock = 64;         // threads per block: few lanes exist (P·n_chunks), spread them over CUs
constexpr int kFacDoubles = 39;      // per eliminated frame: G (12x3) | q (3)
constexpr int kSchurDoubles = 90;    // per lane: lower triangle of the 12x12 Schur complement (78) | rhs (12)
constexpr int kRedDoubles = 63;      // per separator and chain: C (21, lower, 1/diagonal) | Y (36) | y (6)
constexpr int kMinChunk = 4, kMaxChunk = 4096;

struct SmoothArgs {
    const float* xyz;
    const float* cov;
    const uint8_t* valid;
    int T, P, chunk, n_chunks, n_seps;
    int64_t n_lanes, n_blocks;
    double lambda, w0, cov_floor;
    double* fac;    // [step][block][39][64]
    double* schur;  // [block][90][64]
    double* red;    // [sep][63][P]
    double* usol;   // [sep][6][P]
    int* cnt;       // [P] observed frames (zeroed before the eliminate launch)
    int* bad;       // [P] a pivot was not > 0 (zeroed likewise)
    int* fail;      // [P]
    float* out_xyz;
    float* out_resid;
    uint8_t* out_observed;
    uint8_t* out_status;
};

MVP_SMOOTH_HD constexpr int tri(int i, int j) { return i * (i + 1) / 2 + j; }  // i >= j

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

// The bytes of frame (t, p) as they lie in memory: loaded one sweep step ahead of their use, so
// that the step does not wait for them.
struct RawFrame {
    float x[3], c[6];
    uint8_t v;
};

MVP_SMOOTH_HD RawFrame load_raw(const SmoothArgs& a, int t, int p) {
    const int64_t e = (int64_t)t * a.P + p;
    RawFrame f;
#pragma unroll
    for (int k = 0; k < 3; k++) f.x[k] = a.xyz[3 * e + k];
#pragma unroll
    for (int k = 0; k < 6; k++) f.c[k] = a.cov ? a.cov[6 * e + k] : 0.f;
    f.v = a.valid ? a.valid[e] : 1;
    return f;
}

// Frame f: observed? its weight W (6, upper triangle) and measurement z.  W = 0 when not
// observed, and the coordinates are then never used.
MVP_SMOOTH_HD bool frame_weight(const SmoothArgs& a, const RawFrame& f, double (&W)[6], double (&z)[3]) {
    const float x0 = f.x[0], x1 = f.x[1], x2 = f.x[2];
    bool obs = __builtin_isfinite(x0) && __builtin_isfinite(x1) && __builtin_isfinite(x2);
    obs = obs && f.v != 0;
    if (a.cov) {
        double s[6];
        bool fin = true;
#pragma unroll
        for (int k = 0; k < 6; k++) {
            const float c = f.c[k];
            fin = fin && __builtin_isfinite(c);
            s[k] = (double)c;
        }
        s[0] += a.cov_floor;
        s[3] += a.cov_floor;
        s[5] += a.cov_floor;
        const bool pd = spd3_inverse(s, W);
        obs = obs && fin && pd;
    } else {
        W[0] = W[3] = W[5] = a.w0;
        W[1] = W[2] = W[4] = 0.0;
    }
#pragma unroll
    for (int k = 0; k < 6; k++) W[k] = obs ? W[k] : 0.0;
    z[0] = obs ? (double)x0 : 0.0;
    z[1] = obs ? (double)x1 : 0.0;
    z[2] = obs ? (double)x2 : 0.0;
    return obs;
}

// Workspace addressing: lanes in blocks of kSmBlock (one wave), [element][lane of the block] inside.
MVP_SMOOTH_HD int64_t fac_index(const SmoothArgs& a, int step, int64_t lane) {
    return (((int64_t)step * a.n_blocks + lane / kSmBlock) * kFacDoubles) * kSmBlock + lane % kSmBlock;
}
MVP_SMOOTH_HD int64_t schur_index(int64_t lane) {
    return (lane / kSmBlock) * kSchurDoubles * kSmBlock + lane % kSmBlock;
}

// Data term of the frame in window block B: W onto its diagonal block, W z onto its rhs.
template <int B>
MVP_SMOOTH_HD void add_data(double (&M)[120], double (&r)[15], const double (&W)[6], const double (&z)[3]) {
    constexpr int o = 3 * B;
    M[tri(o, o)] += W[0];
    M[tri(o + 1, o)] += W[1];
    M[tri(o + 2, o)] += W[2];
    M[tri(o + 1, o + 1)] += W[3];
    M[tri(o + 2, o + 1)] += W[4];
    M[tri(o + 2, o + 2)] += W[5];
    r[o] += W[0] * z[0] + W[1] * z[1] + W[2] * z[2];
    r[o + 1] += W[1] * z[0] + W[3] * z[1] + W[4] * z[2];
    r[o + 2] += W[2] * z[0] + W[4] * z[1] + W[5] * z[2];
}

// λ v vᵀ ⊗ I₃ with v = (1, −2, 1) on window blocks B, B+1, B+2: one second-difference row.
template <int B>
MVP_SMOOTH_HD void add_element(double (&M)[120], double lam) {
    constexpr double v[3] = {1.0, -2.0, 1.0};
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j <= i; j++)
#pragma unroll
            for (int d = 0; d < 3; d++) M[tri(3 * (B + i) + d, 3 * (B + j) + d)] += lam * v[i] * v[j];
}

// The frames lane (chain p, chunk k) works on.
struct LaneRange {
    int p, k;
    int g0;  // first interior frame
    int n;   // interior frames (>= 1)
    int hi;  // end of the owned frames: interior + right separator (0, 1 or 2 frames)
};

MVP_SMOOTH_HD LaneRange lane_range(const SmoothArgs& a, int64_t lane) {
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
MVP_SMOOTH_HD void eliminate_lane(const SmoothArgs& a, int64_t lane) {
    const LaneRange R = lane_range(a, lane);
    double M[120], r[15];
#pragma unroll
    for (int i = 0; i < 120; i++) M[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 15; i++) r[i] = 0.0;
    int cnt = 0;
    bool bad = false;
    double W[6], z[3];
    const bool has_b = R.g0 + 1 < R.hi;
    const RawFrame fa = load_raw(a, R.g0, R.p);
    const RawFrame fb = load_raw(a, has_b ? R.g0 + 1 : R.g0, R.p);
    RawFrame nxt = load_raw(a, R.g0 + 2 < R.hi ? R.g0 + 2 : R.g0, R.p);
    cnt += frame_weight(a, fa, W, z);
    add_data<2>(M, r, W, z);
    if (has_b) {
        cnt += frame_weight(a, fb, W, z);
        add_data<3>(M, r, W, z);
    }
    if (R.k > 0) {
        add_element<0>(M, a.lambda);
        if (has_b) add_element<1>(M, a.lambda);
    }
    for (int i = 0; i < R.n; i++) {
        // frame c enters; the frame after it is requested now
        const int c = R.g0 + i + 2;
        const RawFrame fc = nxt;
        if (c + 1 < R.hi) nxt = load_raw(a, c + 1, R.p);
#pragma unroll
        for (int j = tri(12, 0); j < 120; j++) M[j] = 0.0;
        r[12] = r[13] = r[14] = 0.0;
        if (c < R.hi) {
            cnt += frame_weight(a, fc, W, z);
            add_data<4>(M, r, W, z);
            add_element<2>(M, a.lambda);
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

MVP_SMOOTH_HD void load_reduce_in(const SmoothArgs& a, int p, int j, double (&v)[kInDoubles]) {
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
MVP_SMOOTH_HD void reduce_chain(const SmoothArgs& a, int p) {
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
    const int failed = (a.cnt[p] < 2 || bad) ? 1 : 0;
    a.fail[p] = failed;
    if (a.out_status) a.out_status[p] = failed ? 0x80 : 0;
}

// A failed chain's frame: the input bits, NaN resid.
MVP_SMOOTH_HD void write_failed(const SmoothArgs& a, int t, int p) {
    const int64_t e = (int64_t)t * a.P + p;
    const uint32_t* in = reinterpret_cast<const uint32_t*>(a.xyz);
    uint32_t* out = reinterpret_cast<uint32_t*>(a.out_xyz);
    out[3 * e] = in[3 * e];
    out[3 * e + 1] = in[3 * e + 1];
    out[3 * e + 2] = in[3 * e + 2];
    if (a.out_resid) a.out_resid[e] = NAN;
    if (a.out_observed) {
        double W[6], z[3];
        a.out_observed[e] = frame_weight(a, load_raw(a, t, p), W, z) ? 1 : 0;
    }
}

MVP_SMOOTH_HD void write_frame(const SmoothArgs& a, int t, int p, const RawFrame& f, double x0, double x1, double x2) {
    const int64_t e = (int64_t)t * a.P + p;
    a.out_xyz[3 * e] = (float)x0;
    a.out_xyz[3 * e + 1] = (float)x1;
    a.out_xyz[3 * e + 2] = (float)x2;
    if (a.out_resid || a.out_observed) {
        double W[6], z[3];
        const bool obs = frame_weight(a, f, W, z);
        if (a.out_observed) a.out_observed[e] = obs ? 1 : 0;
        if (a.out_resid) {
            const double d0 = x0 - z[0], d1 = x1 - z[1], d2 = x2 - z[2];
            const double m = d0 * (W[0] * d0 + W[1] * d1 + W[2] * d2) + d1 * (W[1] * d0 + W[3] * d1 + W[4] * d2) +
                             d2 * (W[2] * d0 + W[4] * d1 + W[5] * d2);
            a.out_resid[e] = obs ? (float)m : NAN;
        }
    }
}

MVP_SMOOTH_HD void backsub_lane(const SmoothArgs& a, int64_t lane) {
    const LaneRange R = lane_range(a, lane);
    if (a.fail[R.p] != 0) {
        for (int t = R.g0; t < R.hi; t++) write_failed(a, t, R.p);
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
            write_frame(a, R.g0 + R.n + q, R.p, load_raw(a, R.g0 + R.n + q, R.p), x[6 + 3 * q], x[7 + 3 * q],
                        x[8 + 3 * q]);
    // the factor and the input frame of step i-1 are requested while step i is solved
    double fc[kFacDoubles], fn[kFacDoubles];
    RawFrame rc = load_raw(a, R.g0 + R.n - 1, R.p), rn = rc;
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
            rn = load_raw(a, R.g0 + i - 1, R.p);
        }
        double xa[3];
#pragma unroll
        for (int d = 0; d < 3; d++) xa[d] = fc[36 + d];
#pragma unroll
        for (int o = 0; o < 12; o++)
#pragma unroll
            for (int d = 0; d < 3; d++) xa[d] -= fc[3 * o + d] * x[o];
        write_frame(a, R.g0 + i, R.p, rc, xa[0], xa[1], xa[2]);
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

__global__ __launch_bounds__(kSmBlock) void smooth_eliminate_kernel(SmoothArgs a) {
    const int64_t lane = (int64_t)blockIdx.x * kSmBlock + threadIdx.x;
    if (lane < a.n_lanes) eliminate_lane(a, lane);
}

__global__ __launch_bounds__(kSmBlock) void smooth_reduce_kernel(SmoothArgs a) {
    const int p = blockIdx.x * kSmBlock + threadIdx.x;
    if (p < a.P) reduce_chain(a, p);
}

__global__ __launch_bounds__(kSmBlock) void smooth_backsub_kernel(SmoothArgs a) {
    const int64_t lane = (int64_t)blockIdx.x * kSmBlock + threadIdx.x;
    if (lane < a.n_lanes) backsub_lane(a, lane);
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

}  // namespace

extern "C" int mvp_trajectory_smooth_plan(int T, int P, int chunk, int* chunk_used, int* n_chunks,
                                          int64_t* workspace_bytes) {
    MVP_ABI_BEGIN
    const SmoothPlan pl = smooth_plan("mvp_trajectory_smooth_plan", T, P, chunk);
    if (chunk_used) *chunk_used = pl.chunk;
    if (n_chunks) *n_chunks = pl.n_chunks;
    if (workspace_bytes) *workspace_bytes = pl.bytes;
    MVP_ABI_END
}

extern "C" int mvp_trajectory_smooth(const float* xyz, const float* cov, const uint8_t* valid, int T, int P,
                                     double lambda_smooth, float sigma0, float cov_floor, int chunk, void* workspace,
                                     int64_t workspace_bytes, float* out_xyz, float* out_resid, uint8_t* out_observed,
                                     uint8_t* out_status, void* stream) {
    MVP_ABI_BEGIN
    const char* fn = "mvp_trajectory_smooth";
    const SmoothPlan pl = smooth_plan(fn, T, P, chunk);
    MVP_REQUIRE(std::isfinite(lambda_smooth) && lambda_smooth > 0, "%s: lambda_smooth=%g must be finite and > 0", fn,
                lambda_smooth);
    MVP_REQUIRE(std::isfinite(sigma0) && sigma0 > 0, "%s: sigma0=%g must be finite and > 0", fn, (double)sigma0);
    MVP_REQUIRE(cov_floor >= 0, "%s: cov_floor=%g must be >= 0", fn, (double)cov_floor);
    MVP_REQUIRE(workspace_bytes >= pl.bytes, "%s: workspace_bytes=%lld < %lld needed (T=%d, P=%d, chunk=%d)", fn,
                (long long)workspace_bytes, (long long)pl.bytes, T, P, pl.chunk);
    MVP_REQUIRE(xyz && out_xyz && workspace, "%s: null device pointer", fn);
    MVP_REQUIRE(out_xyz != xyz, "%s: out_xyz must not alias xyz", fn);
    char* ws = static_cast<char*>(workspace);
    SmoothArgs a{};
    a.xyz = xyz;
    a.cov = cov;
    a.valid = valid;
    a.T = T;
    a.P = P;
    a.chunk = pl.chunk;
    a.n_chunks = pl.n_chunks;
    a.n_seps = pl.n_seps;
    a.n_lanes = pl.n_lanes;
    a.n_blocks = pl.n_blocks;
    a.lambda = lambda_smooth;
    a.w0 = 1.0 / ((double)sigma0 * (double)sigma0);
    a.cov_floor = (double)cov_floor;
    a.fac = reinterpret_cast<double*>(ws + pl.off_fac);
    a.schur = reinterpret_cast<double*>(ws + pl.off_schur);
    a.red = reinterpret_cast<double*>(ws + pl.off_red);
    a.usol = reinterpret_cast<double*>(ws + pl.off_usol);
    a.cnt = reinterpret_cast<int*>(ws + pl.off_cnt);
    a.bad = reinterpret_cast<int*>(ws + pl.off_bad);
    a.fail = reinterpret_cast<int*>(ws + pl.off_fail);
    a.out_xyz = out_xyz;
    a.out_resid = out_resid;
    a.out_observed = out_observed;
    a.out_status = out_status;
    hipStream_t s = (hipStream_t)stream;
    MVP_HIP(hipMemsetAsync(a.cnt, 0, (size_t)P * 8, s));
    hipLaunchKernelGGL(smooth_eliminate_kernel, dim3((unsigned)pl.n_blocks), dim3(kSmBlock), 0, s, a);
    MVP_HIP(hipGetLastError());
    hipLaunchKernelGGL(smooth_reduce_kernel, dim3((unsigned)((P + kSmBlock - 1) / kSmBlock)), dim3(kSmBlock), 0, s, a);
    MVP_HIP(hipGetLastError());
    hipLaunchKernelGGL(smooth_backsub_kernel, dim3((unsigned)pl.n_blocks), dim3(kSmBlock), 0, s, a);
    MVP_HIP(hipGetLastError());
    MVP_ABI_END
}
