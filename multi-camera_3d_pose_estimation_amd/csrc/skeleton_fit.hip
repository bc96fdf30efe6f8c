// The trajectory fit with a person's joints coupled by bone lengths (mvp_skeleton_fit_plan /
// _system / mvp_skeleton_fit; the problem is stated in include/mvpose.h; the reference has the
// term in its Adam loop only, mvp_sgd_refine) for gfx950.
//
// P = G·J chains, chain p = g·J + j the joint j of person (group) g.  Per group, Levenberg-Marquardt
// on
//   f_g = Σ_chains (Σ_t Σ_used rho + ½ λ Σ_t |second difference|²) + ½ β Σ_t Σ_s (r − L_{g,s})²,
// r the distance of segment s's two joints in frame t.  The bone term enters a chain's frame block
// with its exact gradient and with 2β·[n nᵀ + max(0, 1 − L/r)·(I − n nᵀ)] on both ends, the a-b
// cross block dropped: a trial is then one block-pentadiagonal solve per chain, exactly the
// trajectory fit's (smooth_solver.h over trajectory_fit_solver.h's frame source), and the coupling
// acts from trial to trial.  What differs from trajectory_fit.hip is who decides: one mu, one
// accept / reject and one stop per group, written to every chain of the group, so that the solver
// kernels run unchanged.  Stream-ordered launches, fp64, FMA contraction on, no floating-point
// atomics:
//
//   prepare    one lane per (t, p): the f64 copies of the seed and the two numbers a chain's
//              validity is summed from (as the trajectory fit's).
//   terms      one lane per (t, p), lanes along p, so that a frame's joints sit side by side: the
//              trajectory fit's terms plus, over the live segments that end at the lane's joint, the
//              other end's state (same frame, same buffer), the gradient and the curvature; the
//              segment's cost at its end a only.  Writes three cost terms per frame (Σ rho or +inf,
//              the prior's row, the bones).
//   sum        per chain, the frames' three numbers in tiles of 256 frames, as the trajectory fit's.
//   decide     one workgroup per group, lane j the joint j: the chain's tiles in ascending order,
//              then lane 0 adds the chains in ascending order (the same inputs give the same bits)
//              and decides; every lane writes the decision to its chain.  mode 0: validity of the
//              chains; mode 1: the group's cost at the seed; mode 2: accept / reject, mu, the stops.
//   eliminate / reduce / backsub   the partition solver, per chain.
//   output     one lane per (t, p): out_xyz, Σ s², the view counts, r − L of the segments whose end
//              a the lane is; per group the costs and the status.
// The launch sequence is mvp_trajectory_fit's.  A segment is dead when its length is not finite or
// not > 0 or one of its chains is invalid; the segment table (at most 64 pairs) travels in the
// kernel arguments and is read by scalar loads, the loop over it is uniform.
//
// Register / LDS / scratch figures and the measurements are in DESIGN.md §4.15.
#include "trajectory_fit_terms.h"

namespace {

constexpr int kSkMaxSeg = 64;
constexpr int kSkMaxJoints = 255;
constexpr int kSkGroupBlock = 256;   // the decide kernel's lanes: one per joint of the group

struct SkSegs {
    uint8_t a[kSkMaxSeg], b[kSkMaxSeg];
    int n, J;
    const float* len;   // [G][n]
    double beta;
};

// The per-group state of a fit, all [G].
struct SkGroup {
    double* mu;
    double* f;        // the state's cost
    double* fseed;
    double* bone;     // its bone part
    double* bseed;
    int* status;      // the group's status byte
    int* done;
};

// The bone terms of joint j of person g at X: over the live segments that end at j, with Y the
// other end (other(jo, Y) loads it), d = X − Y, r = |d|, u = d / r (n or −n: the terms are even in
// it): g += β·(r − L)·u, H += 2β·[u uᵀ + max(0, 1 − L/r)·(I − u uᵀ)], nothing when r == 0.  Returns
// ½ Σ (r − L)² over the segments whose end a is j.  status: the chains' status (a segment to an
// invalid chain is dead) or null (every segment with a live length is live).
template <bool JAC, class Other>
__device__ __forceinline__ double bone_terms(const SkSegs& sg, int g, int j, const int* __restrict__ status,
                                             const double (&X)[3], Other other, double (&H)[6], double (&gr)[3]) {
#pragma clang fp contract(fast)
    double cb = 0.0;
#pragma unroll 1
    for (int s = 0; s < sg.n; s++) {
        const int a = sg.a[s], b = sg.b[s];
        if (a != j && b != j) continue;
        const int jo = a == j ? b : a;
        const float Lf = sg.len[(int64_t)g * sg.n + s];
        bool live = isfinite(Lf) && Lf > 0.f;
        if (status) live = live && status[g * sg.J + jo] != 0x80;
        if (!live) continue;
        const double L = (double)Lf;
        double Y[3];
        other(jo, Y);
        const double d0 = X[0] - Y[0], d1 = X[1] - Y[1], d2 = X[2] - Y[2];
        const double r = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
        const double e = r - L;
        if (a == j) cb += 0.5 * e * e;
        if (JAC && r != 0.0) {
            const double ir = 1.0 / r;
            const double u0 = d0 * ir, u1 = d1 * ir, u2 = d2 * ir;
            const double w = fmax(0.0, 1.0 - L * ir);
            const double c = 2.0 * sg.beta, cu = c * (1.0 - w), cw = c * w, ge = sg.beta * e;
            H[0] += cu * u0 * u0 + cw;
            H[1] += cu * u0 * u1;
            H[2] += cu * u0 * u2;
            H[3] += cu * u1 * u1 + cw;
            H[4] += cu * u1 * u2;
            H[5] += cu * u2 * u2 + cw;
            gr[0] += ge * u0;
            gr[1] += ge * u1;
            gr[2] += ge * u2;
        }
    }
    return cb;
}

// ------------------------------------------------------------------------------- prepare
__global__ __launch_bounds__(kBlock) void sk_prepare_kernel(FitObs o, const float* __restrict__ xyz0,
                                                            double* __restrict__ x64, double* __restrict__ c3) {
#pragma clang fp contract(fast)
    __shared__ double scam[kMaxCams][MVP_CAM_DOUBLES];
    __shared__ CamFast sfast[kMaxCams];
    load_cams(scam, sfast, o.cams, o.n_cams);
    const int64_t n = (int64_t)o.T * o.P;
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= n) return;
    const int t = (int)(e / o.P), p = (int)(e - (int64_t)t * o.P);
    const float s0 = xyz0[3 * e + 0], s1 = xyz0[3 * e + 1], s2 = xyz0[3 * e + 2];
    const double X[3] = {(double)s0, (double)s1, (double)s2};
    FitFrame f;
    fit_frame<false>(o, scam, t, p, X, f);
    const bool fin = isfinite(s0) && isfinite(s1) && isfinite(s2);
    x64[3 * e + 0] = X[0], x64[3 * e + 1] = X[1], x64[3 * e + 2] = X[2];
    x64[3 * (n + e) + 0] = X[0], x64[3 * (n + e) + 1] = X[1], x64[3 * (n + e) + 2] = X[2];
    c3[3 * e + 0] = f.nviews >= 2 ? 1.0 : 0.0;
    c3[3 * e + 1] = (fin && f.front) ? 0.0 : 1.0;
    c3[3 * e + 2] = 0.0;
}

// ------------------------------------------------------------------------------- terms
struct SkTerms {
    FitObs o;
    SkSegs sg;
    const float* x32;      // mvp_skeleton_fit_system: the state, f32 [T][P][3]; else null
    const double* x64;     // [2][T][P][3]
    FitChain ch;           // (null pointers with x32)
    int trial;             // evaluate the chains' trial buffer, not their state
    double lambda;
    double* H;             // [T][P][6] with JAC
    double* g;             // [T][P][3] with JAC: the gradient without the prior with x32, else the solve's right-hand side
    double* c3;            // [T][P][3] or null
    uint8_t* nviews;       // [T][P] or null
};

template <bool JAC>
__global__ __launch_bounds__(kBlock) void sk_terms_kernel(SkTerms a) {
#pragma clang fp contract(fast)
    __shared__ double scam[kMaxCams][MVP_CAM_DOUBLES];
    __shared__ CamFast sfast[kMaxCams];
    load_cams(scam, sfast, a.o.cams, a.o.n_cams);
    const int T = a.o.T, P = a.o.P;
    const int64_t n = (int64_t)T * P;
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= n) return;
    const int t = (int)(e / P), p = (int)(e - (int64_t)t * P);
    if (!a.x32) {
        if (a.ch.done[p]) return;
        if (JAC && !a.ch.relin[p]) return;
    }
    // the frames t-2 .. t+2 of the chain (the cost reads t-2 .. t only)
    double Xw[5][3];
    const int64_t buf = a.x32 ? 0 : (int64_t)(a.ch.cur[p] ^ a.trial) * n;
#pragma unroll
    for (int q = 0; q < 5; q++) {
        const int tq = t + q - 2;
        const bool in = tq >= 0 && tq < T && (JAC || q <= 2);
        const int64_t eq = in ? e + (int64_t)(q - 2) * P : e;
#pragma unroll
        for (int k = 0; k < 3; k++) Xw[q][k] = a.x32 ? (double)a.x32[3 * eq + k] : a.x64[3 * (buf + eq) + k];
    }
    const double X[3] = {Xw[2][0], Xw[2][1], Xw[2][2]};
    FitFrame f;
    fit_frame<JAC>(a.o, scam, t, p, X, f);
    // the bones: the other ends are the group's chains in the same frame; a group's valid chains
    // share cur, so the lane's own buffer is theirs
    const int g = p / a.sg.J, j = p - g * a.sg.J;
    const int64_t e0 = e - j;
    const double cb = bone_terms<JAC>(
        a.sg, g, j, a.x32 ? (const int*)nullptr : a.ch.status, X,
        [&](int jo, double (&Y)[3]) {
#pragma unroll
            for (int k = 0; k < 3; k++)
                Y[k] = a.x32 ? (double)a.x32[3 * (e0 + jo) + k] : a.x64[3 * (buf + e0 + jo) + k];
        },
        f.H, f.g);
    // second-difference rows t, t+1, t+2 (row s exists for 2 <= s <= T-1)
    double d[3][3];
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const bool row = t + q >= 2 && t + q <= T - 1 && (JAC || q == 0);
#pragma unroll
        for (int k = 0; k < 3; k++) d[q][k] = row ? Xw[q + 2][k] - 2.0 * Xw[q + 1][k] + Xw[q][k] : 0.0;
    }
    if (a.c3) {
        a.c3[3 * e + 0] = f.front ? f.rho : (double)INFINITY;
        a.c3[3 * e + 1] = 0.5 * a.lambda * (d[0][0] * d[0][0] + d[0][1] * d[0][1] + d[0][2] * d[0][2]);
        a.c3[3 * e + 2] = a.sg.beta * cb;
    }
    if (a.nviews) a.nviews[e] = (uint8_t)f.nviews;
    if (JAC) {
#pragma unroll
        for (int k = 0; k < 6; k++) a.H[6 * e + k] = f.H[k];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double prior = a.lambda * (d[0][k] - 2.0 * d[1][k] + d[2][k]);
            a.g[3 * e + k] = a.x32 ? f.g[k] : -(f.g[k] + prior);
        }
    }
}

// mvp_skeleton_fit_system's costs: one workgroup per group, each lane its (frame, joint) pairs in
// ascending order, then a tree over the lanes in a fixed order.
__global__ __launch_bounds__(kBlock) void sk_system_cost_kernel(FitObs o, SkSegs sg, const float* __restrict__ x32,
                                                                double* __restrict__ out_cost) {
#pragma clang fp contract(fast)
    __shared__ double scam[kMaxCams][MVP_CAM_DOUBLES];
    __shared__ CamFast sfast[kMaxCams];
    __shared__ double s_red[3][kBlock];
    load_cams(scam, sfast, o.cams, o.n_cams);
    const int g = blockIdx.x, J = sg.J;
    const int64_t items = (int64_t)o.T * J;
    double rho = 0.0, sm = 0.0, bone = 0.0;
    for (int64_t i = threadIdx.x; i < items; i += kBlock) {
        const int t = (int)(i / J), j = (int)(i - (int64_t)t * J);
        const int p = g * J + j;
        double Xw[3][3];
#pragma unroll
        for (int q = 0; q < 3; q++) {
            const int tq = t + q - 2 >= 0 ? t + q - 2 : t;
#pragma unroll
            for (int k = 0; k < 3; k++) Xw[q][k] = (double)x32[3 * ((int64_t)tq * o.P + p) + k];
        }
        const double X[3] = {Xw[2][0], Xw[2][1], Xw[2][2]};
        FitFrame f;
        fit_frame<false>(o, scam, t, p, X, f);
        rho += f.front ? f.rho : (double)INFINITY;
        if (t >= 2) {
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const double d = Xw[2][k] - 2.0 * Xw[1][k] + Xw[0][k];
                sm += 0.5 * d * d;
            }
        }
        const int64_t e0 = (int64_t)t * o.P + (int64_t)g * J;
        bone += bone_terms<false>(
            sg, g, j, (const int*)nullptr, X,
            [&](int jo, double (&Y)[3]) {
#pragma unroll
                for (int k = 0; k < 3; k++) Y[k] = (double)x32[3 * (e0 + jo) + k];
            },
            f.H, f.g);
    }
    s_red[0][threadIdx.x] = rho;
    s_red[1][threadIdx.x] = sm;
    s_red[2][threadIdx.x] = bone;
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
#pragma unroll
            for (int k = 0; k < 3; k++) s_red[k][threadIdx.x] += s_red[k][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 3; k++) out_cost[3 * g + k] = s_red[k][0];
    }
}

// ------------------------------------------------------------------------------- sum, decide
// part[tile][p][3] = the three numbers of c3 over the tile's frames of chain p.
__global__ __launch_bounds__(kFitRows * 64) void sk_sum_kernel(const double* __restrict__ c3, int T, int P,
                                                               const int* __restrict__ done,
                                                               double* __restrict__ part) {
    __shared__ double s_red[3][kFitRows][64];
    const int px = threadIdx.x & 63, row = threadIdx.x >> 6;
    const int p_tiles = (P + 63) / 64;
    const int tile = blockIdx.x / p_tiles;
    const int p = (blockIdx.x - tile * p_tiles) * 64 + px;
    const int t0 = tile * kFitTile;
    const int t1 = t0 + kFitTile < T ? t0 + kFitTile : T;
    const bool live = p < P && !(done && done[p]);
    double s[3] = {0.0, 0.0, 0.0};
    if (live) {
#pragma unroll 4
        for (int t = t0 + row; t < t1; t += kFitRows) {
            const int64_t e = (int64_t)t * P + p;
#pragma unroll
            for (int k = 0; k < 3; k++) s[k] += c3[3 * e + k];
        }
    }
#pragma unroll
    for (int k = 0; k < 3; k++) s_red[k][row][px] = s[k];
    __syncthreads();
    if (row == 0 && live) {
#pragma unroll
        for (int r = 1; r < kFitRows; r++)
#pragma unroll
            for (int k = 0; k < 3; k++) s[k] += s_red[k][r][px];
#pragma unroll
        for (int k = 0; k < 3; k++) part[3 * ((int64_t)tile * P + p) + k] = s[k];
    }
}

// mode 0: the chains' validity from prepare's sums; mode 1: the group's cost at the seed; mode 2:
// the trial's.  Lane j is chain g·J + j; lanes past J only keep the barriers.
__global__ __launch_bounds__(kSkGroupBlock) void sk_decide_kernel(FitChain ch, SkGroup gr,
                                                                  const double* __restrict__ part, int n_tiles, int P,
                                                                  int J, int mode, int max_iter, double tol,
                                                                  int* __restrict__ bad) {
    __shared__ double s_f[kSkGroupBlock], s_b[kSkGroupBlock];
    __shared__ int s_flag[kSkGroupBlock];
    __shared__ int s_dec[4];       // mode 0: any valid chain; 1: the seed is finite; 2: accept, done
    __shared__ double s_mu;
    const int g = blockIdx.x, j = threadIdx.x;
    if (mode == 2 && gr.done[g]) return;   // the whole workgroup
    const int p = g * J + j;
    const bool mine = j < J;
    // a chain takes part once it is valid: decided in mode 0, from everybody's sums
    const bool part_of = mine && (mode == 0 || ch.status[p] != 0x80);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    if (part_of) {
#pragma unroll 8   // eight loads in flight; the additions stay in index order
        for (int w = 0; w < n_tiles; w++) {
            s0 += part[3 * ((int64_t)w * P + p) + 0];
            s1 += part[3 * ((int64_t)w * P + p) + 1];
            s2 += part[3 * ((int64_t)w * P + p) + 2];
        }
        bad[p] = 0;
    }
    if (mode == 0) {
        const bool valid = mine && s0 >= 2.0 && s1 == 0.0;
        s_flag[j] = valid ? 1 : 0;
        __syncthreads();
        if (j == 0) {
            int any = 0;
            for (int q = 0; q < J; q++) any |= s_flag[q];
            gr.mu[g] = 1e-3;
            gr.f[g] = gr.fseed[g] = gr.bone[g] = gr.bseed[g] = __builtin_nan("");
            gr.status[g] = any ? 0x40 : 0x80;
            gr.done[g] = any ? 0 : 1;
        }
        if (mine) {
            ch.mu[p] = 1e-3;
            ch.f[p] = ch.fseed[p] = __builtin_nan("");
            ch.cur[p] = 0;
            ch.done[p] = valid ? 0 : 1;
            ch.status[p] = valid ? 0 : 0x80;
            ch.relin[p] = 1;
            ch.rej[p] = 0;
        }
        return;
    }
    s_f[j] = s0 + s1;
    s_b[j] = s2;
    s_flag[j] = part_of ? (mode == 2 && ch.rej[p] ? 3 : 1) : 0;   // bit 0: takes part; bit 1: a pivot failed
    __syncthreads();
    if (j == 0) {
        // the chains in ascending order, then the bones
        double F = 0.0, B = 0.0;
        int any = 0, rej = 0;
        for (int q = 0; q < J; q++) {
            if (!(s_flag[q] & 1)) continue;
            any = 1;
            rej |= s_flag[q] >> 1;
            F += s_f[q];
            B += s_b[q];
        }
        const double ft = F + B;
        if (mode == 1) {
            const bool fin = any && isfinite(ft);   // a seed whose cost overflows is no seed
            gr.f[g] = gr.fseed[g] = fin ? ft : __builtin_nan("");
            gr.bone[g] = gr.bseed[g] = fin ? B : __builtin_nan("");
            gr.status[g] = fin ? 0x40 : 0x80;
            gr.done[g] = (fin && max_iter > 0) ? 0 : 1;
            s_dec[0] = fin ? 1 : 0;
        } else {
            const double f = gr.f[g];
            const int trials = (gr.status[g] & 63) + 1;
            const bool accept = !rej && isfinite(ft) && ft <= f;
            bool done = false, conv = false;
            double mu = gr.mu[g];
            if (accept) {
                conv = (f - ft) <= tol * f;
                gr.f[g] = ft;
                gr.bone[g] = B;
                mu = fmax(mu * 0.1, 1e-12);
                done = conv;
            } else {
                mu = mu * 10.0;
                done = mu > 1e12;
            }
            done = done || trials >= max_iter;
            gr.mu[g] = mu;
            gr.status[g] = trials | (conv ? 0 : 0x40);
            gr.done[g] = done ? 1 : 0;
            s_dec[0] = accept ? 1 : 0;
            s_dec[1] = done ? 1 : 0;
            s_mu = mu;
        }
    }
    __syncthreads();
    if (!part_of) return;
    if (mode == 1) {
        const bool fin = s_dec[0] != 0;
        ch.done[p] = (fin && max_iter > 0) ? 0 : 1;
        ch.status[p] = fin ? 0 : 0x80;   // the chains of an invalid group are returned as they came
        ch.relin[p] = 0;                 // the seed has just been linearised
        return;
    }
    const bool accept = s_dec[0] != 0;
    if (accept) ch.cur[p] ^= 1;
    ch.mu[p] = s_mu;
    ch.relin[p] = accept ? 1 : 0;
    ch.done[p] = s_dec[1];
}

__global__ __launch_bounds__(kSmBlock) void sk_eliminate_kernel(FitSolveArgs a) {
    const int64_t lane = (int64_t)blockIdx.x * kSmBlock + threadIdx.x;
    if (lane < a.n_lanes) eliminate_lane(a, lane);
}

__global__ __launch_bounds__(kSmBlock) void sk_reduce_kernel(FitSolveArgs a) {
    const int p = blockIdx.x * kSmBlock + threadIdx.x;
    if (p < a.P) reduce_chain(a, p);
}

__global__ __launch_bounds__(kSmBlock) void sk_backsub_kernel(FitSolveArgs a) {
    const int64_t lane = (int64_t)blockIdx.x * kSmBlock + threadIdx.x;
    if (lane < a.n_lanes) backsub_lane(a, lane);
}

// ------------------------------------------------------------------------------- output
struct SkOut {
    float* xyz;          // [T][P][3]
    float* resid;        // [T][P] or null
    uint8_t* nviews;     // [T][P] or null
    float* bone;         // [T][G][n_seg] or null
    double* cost;        // [G][4] or null
    uint8_t* gstatus;    // [G] or null
    uint8_t* cstatus;    // [P] or null
};

__global__ __launch_bounds__(kBlock) void sk_output_kernel(FitObs o, SkSegs sg, const float* __restrict__ xyz0,
                                                           const double* __restrict__ x64, FitChain ch, SkGroup gr,
                                                           SkOut out) {
#pragma clang fp contract(fast)
    __shared__ double scam[kMaxCams][MVP_CAM_DOUBLES];
    __shared__ CamFast sfast[kMaxCams];
    load_cams(scam, sfast, o.cams, o.n_cams);
    const int64_t n = (int64_t)o.T * o.P;
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= n) return;
    const int t = (int)(e / o.P), p = (int)(e - (int64_t)t * o.P);
    const int g = p / sg.J, j = p - g * sg.J, G = o.P / sg.J;
    const bool valid = ch.status[p] != 0x80;
    const int64_t buf = (int64_t)ch.cur[p] * n;
    const double* xp = x64 + 3 * (buf + e);
    const double X[3] = {xp[0], xp[1], xp[2]};
    FitFrame f;
    fit_frame<false>(o, scam, t, p, X, f);
    const uint32_t* in = reinterpret_cast<const uint32_t*>(xyz0);
    uint32_t* o32 = reinterpret_cast<uint32_t*>(out.xyz);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        if (valid)
            out.xyz[3 * e + k] = (float)X[k];
        else
            o32[3 * e + k] = in[3 * e + k];   // the seed's bits, NaN payloads included
    }
    if (out.resid) out.resid[e] = (valid && f.nviews > 0) ? (float)f.s2 : __builtin_nanf("");
    if (out.nviews) out.nviews[e] = (uint8_t)f.nviews;
    if (out.bone) {
        // the segments whose end a this joint is: every (t, g, s) is written by exactly one lane
        const int64_t e0 = e - j;
#pragma unroll 1
        for (int s = 0; s < sg.n; s++) {
            if (sg.a[s] != j) continue;
            const int jo = sg.b[s];
            const float Lf = sg.len[(int64_t)g * sg.n + s];
            const bool live = valid && isfinite(Lf) && Lf > 0.f && ch.status[g * sg.J + jo] != 0x80;
            float v = __builtin_nanf("");
            if (live) {
                const double* yp = x64 + 3 * (buf + e0 + jo);
                const double d0 = X[0] - yp[0], d1 = X[1] - yp[1], d2 = X[2] - yp[2];
                v = (float)(sqrt(d0 * d0 + d1 * d1 + d2 * d2) - (double)Lf);
            }
            out.bone[((int64_t)t * G + g) * sg.n + s] = v;
        }
    }
    if (t == 0) {
        if (out.cstatus) out.cstatus[p] = valid ? 0 : 0x80;
        if (j == 0) {
            if (out.cost) {
                out.cost[4 * g + 0] = gr.fseed[g];
                out.cost[4 * g + 1] = gr.f[g];
                out.cost[4 * g + 2] = gr.bseed[g];
                out.cost[4 * g + 3] = gr.bone[g];
            }
            if (out.gstatus) out.gstatus[g] = (uint8_t)gr.status[g];
        }
    }
}

// ------------------------------------------------------------------------------- host side
// The segment arguments' checks; returns the table the kernels take.
inline SkSegs sk_parse(const char* fn, int P, int J, const int* seg, int n_seg, const float* seg_len,
                       double lambda_bone) {
    MVP_REQUIRE(J >= 1 && J <= kSkMaxJoints, "%s: J=%d (1..%d)", fn, J, kSkMaxJoints);
    MVP_REQUIRE(P % J == 0, "%s: P=%d is not a multiple of J=%d", fn, P, J);
    MVP_REQUIRE(n_seg >= 0 && n_seg <= kSkMaxSeg, "%s: n_seg=%d (0..%d)", fn, n_seg, kSkMaxSeg);
    MVP_REQUIRE(n_seg == 0 || seg != nullptr, "%s: seg_host is NULL with n_seg=%d", fn, n_seg);
    MVP_REQUIRE(std::isfinite(lambda_bone) && lambda_bone >= 0, "%s: lambda_bone=%g must be finite and >= 0", fn,
                lambda_bone);
    SkSegs sg{};
    for (int s = 0; s < n_seg; s++) {
        const int a = seg[2 * s], b = seg[2 * s + 1];
        MVP_REQUIRE(a >= 0 && a < J && b >= 0 && b < J && a != b, "%s: seg_host[%d]=(%d, %d): two different joints below J=%d",
                    fn, s, a, b, J);
        for (int q = 0; q < s; q++)
            MVP_REQUIRE(!((sg.a[q] == a && sg.b[q] == b) || (sg.a[q] == b && sg.b[q] == a)),
                        "%s: seg_host[%d] repeats the pair of seg_host[%d]", fn, s, q);
        sg.a[s] = (uint8_t)a, sg.b[s] = (uint8_t)b;
    }
    MVP_REQUIRE(n_seg == 0 || seg_len != nullptr, "%s: seg_len_dev is NULL with n_seg=%d", fn, n_seg);
    sg.n = n_seg, sg.J = J, sg.len = seg_len, sg.beta = lambda_bone;
    return sg;
}

struct SkPlan {
    SmoothPlan sp;
    int n_tiles;
    int64_t sum_blocks;
    int64_t off_chain, off_group, off_x, off_H, off_g, off_c3, off_part, bytes;
};

inline SkPlan sk_plan(const char* fn, int T, int P, int J, int chunk) {
    SkPlan pl;
    pl.sp = smooth_plan(fn, T, P, chunk);
    MVP_REQUIRE((int64_t)T * P < (1LL << 31), "%s: T·P=%lld must be < 2^31", fn, (long long)T * P);
    MVP_REQUIRE(J >= 1 && J <= kSkMaxJoints, "%s: J=%d (1..%d)", fn, J, kSkMaxJoints);
    MVP_REQUIRE(P % J == 0, "%s: P=%d is not a multiple of J=%d", fn, P, J);
    const int64_t n = (int64_t)T * P;
    pl.n_tiles = (T + kFitTile - 1) / kFitTile;
    pl.sum_blocks = (int64_t)pl.n_tiles * ((P + 63) / 64);
    MVP_REQUIRE(pl.sum_blocks < (1LL << 31), "%s: too many tiles (T=%d, P=%d)", fn, T, P);
    int64_t b = pl.sp.bytes;
    pl.off_chain = b;
    b = align256(b + (int64_t)P * (3 * 8 + 5 * 4));
    pl.off_group = b;
    b = align256(b + (int64_t)(P / J) * (5 * 8 + 2 * 4));
    pl.off_x = b;
    b = align256(b + 2 * n * 3 * 8);
    pl.off_H = b;
    b = align256(b + n * 6 * 8);
    pl.off_g = b;
    b = align256(b + n * 3 * 8);
    pl.off_c3 = b;
    b = align256(b + n * 3 * 8);
    pl.off_part = b;
    b = align256(b + (int64_t)pl.n_tiles * P * 3 * 8);
    pl.bytes = b;
    return pl;
}

}  // namespace

extern "C" int mvp_skeleton_fit_plan(int T, int P, int J, int chunk, int* chunk_used, int* n_chunks,
                                     int64_t* workspace_bytes) {
    MVP_ABI_BEGIN
    const SkPlan pl = sk_plan("mvp_skeleton_fit_plan", T, P, J, chunk);
    if (chunk_used) *chunk_used = pl.sp.chunk;
    if (n_chunks) *n_chunks = pl.sp.n_chunks;
    if (workspace_bytes) *workspace_bytes = pl.bytes;
    MVP_ABI_END
}

extern "C" int mvp_skeleton_fit_system(const float* kpts, int T, int P, int V, const double* cams, int n_cams,
                                       const int* cam_idx, int n_cam_idx, const float* xyz, const uint8_t* mask,
                                       int weights, const double* gauss, float min_conf, float cov_floor,
                                       double huber_delta, int J, const int* seg_host, int n_seg,
                                       const float* seg_len, double lambda_bone, double* out_H, double* out_g,
                                       uint8_t* out_nviews, double* out_cost, void* stream) {
    MVP_ABI_BEGIN
    const char* fn = "mvp_skeleton_fit_system";
    const FitObs o = fit_parse(fn, kpts, T, P, V, cams, n_cams, cam_idx, n_cam_idx, mask, weights, gauss, min_conf,
                               cov_floor, huber_delta);
    const SkSegs sg = sk_parse(fn, P, J, seg_host, n_seg, seg_len, lambda_bone);
    MVP_REQUIRE(kpts && cams && xyz && out_H && out_g && out_nviews && out_cost, "%s: null device pointer", fn);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    SkTerms a{};
    a.o = o;
    a.sg = sg;
    a.x32 = xyz;
    a.lambda = 1.0;
    a.H = out_H;
    a.g = out_g;
    a.nviews = out_nviews;
    hipLaunchKernelGGL(sk_terms_kernel<true>, dim3(tri_grid(fn, (int64_t)T * P)), dim3(kBlock), 0, s, a);
    MVP_HIP(hipGetLastError());
    SkSegs unit = sg;
    unit.beta = 1.0;
    hipLaunchKernelGGL(sk_system_cost_kernel, dim3((unsigned)(P / J)), dim3(kBlock), 0, s, o, unit, xyz, out_cost);
    MVP_HIP(hipGetLastError());
    MVP_ABI_END
}

extern "C" int mvp_skeleton_fit(const float* kpts, int T, int P, int V, const double* cams, int n_cams,
                                const int* cam_idx, int n_cam_idx, const float* xyz0, const uint8_t* mask, int weights,
                                const double* gauss, float min_conf, float cov_floor, double huber_delta,
                                double lambda_smooth, int J, const int* seg_host, int n_seg, const float* seg_len,
                                double lambda_bone, int max_iter, double tol, int chunk, void* workspace,
                                int64_t workspace_bytes, float* out_xyz, float* out_resid, uint8_t* out_nviews,
                                float* out_bone, double* out_cost, uint8_t* out_group_status,
                                uint8_t* out_chain_status, void* stream) {
    MVP_ABI_BEGIN
    const char* fn = "mvp_skeleton_fit";
    const FitObs o = fit_parse(fn, kpts, T, P, V, cams, n_cams, cam_idx, n_cam_idx, mask, weights, gauss, min_conf,
                               cov_floor, huber_delta);
    const SkPlan pl = sk_plan(fn, T, P, J, chunk);
    const SkSegs sg = sk_parse(fn, P, J, seg_host, n_seg, seg_len, lambda_bone);
    MVP_REQUIRE(std::isfinite(lambda_smooth) && lambda_smooth > 0, "%s: lambda_smooth=%g must be finite and > 0", fn,
                lambda_smooth);
    MVP_REQUIRE(max_iter >= 0 && max_iter <= 63, "%s: max_iter=%d (0..63)", fn, max_iter);
    MVP_REQUIRE(std::isfinite(tol) && tol > 0, "%s: tol=%g (finite, > 0)", fn, tol);
    MVP_REQUIRE(workspace_bytes >= pl.bytes, "%s: workspace_bytes=%lld < %lld needed (T=%d, P=%d, J=%d, chunk=%d)", fn,
                (long long)workspace_bytes, (long long)pl.bytes, T, P, J, pl.sp.chunk);
    MVP_REQUIRE(kpts && cams && xyz0 && workspace && out_xyz, "%s: null device pointer", fn);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    const int64_t n = (int64_t)T * P;
    const int G = P / J;
    FitChain ch;
    {
        char* c = ws + pl.off_chain;
        ch.mu = reinterpret_cast<double*>(c);
        ch.f = ch.mu + P;
        ch.fseed = ch.f + P;
        ch.cur = reinterpret_cast<int*>(ch.fseed + P);
        ch.done = ch.cur + P;
        ch.status = ch.done + P;
        ch.relin = ch.status + P;
        ch.rej = ch.relin + P;
    }
    SkGroup gr;
    {
        char* c = ws + pl.off_group;
        gr.mu = reinterpret_cast<double*>(c);
        gr.f = gr.mu + G;
        gr.fseed = gr.f + G;
        gr.bone = gr.fseed + G;
        gr.bseed = gr.bone + G;
        gr.status = reinterpret_cast<int*>(gr.bseed + G);
        gr.done = gr.status + G;
    }
    double* x64 = reinterpret_cast<double*>(ws + pl.off_x);
    double* c3 = reinterpret_cast<double*>(ws + pl.off_c3);
    double* part = reinterpret_cast<double*>(ws + pl.off_part);
    FitSolveArgs sa{};
    sa.T = T, sa.P = P, sa.chunk = pl.sp.chunk, sa.n_chunks = pl.sp.n_chunks, sa.n_seps = pl.sp.n_seps;
    sa.n_lanes = pl.sp.n_lanes, sa.n_blocks = pl.sp.n_blocks;
    sa.lambda = lambda_smooth;
    sa.fac = reinterpret_cast<double*>(ws + pl.sp.off_fac);
    sa.schur = reinterpret_cast<double*>(ws + pl.sp.off_schur);
    sa.red = reinterpret_cast<double*>(ws + pl.sp.off_red);
    sa.usol = reinterpret_cast<double*>(ws + pl.sp.off_usol);
    sa.cnt = reinterpret_cast<int*>(ws + pl.sp.off_cnt);
    sa.bad = reinterpret_cast<int*>(ws + pl.sp.off_bad);
    sa.H = reinterpret_cast<double*>(ws + pl.off_H);
    sa.g = reinterpret_cast<double*>(ws + pl.off_g);
    sa.x64 = x64;
    sa.ch = ch;
    SkTerms ta{};
    ta.o = o;
    ta.sg = sg;
    ta.x64 = x64;
    ta.ch = ch;
    ta.lambda = lambda_smooth;
    ta.H = reinterpret_cast<double*>(ws + pl.off_H);
    ta.g = reinterpret_cast<double*>(ws + pl.off_g);
    ta.c3 = c3;
    const dim3 flat(tri_grid(fn, n)), blk(kBlock);
    const dim3 sum_grid((unsigned)pl.sum_blocks), sum_blk(kFitRows * 64);
    const dim3 chain_grid((unsigned)((P + kSmBlock - 1) / kSmBlock)), lane_grid((unsigned)pl.sp.n_blocks), sm_blk(kSmBlock);
    auto sum_decide = [&](int mode) {
        hipLaunchKernelGGL(sk_sum_kernel, sum_grid, sum_blk, 0, s, c3, T, P, mode == 0 ? (const int*)nullptr : ch.done,
                           part);
        hipLaunchKernelGGL(sk_decide_kernel, dim3((unsigned)G), dim3(kSkGroupBlock), 0, s, ch, gr, part, pl.n_tiles, P, J,
                           mode, max_iter, tol, sa.bad);
        MVP_HIP(hipGetLastError());
    };
    MVP_HIP(hipMemsetAsync(sa.cnt, 0, (size_t)P * 8, s));
    hipLaunchKernelGGL(sk_prepare_kernel, flat, blk, 0, s, o, xyz0, x64, c3);
    MVP_HIP(hipGetLastError());
    sum_decide(0);
    ta.trial = 0;
    hipLaunchKernelGGL(sk_terms_kernel<true>, flat, blk, 0, s, ta);
    sum_decide(1);
    for (int it = 0; it < max_iter; it++) {
        hipLaunchKernelGGL(sk_eliminate_kernel, lane_grid, sm_blk, 0, s, sa);
        hipLaunchKernelGGL(sk_reduce_kernel, chain_grid, sm_blk, 0, s, sa);
        hipLaunchKernelGGL(sk_backsub_kernel, lane_grid, sm_blk, 0, s, sa);
        ta.trial = 1;
        hipLaunchKernelGGL(sk_terms_kernel<false>, flat, blk, 0, s, ta);
        sum_decide(2);
        if (it + 1 < max_iter) {
            ta.trial = 0;
            hipLaunchKernelGGL(sk_terms_kernel<true>, flat, blk, 0, s, ta);
            MVP_HIP(hipGetLastError());
        }
    }
    SkOut out{out_xyz, out_resid, out_nviews, out_bone, out_cost, out_group_status, out_chain_status};
    hipLaunchKernelGGL(sk_output_kernel, flat, blk, 0, s, o, sg, xyz0, x64, ch, gr, out);
    MVP_HIP(hipGetLastError());
    MVP_ABI_END
}
