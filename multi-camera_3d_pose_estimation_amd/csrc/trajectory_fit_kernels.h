// The kernels, the decision rules and the launch sequence that the trajectory fit
// (trajectory_fit.hip) and the skeleton fit (skeleton_fit.hip) share, written once and templated on
// a coupling policy C: what ties a chain's frame to other chains of the same frame.
//
//   C::kCosts                     the cost terms a frame has: Σ rho, the prior's row, then the policy's
//   joints(), C::Item             chain p is joint j of group g, p = g·joints() + j; the system-cost
//                                 kernel's workgroup walks a group's T·joints() (frame, joint)
//                                 pairs, counted in Item
//   frame_terms<JAC>(e, g, j, status, X, other, f)   the policy's cost of the chain's frame
//                                 e = t·P + p at X before its weight, with JAC its gradient and
//                                 curvature onto f.g, f.H; other(e', Y) loads the state of frame e'
//                                 from the same buffer; status as bone_terms takes it
//   weight()                      the weight of that cost in the fit (the _system calls return the
//                                 costs unweighted)
//   output_frame(...), output_chain(...)       what the output kernel writes beyond a frame's
//                                 coordinates, resid and view count: per frame, and per chain (by
//                                 the lane of frame 0)
//
// NoCoupling (here) is the trajectory fit: two costs, nothing added, and being empty it costs the
// kernels no register and no kernel-argument load.  The skeleton fit's policy is SkBones
// (skeleton_fit.hip).  The policy travels by value behind the kernel's other arguments.
//
// Every kernel body that does floating-point work on the state carries fp contract(fast), as
// fit_frame does; the decision rules carry none.
#pragma once
#include "trajectory_fit_terms.h"

namespace {

struct NoCoupling {
    static constexpr int kCosts = 2;
    using Item = int;
    __device__ __forceinline__ int joints() const { return 1; }
    template <bool JAC, class Other>
    __device__ __forceinline__ double frame_terms(int64_t, int, int, const int*, const double (&)[3], Other,
                                                  FitFrame&) const {
        return 0.0;
    }
    __device__ __forceinline__ void output_frame(const FitObs&, const FitChain&, const double*, int64_t, int64_t, int, int,
                                                 int, bool, const double (&)[3]) const {}
    // out_cost [P][2]: the seed's cost and the state's; out_status [P]
    __device__ __forceinline__ void output_chain(const FitChain& ch, int p, int, int, int status,
                                                 double* __restrict__ out_cost, uint8_t* __restrict__ out_status) const {
        if (out_cost) {
            out_cost[2 * p + 0] = ch.fseed[p];
            out_cost[2 * p + 1] = ch.f[p];
        }
        if (out_status) out_status[p] = (uint8_t)status;
    }
};

// ------------------------------------------------------------------------------- prepare
// One lane per (t, p): the f64 copy of the seed in both state buffers and the two numbers a chain's
// validity is summed from (the frame has >= 2 used views; its seed is not finite or lies behind a
// used view); a policy's further costs start at zero.
template <int NC>
__global__ __launch_bounds__(kBlock) void fit_prepare_kernel(FitObs o, const float* __restrict__ xyz0,
                                                             double* __restrict__ x64, double* __restrict__ cost) {
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
    cost[NC * e + 0] = f.nviews >= 2 ? 1.0 : 0.0;
    cost[NC * e + 1] = (fin && f.front) ? 0.0 : 1.0;
#pragma unroll
    for (int k = 2; k < NC; k++) cost[NC * e + k] = 0.0;
}

// ------------------------------------------------------------------------------- terms
struct FitTerms {
    FitObs o;
    const float* x32;      // the _system and _cov calls: the state, f32 [T][P][3]; else null
    const double* x64;     // [2][T][P][3]
    FitChain ch;           // (null pointers with x32)
    int trial;             // evaluate the chain's trial buffer, not its state
    double lambda;
    double* H;             // [T][P][6] with JAC
    double* g;             // [T][P][3] with JAC: the gradient without the prior with x32, else the solve's right-hand side
    double* cost;          // [T][P][kCosts] or null
    uint8_t* nviews;       // [T][P] or null
};

template <bool JAC, class C>
__global__ __launch_bounds__(kBlock) void fit_terms_kernel(FitTerms a, C cp) {
#pragma clang fp contract(fast)
    constexpr int NC = C::kCosts;
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
    // the coupling: the other chains in the same frame; chains that decide together share cur, so
    // the lane's own buffer is theirs
    const int J = cp.joints(), g = p / J, j = p - g * J;
    const double cc = cp.template frame_terms<JAC>(
        e, g, j, a.x32 ? (const int*)nullptr : a.ch.status, X,
        [&](int64_t eo, double (&Y)[3]) {
#pragma unroll
            for (int k = 0; k < 3; k++) Y[k] = a.x32 ? (double)a.x32[3 * eo + k] : a.x64[3 * (buf + eo) + k];
        },
        f);
    // second-difference rows t, t+1, t+2 (row s exists for 2 <= s <= T-1)
    double d[3][3];
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const bool row = t + q >= 2 && t + q <= T - 1 && (JAC || q == 0);
#pragma unroll
        for (int k = 0; k < 3; k++) d[q][k] = row ? Xw[q + 2][k] - 2.0 * Xw[q + 1][k] + Xw[q][k] : 0.0;
    }
    if (a.cost) {
        a.cost[NC * e + 0] = f.front ? f.rho : (double)INFINITY;
        a.cost[NC * e + 1] = 0.5 * a.lambda * (d[0][0] * d[0][0] + d[0][1] * d[0][1] + d[0][2] * d[0][2]);
        if constexpr (NC > 2) a.cost[NC * e + 2] = cp.weight() * cc;
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

// The _system calls' costs: one workgroup per group of joints() chains, each lane its (frame, joint)
// pairs in ascending order (a chain alone: lane x takes t = x, x + kBlock, ...), then a tree over
// the lanes in a fixed order.  out_cost [groups][kCosts].
template <class C>
__global__ __launch_bounds__(kBlock) void fit_system_cost_kernel(FitObs o, const float* __restrict__ x32,
                                                                 double* __restrict__ out_cost, C cp) {
#pragma clang fp contract(fast)
    constexpr int NC = C::kCosts;
    using Item = typename C::Item;
    __shared__ double scam[kMaxCams][MVP_CAM_DOUBLES];
    __shared__ CamFast sfast[kMaxCams];
    __shared__ double s_red[NC][kBlock];
    load_cams(scam, sfast, o.cams, o.n_cams);
    const int g = blockIdx.x, J = cp.joints();
    const Item items = (Item)o.T * J;
    double rho = 0.0, sm = 0.0, cc = 0.0;
    for (Item i = threadIdx.x; i < items; i += kBlock) {
        const int t = (int)(i / J), j = (int)(i - (Item)t * J);
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
        cc += cp.template frame_terms<false>(
            (int64_t)t * o.P + p, g, j, (const int*)nullptr, X,
            [&](int64_t eo, double (&Y)[3]) {
#pragma unroll
                for (int k = 0; k < 3; k++) Y[k] = (double)x32[3 * eo + k];
            },
            f);
    }
    s_red[0][threadIdx.x] = rho;
    s_red[1][threadIdx.x] = sm;
    if constexpr (NC > 2) s_red[2][threadIdx.x] = cc;
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
#pragma unroll
            for (int k = 0; k < NC; k++) s_red[k][threadIdx.x] += s_red[k][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < NC; k++) out_cost[NC * g + k] = s_red[k][0];
    }
}

// ------------------------------------------------------------------------------- sum
// part[tile][p][NC] = the NC numbers of cost over the tile's frames of chain p: each of the
// workgroup's 4 rows of lanes adds its frames in ascending order, then rows 1..3 onto row 0.
template <int NC>
__global__ __launch_bounds__(kFitRows * 64) void fit_sum_kernel(const double* __restrict__ cost, int T, int P,
                                                                const int* __restrict__ done,
                                                                double* __restrict__ part) {
    __shared__ double s_red[NC][kFitRows][64];
    const int px = threadIdx.x & 63, row = threadIdx.x >> 6;
    const int p_tiles = (P + 63) / 64;   // tiles of chains and of frames share grid.x: no limit of grid.y on P
    const int tile = blockIdx.x / p_tiles;
    const int p = (blockIdx.x - tile * p_tiles) * 64 + px;
    const int t0 = tile * kFitTile;
    const int t1 = t0 + kFitTile < T ? t0 + kFitTile : T;
    const bool live = p < P && !(done && done[p]);
    double s[NC];
#pragma unroll
    for (int k = 0; k < NC; k++) s[k] = 0.0;
    if (live) {
#pragma unroll 4
        for (int t = t0 + row; t < t1; t += kFitRows) {
            const int64_t e = (int64_t)t * P + p;
#pragma unroll
            for (int k = 0; k < NC; k++) s[k] += cost[NC * e + k];
        }
    }
#pragma unroll
    for (int k = 0; k < NC; k++) s_red[k][row][px] = s[k];
    __syncthreads();
    if (row == 0 && live) {
#pragma unroll
        for (int r = 1; r < kFitRows; r++)
#pragma unroll
            for (int k = 0; k < NC; k++) s[k] += s_red[k][r][px];
#pragma unroll
        for (int k = 0; k < NC; k++) part[NC * ((int64_t)tile * P + p) + k] = s[k];
    }
}

// ------------------------------------------------------------------------------- the decision rules
// Used by fit_decide_kernel (one lane per chain) and sk_decide_kernel (one workgroup per group).

// Chain p's sums of the tiles' NC numbers, tiles ascending (the same inputs give the same bits).
template <int NC>
__device__ __forceinline__ void fit_sum_tiles(const double* __restrict__ part, int n_tiles, int P, int p, double (&s)[NC]) {
#pragma unroll
    for (int k = 0; k < NC; k++) s[k] = 0.0;
#pragma unroll 8   // eight loads in flight; the additions stay in index order
    for (int w = 0; w < n_tiles; w++) {
#pragma unroll
        for (int k = 0; k < NC; k++) s[k] += part[NC * ((int64_t)w * P + p) + k];
    }
}

// A chain is valid when at least two of its frames have >= 2 used views and no frame's seed is
// non-finite or behind a used view: prepare's two sums.
__device__ __forceinline__ bool fit_chain_valid(double s0, double s1) { return s0 >= 2.0 && s1 == 0.0; }

// A seed whose cost overflows is no seed.
__device__ __forceinline__ bool fit_seed_ok(double f) { return isfinite(f); }

// Mode 0's state of chain p; `status` is what a valid chain starts with.
__device__ __forceinline__ void fit_chain_reset(const FitChain& ch, int p, bool valid, int status) {
    ch.mu[p] = 1e-3;
    ch.f[p] = ch.fseed[p] = __builtin_nan("");
    ch.cur[p] = 0;
    ch.done[p] = valid ? 0 : 1;
    ch.status[p] = valid ? status : 0x80;
    ch.relin[p] = 1;
    ch.rej[p] = 0;
}

// One Levenberg-Marquardt decision: the trial's cost ft against the state's f; `rejected`: a pivot
// of the trial's solve failed.  The status byte counts the trials in its low six bits and keeps
// 0x40 until a step converges.
struct LmStep {
    bool accept, done;
    double mu;
    int status;
};

__device__ __forceinline__ LmStep lm_step(double f, double ft, bool rejected, double mu, int status, int max_iter,
                                          double tol) {
    const int trials = (status & 63) + 1;
    LmStep r;
    r.accept = !rejected && isfinite(ft) && ft <= f;
    bool conv = false;
    if (r.accept) {
        conv = (f - ft) <= tol * f;
        mu = fmax(mu * 0.1, 1e-12);
        r.done = conv;
    } else {
        mu = mu * 10.0;
        r.done = mu > 1e12;
    }
    r.done = r.done || trials >= max_iter;
    r.mu = mu;
    r.status = trials | (conv ? 0 : 0x40);
    return r;
}

// ------------------------------------------------------------------------------- output
// One lane per (t, p): out_xyz (an invalid chain's seed bits come back), Σ s² at the final state,
// the view counts; then the policy's outputs.
template <class C>
__global__ __launch_bounds__(kBlock) void fit_output_kernel(FitObs o, const float* __restrict__ xyz0,
                                                            const double* __restrict__ x64, FitChain ch,
                                                            float* __restrict__ out_xyz, float* __restrict__ out_resid,
                                                            uint8_t* __restrict__ out_nviews,
                                                            double* __restrict__ out_cost,
                                                            uint8_t* __restrict__ out_status, C cp) {
#pragma clang fp contract(fast)
    __shared__ double scam[kMaxCams][MVP_CAM_DOUBLES];
    __shared__ CamFast sfast[kMaxCams];
    load_cams(scam, sfast, o.cams, o.n_cams);
    const int64_t n = (int64_t)o.T * o.P;
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= n) return;
    const int t = (int)(e / o.P), p = (int)(e - (int64_t)t * o.P);
    const int J = cp.joints(), g = p / J, j = p - g * J;
    const int status = ch.status[p];
    const bool valid = status != 0x80;
    const int64_t buf = (int64_t)ch.cur[p] * n;
    const double* xp = x64 + 3 * (buf + e);
    const double X[3] = {xp[0], xp[1], xp[2]};
    FitFrame f;
    fit_frame<false>(o, scam, t, p, X, f);
    const uint32_t* in = reinterpret_cast<const uint32_t*>(xyz0);
    uint32_t* out = reinterpret_cast<uint32_t*>(out_xyz);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        if (valid)
            out_xyz[3 * e + k] = (float)X[k];
        else
            out[3 * e + k] = in[3 * e + k];   // the seed's bits, NaN payloads included
    }
    if (out_resid) out_resid[e] = (valid && f.nviews > 0) ? (float)f.s2 : __builtin_nanf("");
    if (out_nviews) out_nviews[e] = (uint8_t)f.nviews;
    cp.output_frame(o, ch, x64, buf, e, t, g, j, valid, X);
    if (t == 0) cp.output_chain(ch, p, g, j, status, out_cost, out_status);
}

// ------------------------------------------------------------------------------- host side
// The checks of a fit's own arguments.  J > 0: the skeleton fit's, named in the workspace message.
inline void fit_check_args(const char* fn, double lambda_smooth, int max_iter, double tol, int64_t workspace_bytes,
                           int64_t need, int T, int P, int J, int chunk) {
    MVP_REQUIRE(std::isfinite(lambda_smooth) && lambda_smooth > 0, "%s: lambda_smooth=%g must be finite and > 0", fn,
                lambda_smooth);
    MVP_REQUIRE(max_iter >= 0 && max_iter <= 63, "%s: max_iter=%d (0..63)", fn, max_iter);
    MVP_REQUIRE(std::isfinite(tol) && tol > 0, "%s: tol=%g (finite, > 0)", fn, tol);
    if (J > 0) {
        MVP_REQUIRE(workspace_bytes >= need, "%s: workspace_bytes=%lld < %lld needed (T=%d, P=%d, J=%d, chunk=%d)", fn,
                    (long long)workspace_bytes, (long long)need, T, P, J, chunk);
    } else {
        MVP_REQUIRE(workspace_bytes >= need, "%s: workspace_bytes=%lld < %lld needed (T=%d, P=%d, chunk=%d)", fn,
                    (long long)workspace_bytes, (long long)need, T, P, chunk);
    }
}

// The sum launch over the frames' costs; done: the chains to leave out, or null.
template <int NC>
void fit_launch_sum(hipStream_t s, const FitPlan& pl, const double* cost, int T, int P, const int* done, double* part) {
    hipLaunchKernelGGL(fit_sum_kernel<NC>, dim3((unsigned)pl.sum_blocks), dim3(kFitRows * 64), 0, s, cost, T, P, done, part);
}

// The kernels fit_run launches for the data term and the solve: these over the coupling policy C.
// mvp_trajectory_fit_lag has its own set (trajectory_fit_lag.hip).
//   Solve, kCosts                 the solver's frame source and the cost terms a frame has
//   bind(sa, ws)                  what the source has beyond FitSolveArgs' fields
//   prepare(...), terms<JAC>(...) the launches
template <class C>
struct FitLaunch {
    using Solve = FitSolveArgs;
    static constexpr int kCosts = C::kCosts;
    C cp;
    void bind(Solve&, char*) const {}
    void prepare(dim3 grid, dim3 blk, hipStream_t s, const FitTerms& ta, const float* xyz0) const {
        hipLaunchKernelGGL(fit_prepare_kernel<kCosts>, grid, blk, 0, s, ta.o, xyz0, const_cast<double*>(ta.x64), ta.cost);
    }
    template <bool JAC>
    void terms(dim3 grid, dim3 blk, hipStream_t s, const FitTerms& ta) const {
        hipLaunchKernelGGL((fit_terms_kernel<JAC, C>), grid, blk, 0, s, ta, cp);
    }
};

// The launch sequence of a fit: prepare, sum, decide(0), terms<JAC>, sum, decide(1), then max_iter
// x (eliminate, reduce, backsub, terms at the trial, sum, decide(2), terms<JAC> at the state) and
// output, over the workspace ws of plan pl, with the kernels of K (a FitLaunch, or what has its
// members).  decide(mode, ch, part, bad) launches the caller's decide kernel and
// output(grid, block, ch, x64) its output kernel.
template <class K, class Decide, class Output>
void fit_run_with(const char* fn, hipStream_t s, const FitPlan& pl, char* ws, const FitObs& o, const K& k,
                  double lambda_smooth, const float* xyz0, int max_iter, Decide decide, Output output) {
    using Solve = typename K::Solve;
    const int T = o.T, P = o.P;
    double* part = reinterpret_cast<double*>(ws + pl.off_part);
    Solve sa{};
    bind_core(sa, ws, pl.sp, T, P, lambda_smooth);
    sa.H = reinterpret_cast<double*>(ws + pl.off_H);
    sa.g = reinterpret_cast<double*>(ws + pl.off_g);
    sa.x64 = reinterpret_cast<double*>(ws + pl.off_x);
    sa.ch = bind_chain(ws + pl.off_chain, P);
    k.bind(sa, ws);
    FitTerms ta{};
    ta.o = o;
    ta.x64 = sa.x64;
    ta.ch = sa.ch;
    ta.lambda = lambda_smooth;
    ta.H = reinterpret_cast<double*>(ws + pl.off_H);
    ta.g = reinterpret_cast<double*>(ws + pl.off_g);
    ta.cost = reinterpret_cast<double*>(ws + pl.off_cost);
    const dim3 flat(tri_grid(fn, (int64_t)T * P)), blk(kBlock);
    const dim3 chain_grid((unsigned)((P + kSmBlock - 1) / kSmBlock)), lane_grid((unsigned)pl.sp.n_blocks), sm_blk(kSmBlock);
    auto sum_decide = [&](int mode) {
        fit_launch_sum<K::kCosts>(s, pl, ta.cost, T, P, mode == 0 ? (const int*)nullptr : sa.ch.done, part);
        decide(mode, sa.ch, part, sa.bad);
        MVP_HIP(hipGetLastError());
    };
    MVP_HIP(hipMemsetAsync(sa.cnt, 0, (size_t)P * 8, s));
    k.prepare(flat, blk, s, ta, xyz0);
    MVP_HIP(hipGetLastError());
    sum_decide(0);
    ta.trial = 0;
    k.template terms<true>(flat, blk, s, ta);
    sum_decide(1);
    for (int it = 0; it < max_iter; it++) {
        hipLaunchKernelGGL(solve_eliminate_kernel<Solve>, lane_grid, sm_blk, 0, s, sa);
        hipLaunchKernelGGL(solve_reduce_kernel<Solve>, chain_grid, sm_blk, 0, s, sa);
        hipLaunchKernelGGL(solve_backsub_kernel<Solve>, lane_grid, sm_blk, 0, s, sa);
        ta.trial = 1;
        k.template terms<false>(flat, blk, s, ta);
        sum_decide(2);
        if (it + 1 < max_iter) {
            ta.trial = 0;
            k.template terms<true>(flat, blk, s, ta);
            MVP_HIP(hipGetLastError());
        }
    }
    output(flat, blk, sa.ch, sa.x64);
    MVP_HIP(hipGetLastError());
}

template <class C, class Decide, class Output>
void fit_run(const char* fn, hipStream_t s, const FitPlan& pl, char* ws, const FitObs& o, const C& cp,
             double lambda_smooth, const float* xyz0, int max_iter, Decide decide, Output output) {
    fit_run_with(fn, s, pl, ws, o, FitLaunch<C>{cp}, lambda_smooth, xyz0, max_iter, decide, output);
}

}  // namespace
