// The trajectory fit with sub-frame time offsets between the cameras (mvp_trajectory_fit_lag_plan /
// _lag_system / mvp_trajectory_fit_lag; the problem is stated in include/mvpose.h; no reference
// counterpart) for gfx950.
//
// View i's frame t was taken a_i of a frame after rig instant t (0 <= a_i < 1), so its observation
// scores Y = (1 − a_i)·X_t + a_i·X_{t+1}, the chain's position interpolated between the two nodes.
// Its H_i = Jᵀ W̃ J and g_i = Jᵀ W̃ r at Y then belong to node t with (1−a_i)², (1−a_i), to node t+1
// with a_i², a_i, and to the pair with a_i(1−a_i): the Gauss-Newton matrix gains one symmetric 3x3
// block C_t between neighbouring frames, inside the band the prior has already.  The loop, the
// decisions and the solver are mvp_trajectory_fit's (trajectory_fit_kernels.h: fit_run_with,
// fit_sum_kernel; trajectory_fit_decide.h: fit_decide_kernel; smooth_solver.h over FitLagSolveArgs, the source with a cross
// block); this file has the kernels that see the offsets:
//
//   lag_prepare_kernel   one lane per (t, p): as fit_prepare_kernel, P_z tested at the seed's Ys.
//   lag_terms_kernel<JAC>   one lane per NODE (t, p).  A lane gathers what lands on its node: the
//              observations of frame t at their Y (weights (1−a)², (1−a); their a(1−a)·H_i is
//              C_t) and, for the views with a > 0, the observations of frame t−1 at theirs
//              (weights a², a), evaluated a second time here so that no lane writes to a neighbour's
//              record: no scatter, no atomics, one fixed order.  The cost terms are frame t's own.
//              Views with a = 0 take one evaluation, as in mvp_trajectory_fit.
//   lag_dlag_kernel, lag_dlag_finish_kernel   the offset derivative at the final state: per view
//              (grid.y) and tile of 256 frames the sums of dᵀW̃r and dᵀW̃d, d = J·(X_{t+1} − X_t), in
//              fit_sum_kernel's order (each of 4 rows of lanes its frames ascending, the rows in
//              order), then per (chain, view) the tiles ascending.
//   lag_system_cost_kernel, lag_system_dlag_kernel   the _system call's sums, one workgroup per
//              chain (and view), as fit_system_cost_kernel.
//   lag_output_kernel   one lane per (t, p): out_xyz, Σ s² of frame t's observations at the final
//              state, the view counts; per chain the costs and the status.
//
// Arithmetic in fp64, FMA contraction on (no bit contract), no floating-point atomics.  Register /
// LDS / scratch figures and the measurements are in DESIGN.md §4.17.
#include "trajectory_fit_decide.h"

namespace {

static_assert(kLagViews == kMaxCams, "the plan's view count is the view list's");

struct LagFrac {
    double a[kMaxCams];   // per listed view
};

// What lands on node (t, p): frame t's cost terms, and with JAC the node's H̃ and g̃ and the block
// C between nodes t and t+1.
struct LagNode {
    double rho, s2, H[6], g[3], C[6];
    int nviews;
    bool front;
};

// Y = (1 − a)·X0 + a·X1; X0 itself for a = 0 (X1 is then not looked at).
__device__ __forceinline__ void lag_point(double a, const double (&X0)[3], const double (&X1)[3], double (&Y)[3]) {
#pragma unroll
    for (int k = 0; k < 3; k++) Y[k] = a > 0 ? (1.0 - a) * X0[k] + a * X1[k] : X0[k];
}

// Xm, X0, Xp: the state at t−1, t, t+1 (whatever is at hand where the frame does not exist: it is
// not used).  sfrac: the offsets in LDS.
template <bool JAC>
__device__ __forceinline__ void lag_node(const FitObs& o, const double (*scam)[MVP_CAM_DOUBLES], const double* sfrac,
                                         int t, int p, const double (&Xm)[3], const double (&X0)[3],
                                         const double (&Xp)[3], LagNode& f) {
#pragma clang fp contract(fast)
    const int64_t e = (int64_t)t * o.P + p;
    const int64_t em = t > 0 ? e - o.P : e;
    const unsigned allowed = reproj_allowed(o.obs, e);
    const unsigned allowed_m = reproj_allowed(o.obs, em);
    const bool last = t == o.T - 1;
    f.rho = 0.0, f.s2 = 0.0, f.nviews = 0, f.front = true;
#pragma unroll
    for (int k = 0; k < 6; k++) f.H[k] = 0.0, f.C[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 3; k++) f.g[k] = 0.0;
#pragma unroll 1
    for (int j = 0; j < o.vl.nv; j++) {
        const int col = o.vl.col(j);
        const double a = sfrac[j], b = 1.0 - a;
        const RefineCam c = refine_cam(&scam[col][0]);
        {
            double zx, zy, wxx, wxy, wyy, Y[3];
            bool u = reproj_observe(o.obs, e, t, p, col, (allowed >> j) & 1u, zx, zy, wxx, wxy, wyy);
            u = u && !(last && a > 0);   // its neighbour does not exist
            lag_point(a, X0, Xp, Y);
            double rho = 0.0, s2 = 0.0, g[3] = {0, 0, 0}, H[6] = {0, 0, 0, 0, 0, 0};
            const bool infront = refine_view_terms_huber<JAC>(c, Y, zx, zy, wxx, wxy, wyy, o.obs.hub, rho, s2, g, H);
            f.front = f.front && (infront || !u);
            f.nviews += u ? 1 : 0;
            f.rho += u ? rho : 0.0;
            f.s2 += u ? s2 : 0.0;
            if (JAC) {
#pragma unroll
                for (int k = 0; k < 3; k++) f.g[k] += u ? b * g[k] : 0.0;
#pragma unroll
                for (int k = 0; k < 6; k++) {
                    f.H[k] += u ? (b * b) * H[k] : 0.0;
                    f.C[k] += (u && a > 0) ? (a * b) * H[k] : 0.0;   // a = 0: exactly nothing, whatever H is
                }
            }
        }
        if (JAC && a > 0 && t > 0) {
            // frame t−1's observation by the same view: its share of this node
            double zx, zy, wxx, wxy, wyy, Y[3];
            const bool u = reproj_observe(o.obs, em, t - 1, p, col, (allowed_m >> j) & 1u, zx, zy, wxx, wxy, wyy);
            lag_point(a, Xm, X0, Y);
            double rho = 0.0, s2 = 0.0, g[3] = {0, 0, 0}, H[6] = {0, 0, 0, 0, 0, 0};
            refine_view_terms_huber<true>(c, Y, zx, zy, wxx, wxy, wyy, o.obs.hub, rho, s2, g, H);
#pragma unroll
            for (int k = 0; k < 3; k++) f.g[k] += u ? a * g[k] : 0.0;
#pragma unroll
            for (int k = 0; k < 6; k++) f.H[k] += u ? (a * a) * H[k] : 0.0;
        }
    }
}

// What every kernel here keeps in LDS: the camera records and the offsets.
struct LagLds {
    double cam[kMaxCams][MVP_CAM_DOUBLES];
    double frac[kMaxCams];
};

__device__ __forceinline__ void lag_load(LagLds& s, const FitObs& o, const LagFrac& fr) {
    const int total = o.n_cams * MVP_CAM_DOUBLES;
    for (int i = threadIdx.x; i < total; i += blockDim.x) s.cam[i / MVP_CAM_DOUBLES][i % MVP_CAM_DOUBLES] = o.cams[i];
    if (threadIdx.x < kMaxCams) s.frac[threadIdx.x] = fr.a[threadIdx.x];
    __syncthreads();
}

// ------------------------------------------------------------------------------- prepare
__global__ __launch_bounds__(kBlock) void lag_prepare_kernel(FitObs o, LagFrac fr, const float* __restrict__ xyz0,
                                                             double* __restrict__ x64, double* __restrict__ cost) {
#pragma clang fp contract(fast)
    __shared__ LagLds lds;
    lag_load(lds, o, fr);
    const int64_t n = (int64_t)o.T * o.P;
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= n) return;
    const int t = (int)(e / o.P), p = (int)(e - (int64_t)t * o.P);
    const int64_t ep = t + 1 < o.T ? e + o.P : e;
    const float s0 = xyz0[3 * e + 0], s1 = xyz0[3 * e + 1], s2 = xyz0[3 * e + 2];
    const double X[3] = {(double)s0, (double)s1, (double)s2};
    const double Xp[3] = {(double)xyz0[3 * ep + 0], (double)xyz0[3 * ep + 1], (double)xyz0[3 * ep + 2]};
    LagNode f;
    lag_node<false>(o, lds.cam, lds.frac, t, p, X, X, Xp, f);
    const bool fin = isfinite(s0) && isfinite(s1) && isfinite(s2);
    x64[3 * e + 0] = X[0], x64[3 * e + 1] = X[1], x64[3 * e + 2] = X[2];
    x64[3 * (n + e) + 0] = X[0], x64[3 * (n + e) + 1] = X[1], x64[3 * (n + e) + 2] = X[2];
    cost[2 * e + 0] = f.nviews >= 2 ? 1.0 : 0.0;
    cost[2 * e + 1] = (fin && f.front) ? 0.0 : 1.0;
}

// ------------------------------------------------------------------------------- terms
struct LagTerms {
    FitTerms t;     // as fit_terms_kernel takes it
    LagFrac fr;
    double* Cx;     // [T][P][6] with JAC: the block between t and t+1
};

template <bool JAC>
__global__ __launch_bounds__(kBlock) void lag_terms_kernel(LagTerms la) {
#pragma clang fp contract(fast)
    __shared__ LagLds lds;
    const FitTerms& a = la.t;
    lag_load(lds, a.o, la.fr);
    const int T = a.o.T, P = a.o.P;
    const int64_t n = (int64_t)T * P;
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= n) return;
    const int t = (int)(e / P), p = (int)(e - (int64_t)t * P);
    if (!a.x32) {
        if (a.ch.done[p]) return;
        if (JAC && !a.ch.relin[p]) return;
    }
    // the frames t-2 .. t+2 of the chain (the cost reads t-2 .. t+1 only)
    double Xw[5][3];
    const int64_t buf = a.x32 ? 0 : (int64_t)(a.ch.cur[p] ^ a.trial) * n;
#pragma unroll
    for (int q = 0; q < 5; q++) {
        const int tq = t + q - 2;
        const bool in = tq >= 0 && tq < T && (JAC || q <= 3);
        const int64_t eq = in ? e + (int64_t)(q - 2) * P : e;
#pragma unroll
        for (int k = 0; k < 3; k++) Xw[q][k] = a.x32 ? (double)a.x32[3 * eq + k] : a.x64[3 * (buf + eq) + k];
    }
    LagNode f;
    lag_node<JAC>(a.o, lds.cam, lds.frac, t, p, Xw[1], Xw[2], Xw[3], f);
    // second-difference rows t, t+1, t+2 (row s exists for 2 <= s <= T-1)
    double d[3][3];
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const bool row = t + q >= 2 && t + q <= T - 1 && (JAC || q == 0);
#pragma unroll
        for (int k = 0; k < 3; k++) d[q][k] = row ? Xw[q + 2][k] - 2.0 * Xw[q + 1][k] + Xw[q][k] : 0.0;
    }
    if (a.cost) {
        a.cost[2 * e + 0] = f.front ? f.rho : (double)INFINITY;
        a.cost[2 * e + 1] = 0.5 * a.lambda * (d[0][0] * d[0][0] + d[0][1] * d[0][1] + d[0][2] * d[0][2]);
    }
    if (a.nviews) a.nviews[e] = (uint8_t)f.nviews;
    if (JAC) {
#pragma unroll
        for (int k = 0; k < 6; k++) {
            a.H[6 * e + k] = f.H[k];
            la.Cx[6 * e + k] = f.C[k];
        }
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double prior = a.lambda * (d[0][k] - 2.0 * d[1][k] + d[2][k]);
            a.g[3 * e + k] = a.x32 ? f.g[k] : -(f.g[k] + prior);
        }
    }
}

// ------------------------------------------------------------------------------- the offset derivative
// View j's terms of frame (t, p) at the state X0 = X_t, Xp = X_{t+1}: dᵀW̃r and dᵀW̃d with
// d = J·(Xp − X0), i.e. ΔᵀG_i and ΔᵀH_iΔ; zeros when the view is not used or t is the last frame.
__device__ __forceinline__ void lag_dlag_terms(const FitObs& o, const double (*scam)[MVP_CAM_DOUBLES], double a, int j,
                                               int t, int p, const double (&X0)[3], const double (&Xp)[3], double& ga,
                                               double& ha) {
#pragma clang fp contract(fast)
    const int64_t e = (int64_t)t * o.P + p;
    const int col = o.vl.col(j);
    double zx, zy, wxx, wxy, wyy, Y[3];
    bool u = reproj_observe(o.obs, e, t, p, col, (reproj_allowed(o.obs, e) >> j) & 1u, zx, zy, wxx, wxy, wyy);
    u = u && t + 1 < o.T;
    lag_point(a, X0, Xp, Y);
    const RefineCam c = refine_cam(&scam[col][0]);
    double rho = 0.0, s2 = 0.0, g[3] = {0, 0, 0}, H[6] = {0, 0, 0, 0, 0, 0};
    refine_view_terms_huber<true>(c, Y, zx, zy, wxx, wxy, wyy, o.obs.hub, rho, s2, g, H);
    const double D[3] = {Xp[0] - X0[0], Xp[1] - X0[1], Xp[2] - X0[2]};
    const double hd0 = H[0] * D[0] + H[1] * D[1] + H[2] * D[2];
    const double hd1 = H[1] * D[0] + H[3] * D[1] + H[4] * D[2];
    const double hd2 = H[2] * D[0] + H[4] * D[1] + H[5] * D[2];
    ga = u ? D[0] * g[0] + D[1] * g[1] + D[2] * g[2] : 0.0;
    ha = u ? D[0] * hd0 + D[1] * hd1 + D[2] * hd2 : 0.0;
}

// part[tile][p][kMaxCams][2] for view blockIdx.y, over the chains' final states; fit_sum_kernel's
// grid and order.
__global__ __launch_bounds__(kFitRows * 64) void lag_dlag_kernel(FitObs o, LagFrac fr, const double* __restrict__ x64,
                                                                  FitChain ch, double* __restrict__ part) {
#pragma clang fp contract(fast)
    __shared__ LagLds lds;
    __shared__ double s_red[2][kFitRows][64];
    lag_load(lds, o, fr);
    const int T = o.T, P = o.P, j = blockIdx.y;
    const int px = threadIdx.x & 63, row = threadIdx.x >> 6;
    const int p_tiles = (P + 63) / 64;
    const int tile = blockIdx.x / p_tiles;
    const int p = (blockIdx.x - tile * p_tiles) * 64 + px;
    const int t0 = tile * kFitTile;
    const int t1 = t0 + kFitTile < T ? t0 + kFitTile : T;
    const bool live = p < P;
    double s[2] = {0.0, 0.0};
    if (live) {
        const int64_t buf = (int64_t)ch.cur[p] * T * P;
        const double a = lds.frac[j];
        for (int t = t0 + row; t < t1; t += kFitRows) {
            const int64_t e = (int64_t)t * P + p, ep = t + 1 < T ? e + P : e;
            const double X0[3] = {x64[3 * (buf + e)], x64[3 * (buf + e) + 1], x64[3 * (buf + e) + 2]};
            const double Xp[3] = {x64[3 * (buf + ep)], x64[3 * (buf + ep) + 1], x64[3 * (buf + ep) + 2]};
            double ga, ha;
            lag_dlag_terms(o, lds.cam, a, j, t, p, X0, Xp, ga, ha);
            s[0] += ga;
            s[1] += ha;
        }
    }
    s_red[0][row][px] = s[0];
    s_red[1][row][px] = s[1];
    __syncthreads();
    if (row == 0 && live) {
#pragma unroll
        for (int r = 1; r < kFitRows; r++) {
            s[0] += s_red[0][r][px];
            s[1] += s_red[1][r][px];
        }
        double* out = part + 2 * (((int64_t)tile * P + p) * kMaxCams + j);
        out[0] = s[0];
        out[1] = s[1];
    }
}

// out_dlag [P][nv][2]: the tiles in ascending order; NaN for an invalid chain.
__global__ __launch_bounds__(kSmBlock) void lag_dlag_finish_kernel(const double* __restrict__ part, int n_tiles, int P,
                                                                   int nv, const int* __restrict__ status,
                                                                   double* __restrict__ out) {
    const int i = blockIdx.x * kSmBlock + threadIdx.x;
    if (i >= P * nv) return;
    const int p = i / nv, j = i - p * nv;
    double s[2] = {0.0, 0.0};
    for (int w = 0; w < n_tiles; w++) {
        const double* q = part + 2 * (((int64_t)w * P + p) * kMaxCams + j);
        s[0] += q[0];
        s[1] += q[1];
    }
    const bool valid = status[p] != 0x80;
    out[2 * i + 0] = valid ? s[0] : __builtin_nan("");
    out[2 * i + 1] = valid ? s[1] : __builtin_nan("");
}

// ------------------------------------------------------------------------------- the _system call's sums
// Lane x's partial sums of NS numbers over the workgroup, a tree in a fixed order; the result in
// every s_red[k][0].
template <int NS>
__device__ __forceinline__ void lag_tree(double (*s_red)[kBlock], const double (&s)[NS]) {
#pragma unroll
    for (int k = 0; k < NS; k++) s_red[k][threadIdx.x] = s[k];
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
#pragma unroll
            for (int k = 0; k < NS; k++) s_red[k][threadIdx.x] += s_red[k][threadIdx.x + w];
        }
        __syncthreads();
    }
}

__device__ __forceinline__ void lag_load32(const float* __restrict__ x32, int64_t e, double (&X)[3]) {
#pragma unroll
    for (int k = 0; k < 3; k++) X[k] = (double)x32[3 * e + k];
}

// out_cost [P][2]: one workgroup per chain, lane x takes t = x, x + kBlock, ...
__global__ __launch_bounds__(kBlock) void lag_system_cost_kernel(FitObs o, LagFrac fr, const float* __restrict__ x32,
                                                                 double* __restrict__ out_cost) {
#pragma clang fp contract(fast)
    __shared__ LagLds lds;
    __shared__ double s_red[2][kBlock];
    lag_load(lds, o, fr);
    const int p = blockIdx.x;
    double s[2] = {0.0, 0.0};
    for (int t = threadIdx.x; t < o.T; t += kBlock) {
        const int64_t e = (int64_t)t * o.P + p;
        double X0[3], Xp[3], X1[3], X2[3];
        lag_load32(x32, e, X0);
        lag_load32(x32, t + 1 < o.T ? e + o.P : e, Xp);
        LagNode f;
        lag_node<false>(o, lds.cam, lds.frac, t, p, X0, X0, Xp, f);
        s[0] += f.front ? f.rho : (double)INFINITY;
        if (t >= 2) {
            lag_load32(x32, e - o.P, X1);
            lag_load32(x32, e - 2 * (int64_t)o.P, X2);
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const double d = X0[k] - 2.0 * X1[k] + X2[k];
                s[1] += 0.5 * d * d;
            }
        }
    }
    lag_tree<2>(s_red, s);
    if (threadIdx.x == 0) {
        out_cost[2 * p + 0] = s_red[0][0];
        out_cost[2 * p + 1] = s_red[1][0];
    }
}

// out_dlag [P][nv][2]: one workgroup per (chain, view).
__global__ __launch_bounds__(kBlock) void lag_system_dlag_kernel(FitObs o, LagFrac fr, const float* __restrict__ x32,
                                                                 double* __restrict__ out_dlag) {
#pragma clang fp contract(fast)
    __shared__ LagLds lds;
    __shared__ double s_red[2][kBlock];
    lag_load(lds, o, fr);
    const int p = blockIdx.x, j = blockIdx.y;
    const double a = lds.frac[j];
    double s[2] = {0.0, 0.0};
    for (int t = threadIdx.x; t < o.T; t += kBlock) {
        const int64_t e = (int64_t)t * o.P + p;
        double X0[3], Xp[3], ga, ha;
        lag_load32(x32, e, X0);
        lag_load32(x32, t + 1 < o.T ? e + o.P : e, Xp);
        lag_dlag_terms(o, lds.cam, a, j, t, p, X0, Xp, ga, ha);
        s[0] += ga;
        s[1] += ha;
    }
    lag_tree<2>(s_red, s);
    if (threadIdx.x == 0) {
        out_dlag[2 * ((int64_t)p * o.vl.nv + j) + 0] = s_red[0][0];
        out_dlag[2 * ((int64_t)p * o.vl.nv + j) + 1] = s_red[1][0];
    }
}

// ------------------------------------------------------------------------------- output
__global__ __launch_bounds__(kBlock) void lag_output_kernel(FitObs o, LagFrac fr, const float* __restrict__ xyz0,
                                                            const double* __restrict__ x64, FitChain ch,
                                                            float* __restrict__ out_xyz, float* __restrict__ out_resid,
                                                            uint8_t* __restrict__ out_nviews,
                                                            double* __restrict__ out_cost,
                                                            uint8_t* __restrict__ out_status) {
#pragma clang fp contract(fast)
    __shared__ LagLds lds;
    lag_load(lds, o, fr);
    const int64_t n = (int64_t)o.T * o.P;
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= n) return;
    const int t = (int)(e / o.P), p = (int)(e - (int64_t)t * o.P);
    const int status = ch.status[p];
    const bool valid = status != 0x80;
    const int64_t buf = (int64_t)ch.cur[p] * n;
    const double* xp = x64 + 3 * (buf + e);
    const double* xn = x64 + 3 * (buf + (t + 1 < o.T ? e + o.P : e));
    const double X[3] = {xp[0], xp[1], xp[2]}, Xp[3] = {xn[0], xn[1], xn[2]};
    LagNode f;
    lag_node<false>(o, lds.cam, lds.frac, t, p, X, X, Xp, f);
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
    if (t == 0) NoCoupling{}.output_chain(ch, p, 0, 0, status, out_cost, out_status);
}

// ------------------------------------------------------------------------------- host side
// frac_host [nv]: each finite, 0 <= a < 1.
LagFrac lag_parse_frac(const char* fn, const double* frac, int nv) {
    MVP_REQUIRE(frac != nullptr, "%s: frac_host is NULL", fn);
    LagFrac fr{};
    for (int j = 0; j < nv; j++) {
        MVP_REQUIRE(std::isfinite(frac[j]) && frac[j] >= 0.0 && frac[j] < 1.0, "%s: frac[%d]=%g (finite, 0 <= frac < 1)", fn,
                    j, frac[j]);
        fr.a[j] = frac[j];
    }
    return fr;
}

// fit_run_with's kernels for the fit with offsets.
struct LagLaunch {
    using Solve = FitLagSolveArgs;
    static constexpr int kCosts = 2;
    LagFrac fr;
    double* cx;   // the workspace's [T][P][6] blocks between neighbouring frames
    void bind(Solve& sa, char*) const { sa.Cx = cx; }
    void prepare(dim3 grid, dim3 blk, hipStream_t s, const FitTerms& ta, const float* xyz0) const {
        hipLaunchKernelGGL(lag_prepare_kernel, grid, blk, 0, s, ta.o, fr, xyz0, const_cast<double*>(ta.x64), ta.cost);
    }
    template <bool JAC>
    void terms(dim3 grid, dim3 blk, hipStream_t s, const FitTerms& ta) const {
        LagTerms la{ta, fr, cx};
        hipLaunchKernelGGL(lag_terms_kernel<JAC>, grid, blk, 0, s, la);
    }
};

}  // namespace

extern "C" int mvp_trajectory_fit_lag_plan(int T, int P, int chunk, int* chunk_used, int* n_chunks,
                                           int64_t* workspace_bytes) {
    MVP_ABI_BEGIN
    const FitPlan pl = fit_plan("mvp_trajectory_fit_lag_plan", T, P, chunk);
    const LagPlan lp = lag_plan(pl, T, P);
    if (chunk_used) *chunk_used = pl.sp.chunk;
    if (n_chunks) *n_chunks = pl.sp.n_chunks;
    if (workspace_bytes) *workspace_bytes = lp.bytes;
    MVP_ABI_END
}

extern "C" int mvp_trajectory_fit_lag_system(const float* kpts, int T, int P, int V, const double* cams, int n_cams,
                                             const int* cam_idx, int n_cam_idx, const double* frac, const float* xyz,
                                             const uint8_t* mask, int weights, const double* gauss, float min_conf,
                                             float cov_floor, double huber_delta, double* out_H, double* out_C,
                                             double* out_g, uint8_t* out_nviews, double* out_cost, double* out_dlag,
                                             void* stream) {
    MVP_ABI_BEGIN
    const char* fn = "mvp_trajectory_fit_lag_system";
    const FitObs o = fit_parse(fn, kpts, T, P, V, cams, n_cams, cam_idx, n_cam_idx, mask, weights, gauss, min_conf,
                               cov_floor, huber_delta);
    const LagFrac fr = lag_parse_frac(fn, frac, n_cam_idx);
    MVP_REQUIRE(kpts && cams && xyz && out_H && out_C && out_g && out_nviews && out_cost && out_dlag,
                "%s: null device pointer", fn);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    LagTerms la{};
    la.t.o = o;
    la.t.x32 = xyz;
    la.t.lambda = 1.0;
    la.t.H = out_H;
    la.t.g = out_g;
    la.t.nviews = out_nviews;
    la.fr = fr;
    la.Cx = out_C;
    hipLaunchKernelGGL(lag_terms_kernel<true>, dim3(tri_grid(fn, (int64_t)T * P)), dim3(kBlock), 0, s, la);
    MVP_HIP(hipGetLastError());
    hipLaunchKernelGGL(lag_system_cost_kernel, dim3((unsigned)P), dim3(kBlock), 0, s, o, fr, xyz, out_cost);
    MVP_HIP(hipGetLastError());
    hipLaunchKernelGGL(lag_system_dlag_kernel, dim3((unsigned)P, (unsigned)n_cam_idx), dim3(kBlock), 0, s, o, fr, xyz,
                       out_dlag);
    MVP_HIP(hipGetLastError());
    MVP_ABI_END
}

extern "C" int mvp_trajectory_fit_lag(const float* kpts, int T, int P, int V, const double* cams, int n_cams,
                                      const int* cam_idx, int n_cam_idx, const double* frac, const float* xyz0,
                                      const uint8_t* mask, int weights, const double* gauss, float min_conf,
                                      float cov_floor, double huber_delta, double lambda_smooth, int max_iter, double tol,
                                      int chunk, void* workspace, int64_t workspace_bytes, float* out_xyz,
                                      float* out_resid, uint8_t* out_nviews, double* out_cost, uint8_t* out_status,
                                      double* out_dlag, void* stream) {
    MVP_ABI_BEGIN
    const char* fn = "mvp_trajectory_fit_lag";
    const FitObs o = fit_parse(fn, kpts, T, P, V, cams, n_cams, cam_idx, n_cam_idx, mask, weights, gauss, min_conf,
                               cov_floor, huber_delta);
    const LagFrac fr = lag_parse_frac(fn, frac, n_cam_idx);
    const FitPlan pl = fit_plan(fn, T, P, chunk);
    const LagPlan lp = lag_plan(pl, T, P);
    fit_check_args(fn, lambda_smooth, max_iter, tol, workspace_bytes, lp.bytes, T, P, 0, pl.sp.chunk);
    MVP_REQUIRE(kpts && cams && xyz0 && workspace && out_xyz, "%s: null device pointer", fn);
    MVP_REQUIRE((int64_t)P * n_cam_idx < (1LL << 31), "%s: P·n_cam_idx=%lld must be < 2^31", fn,
                (long long)P * n_cam_idx);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    LagLaunch k{};
    k.fr = fr;
    k.cx = reinterpret_cast<double*>(ws + lp.off_C);
    fit_run_with(
        fn, s, pl, ws, o, k, lambda_smooth, xyz0, max_iter,
        [&](int mode, const FitChain& ch, const double* part, int* bad) {
            hipLaunchKernelGGL(fit_decide_kernel, dim3((unsigned)((P + kSmBlock - 1) / kSmBlock)), dim3(kSmBlock), 0, s, ch,
                               part, pl.n_tiles, P, mode, max_iter, tol, bad);
        },
        [&](dim3 flat, dim3 blk, const FitChain& ch, const double* x64) {
            hipLaunchKernelGGL(lag_output_kernel, flat, blk, 0, s, o, fr, xyz0, x64, ch, out_xyz, out_resid, out_nviews,
                               out_cost, out_status);
            if (out_dlag) {
                double* dpart = reinterpret_cast<double*>(ws + lp.off_dpart);
                hipLaunchKernelGGL(lag_dlag_kernel, dim3((unsigned)pl.sum_blocks, (unsigned)n_cam_idx), dim3(kFitRows * 64),
                                   0, s, o, fr, x64, ch, dpart);
                hipLaunchKernelGGL(lag_dlag_finish_kernel, dim3((unsigned)((P * n_cam_idx + kSmBlock - 1) / kSmBlock)),
                                   dim3(kSmBlock), 0, s, dpart, pl.n_tiles, P, n_cam_idx, ch.status, out_dlag);
            }
        });
    MVP_ABI_END
}
