// Trajectories fitted to the 2D keypoints (mvp_trajectory_fit_plan / _system / mvp_trajectory_fit;
// the problem is stated in include/mvpose.h; no reference counterpart) for gfx950.
//
// Per chain p, Levenberg-Marquardt on
//   f(X) = Σ_t Σ_used rho(reprojection of X_t in view i) + ½ λ Σ_{t>=2} |X_t − 2 X_{t−1} + X_{t−2}|².
// A Gauss-Newton step of it is the block-pentadiagonal system the smoother solves, with the frames'
// 3x3 information blocks H̃_t where the smoother has W_t: frames seen by one view enter with their
// rank-2 block, frames seen by none with nothing, and the prior carries them.  Stream-ordered
// launches, arithmetic in fp64, FMA contraction on (no bit contract), no floating-point atomics:
//
//   prepare    one lane per (t, p): the f64 copy of the seed, the number of used views, and the two
//              numbers a chain's validity is summed from (frames with >= 2 used views; frames whose
//              seed is not finite or lies behind a used view).
//   terms      one lane per (t, p), lanes along p, the camera records in LDS: the used views'
//              rho, and with JAC the frame's H̃ (6) and the right-hand side −(g̃ + λ·(D₂ᵀD₂ X)_t) (3),
//              read from the fp64 state at t±1, t±2.  Writes the frame's two cost terms (Σ rho, or
//              +inf behind a camera; the prior's row t).  The used set depends on the keypoints
//              alone (refine_common.h's rule), so it is re-derived, not stored.
//   sum        per chain, the frames' two numbers in tiles of 256 frames: each of a workgroup's 4
//              rows of lanes adds its frames in ascending order, the rows are added in order.
//   decide     one lane per chain: the tiles' sums in ascending order (the same inputs give the same
//              bits), then mode 0: validity; mode 1: the seed's cost; mode 2: accept / reject, mu,
//              the stop tests, and which of the two state buffers holds the state.
//   eliminate / reduce / backsub   the partition solver of smooth_solver.h over the information-
//              form buffer, the Marquardt factor (1 + mu_p) on the diagonal entries; backsub writes
//              the trial state X + δ into the chain's other buffer.
//   output     one lane per (t, p): out_xyz, Σ s² at the final state, the view counts; per chain
//              the costs and the status.
// mvp_trajectory_fit enqueues prepare, sum, decide(0), terms<JAC>, sum, decide(1), then max_iter
// x (eliminate, reduce, backsub, terms at the trial, sum, decide(2), terms<JAC> at the state) and
// output.  A per-chain flag in the workspace makes a finished chain's lanes return at once, and a
// chain whose last trial was rejected keeps its linearisation.  Nothing is decided on the host.
//
// mvp_trajectory_fit_cov enqueues prepare, sum, decide(0) (the validity pass, at the given state),
// terms<JAC> at that state, then eliminate with no Marquardt factor and the pivots kept, reduce with
// the reduced system's selected inverse behind it, and the covariance sweep of smooth_solver.h.
//
// Register / LDS / scratch figures and the measurements are in DESIGN.md §4.14 and §4.16.
#include "trajectory_fit_terms.h"

namespace {

// ------------------------------------------------------------------------------- prepare
__global__ __launch_bounds__(kBlock) void fit_prepare_kernel(FitObs o, const float* __restrict__ xyz0,
                                                             double* __restrict__ x64, double* __restrict__ c2) {
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
    c2[2 * e + 0] = f.nviews >= 2 ? 1.0 : 0.0;
    c2[2 * e + 1] = (fin && f.front) ? 0.0 : 1.0;
}

// ------------------------------------------------------------------------------- terms
struct FitTerms {
    FitObs o;
    const float* x32;      // mvp_trajectory_fit_system: the state, f32 [T][P][3]; else null
    const double* x64;     // [2][T][P][3]
    FitChain ch;           // (null pointers with x32)
    int trial;             // evaluate the chain's trial buffer, not its state
    double lambda;
    double* H;             // [T][P][6] with JAC
    double* g;             // [T][P][3] with JAC: g̃ with x32, else the solve's right-hand side
    double* c2;            // [T][P][2] or null
    uint8_t* nviews;       // [T][P] or null
};

template <bool JAC>
__global__ __launch_bounds__(kBlock) void fit_terms_kernel(FitTerms a) {
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
    // second-difference rows t, t+1, t+2 (row s exists for 2 <= s <= T-1)
    double d[3][3];
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const bool row = t + q >= 2 && t + q <= T - 1 && (JAC || q == 0);
#pragma unroll
        for (int k = 0; k < 3; k++) d[q][k] = row ? Xw[q + 2][k] - 2.0 * Xw[q + 1][k] + Xw[q][k] : 0.0;
    }
    if (a.c2) {
        a.c2[2 * e + 0] = f.front ? f.rho : (double)INFINITY;
        a.c2[2 * e + 1] = 0.5 * a.lambda * (d[0][0] * d[0][0] + d[0][1] * d[0][1] + d[0][2] * d[0][2]);
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

// mvp_trajectory_fit_system's costs: one workgroup per chain, each lane its frames in ascending
// order, then a tree over the lanes in a fixed order.
__global__ __launch_bounds__(kBlock) void fit_system_cost_kernel(FitObs o, const float* __restrict__ x32,
                                                                 double* __restrict__ out_cost) {
#pragma clang fp contract(fast)
    __shared__ double scam[kMaxCams][MVP_CAM_DOUBLES];
    __shared__ CamFast sfast[kMaxCams];
    __shared__ double s_red[2][kBlock];
    load_cams(scam, sfast, o.cams, o.n_cams);
    const int p = blockIdx.x;
    double rho = 0.0, sm = 0.0;
    for (int t = threadIdx.x; t < o.T; t += kBlock) {
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
    }
    s_red[0][threadIdx.x] = rho;
    s_red[1][threadIdx.x] = sm;
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            s_red[0][threadIdx.x] += s_red[0][threadIdx.x + s];
            s_red[1][threadIdx.x] += s_red[1][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out_cost[2 * p + 0] = s_red[0][0];
        out_cost[2 * p + 1] = s_red[1][0];
    }
}

// ------------------------------------------------------------------------------- sum, decide
// part[tile][p][2] = the two numbers of c2 over the tile's frames of chain p.
__global__ __launch_bounds__(kFitRows * 64) void fit_sum_kernel(const double* __restrict__ c2, int T, int P,
                                                                const int* __restrict__ done,
                                                                double* __restrict__ part) {
    __shared__ double s_red[2][kFitRows][64];
    const int px = threadIdx.x & 63, row = threadIdx.x >> 6;
    const int p_tiles = (P + 63) / 64;   // tiles of chains and of frames share grid.x: no limit of grid.y on P
    const int tile = blockIdx.x / p_tiles;
    const int p = (blockIdx.x - tile * p_tiles) * 64 + px;
    const int t0 = tile * kFitTile;
    const int t1 = t0 + kFitTile < T ? t0 + kFitTile : T;
    const bool live = p < P && !(done && done[p]);
    double s0 = 0.0, s1 = 0.0;
    if (live) {
#pragma unroll 4
        for (int t = t0 + row; t < t1; t += kFitRows) {
            const int64_t e = (int64_t)t * P + p;
            s0 += c2[2 * e + 0];
            s1 += c2[2 * e + 1];
        }
    }
    s_red[0][row][px] = s0;
    s_red[1][row][px] = s1;
    __syncthreads();
    if (row == 0 && live) {
#pragma unroll
        for (int r = 1; r < kFitRows; r++) {
            s0 += s_red[0][r][px];
            s1 += s_red[1][r][px];
        }
        part[2 * ((int64_t)tile * P + p) + 0] = s0;
        part[2 * ((int64_t)tile * P + p) + 1] = s1;
    }
}

// mode 0: validity from prepare's sums; mode 1: the seed's cost; mode 2: the trial's.
__global__ __launch_bounds__(kSmBlock) void fit_decide_kernel(FitChain ch, const double* __restrict__ part, int n_tiles,
                                                              int P, int mode, int max_iter, double tol,
                                                              int* __restrict__ bad) {
    const int p = blockIdx.x * kSmBlock + threadIdx.x;
    if (p >= P) return;
    if (mode != 0 && ch.done[p]) return;
    double s0 = 0.0, s1 = 0.0;
#pragma unroll 8   // eight loads in flight; the additions stay in index order
    for (int w = 0; w < n_tiles; w++) {
        s0 += part[2 * ((int64_t)w * P + p) + 0];
        s1 += part[2 * ((int64_t)w * P + p) + 1];
    }
    bad[p] = 0;
    if (mode == 0) {
        const bool valid = s0 >= 2.0 && s1 == 0.0;
        ch.mu[p] = 1e-3;
        ch.f[p] = ch.fseed[p] = __builtin_nan("");
        ch.cur[p] = 0;
        ch.done[p] = valid ? 0 : 1;
        ch.status[p] = valid ? 0x40 : 0x80;
        ch.relin[p] = 1;
        ch.rej[p] = 0;
        return;
    }
    const double ft = s0 + s1;
    if (mode == 1) {
        const bool fin = isfinite(ft);   // a seed whose cost overflows is no seed
        ch.f[p] = ch.fseed[p] = fin ? ft : __builtin_nan("");
        ch.done[p] = (fin && max_iter > 0) ? 0 : 1;
        ch.status[p] = fin ? 0x40 : 0x80;
        ch.relin[p] = 0;   // the seed has just been linearised
        return;
    }
    const double f = ch.f[p];
    const int trials = (ch.status[p] & 63) + 1;
    const bool accept = !ch.rej[p] && isfinite(ft) && ft <= f;
    bool done = false, conv = false;
    double mu = ch.mu[p];
    if (accept) {
        conv = (f - ft) <= tol * f;
        ch.cur[p] ^= 1;
        ch.f[p] = ft;
        mu = fmax(mu * 0.1, 1e-12);
        done = conv;
    } else {
        mu = mu * 10.0;
        done = mu > 1e12;
    }
    done = done || trials >= max_iter;
    ch.mu[p] = mu;
    ch.relin[p] = accept ? 1 : 0;
    ch.status[p] = trials | (conv ? 0 : 0x40);
    ch.done[p] = done ? 1 : 0;
}

__global__ __launch_bounds__(kSmBlock) void fit_eliminate_kernel(FitSolveArgs a) {
    const int64_t lane = (int64_t)blockIdx.x * kSmBlock + threadIdx.x;
    if (lane < a.n_lanes) eliminate_lane(a, lane);
}

__global__ __launch_bounds__(kSmBlock) void fit_reduce_kernel(FitSolveArgs a) {
    const int p = blockIdx.x * kSmBlock + threadIdx.x;
    if (p < a.P) reduce_chain(a, p);
}

__global__ __launch_bounds__(kSmBlock) void fit_backsub_kernel(FitSolveArgs a) {
    const int64_t lane = (int64_t)blockIdx.x * kSmBlock + threadIdx.x;
    if (lane < a.n_lanes) backsub_lane(a, lane);
}

// mvp_trajectory_fit_cov: the solver's sweeps over the undamped linearisation at a given state,
// then the covariance sweep of smooth_solver.h where the fit has its backsub.
__global__ __launch_bounds__(kSmBlock) void fit_cov_eliminate_kernel(FitCovArgs a) {
    const int64_t lane = (int64_t)blockIdx.x * kSmBlock + threadIdx.x;
    if (lane < a.n_lanes) eliminate_lane(a, lane);
}

__global__ __launch_bounds__(kSmBlock) void fit_cov_reduce_kernel(FitCovArgs a) {
    const int p = blockIdx.x * kSmBlock + threadIdx.x;
    if (p < a.P) {
        reduce_chain(a, p);
        reduce_cov_chain(a, p);
    }
}

__global__ __launch_bounds__(kSmBlock) void fit_cov_kernel(FitCovArgs a) {
    const int64_t lane = (int64_t)blockIdx.x * kSmBlock + threadIdx.x;
    if (lane < a.n_lanes) cov_lane(a, lane);
}

// ------------------------------------------------------------------------------- output
__global__ __launch_bounds__(kBlock) void fit_output_kernel(FitObs o, const float* __restrict__ xyz0,
                                                            const double* __restrict__ x64, FitChain ch,
                                                            float* __restrict__ out_xyz, float* __restrict__ out_resid,
                                                            uint8_t* __restrict__ out_nviews,
                                                            double* __restrict__ out_cost,
                                                            uint8_t* __restrict__ out_status) {
#pragma clang fp contract(fast)
    __shared__ double scam[kMaxCams][MVP_CAM_DOUBLES];
    __shared__ CamFast sfast[kMaxCams];
    load_cams(scam, sfast, o.cams, o.n_cams);
    const int64_t n = (int64_t)o.T * o.P;
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= n) return;
    const int t = (int)(e / o.P), p = (int)(e - (int64_t)t * o.P);
    const int status = ch.status[p];
    const bool valid = status != 0x80;
    const double* xp = x64 + 3 * ((int64_t)ch.cur[p] * n + e);
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
    if (t == 0) {
        if (out_cost) {
            out_cost[2 * p + 0] = ch.fseed[p];
            out_cost[2 * p + 1] = ch.f[p];
        }
        if (out_status) out_status[p] = (uint8_t)status;
    }
}

}  // namespace

// ------------------------------------------------------------------------------- host side

extern "C" int mvp_trajectory_fit_plan(int T, int P, int chunk, int* chunk_used, int* n_chunks,
                                       int64_t* workspace_bytes) {
    MVP_ABI_BEGIN
    const FitPlan pl = fit_plan("mvp_trajectory_fit_plan", T, P, chunk);
    if (chunk_used) *chunk_used = pl.sp.chunk;
    if (n_chunks) *n_chunks = pl.sp.n_chunks;
    if (workspace_bytes) *workspace_bytes = pl.bytes;
    MVP_ABI_END
}

extern "C" int mvp_trajectory_fit_system(const float* kpts, int T, int P, int V, const double* cams, int n_cams,
                                         const int* cam_idx, int n_cam_idx, const float* xyz, const uint8_t* mask,
                                         int weights, const double* gauss, float min_conf, float cov_floor,
                                         double huber_delta, double* out_H, double* out_g, uint8_t* out_nviews,
                                         double* out_cost, void* stream) {
    MVP_ABI_BEGIN
    const char* fn = "mvp_trajectory_fit_system";
    const FitObs o = fit_parse(fn, kpts, T, P, V, cams, n_cams, cam_idx, n_cam_idx, mask, weights, gauss, min_conf,
                               cov_floor, huber_delta);
    MVP_REQUIRE(kpts && cams && xyz && out_H && out_g && out_nviews && out_cost, "%s: null device pointer", fn);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    FitTerms a{};
    a.o = o;
    a.x32 = xyz;
    a.lambda = 1.0;
    a.H = out_H;
    a.g = out_g;
    a.nviews = out_nviews;
    hipLaunchKernelGGL(fit_terms_kernel<true>, dim3(tri_grid(fn, (int64_t)T * P)), dim3(kBlock), 0, s, a);
    MVP_HIP(hipGetLastError());
    hipLaunchKernelGGL(fit_system_cost_kernel, dim3((unsigned)P), dim3(kBlock), 0, s, o, xyz, out_cost);
    MVP_HIP(hipGetLastError());
    MVP_ABI_END
}

extern "C" int mvp_trajectory_fit_cov_plan(int T, int P, int chunk, int* chunk_used, int* n_chunks,
                                           int64_t* workspace_bytes) {
    MVP_ABI_BEGIN
    const FitPlan pl = fit_plan("mvp_trajectory_fit_cov_plan", T, P, chunk);
    const CovPlan cp = cov_plan(pl.sp, P, pl.bytes);
    if (chunk_used) *chunk_used = pl.sp.chunk;
    if (n_chunks) *n_chunks = pl.sp.n_chunks;
    if (workspace_bytes) *workspace_bytes = cp.bytes;
    MVP_ABI_END
}

// prepare, sum, decide(0): the fit's validity pass at xyz; terms<JAC> at xyz: H̃; then eliminate
// (no Marquardt factor, pivots kept), reduce + its selected inverse, and the covariance sweep.
extern "C" int mvp_trajectory_fit_cov(const float* kpts, int T, int P, int V, const double* cams, int n_cams,
                                      const int* cam_idx, int n_cam_idx, const float* xyz, const uint8_t* mask,
                                      int weights, const double* gauss, float min_conf, float cov_floor,
                                      double huber_delta, double lambda_smooth, int chunk, void* workspace,
                                      int64_t workspace_bytes, float* out_cov, float* out_cross, uint8_t* out_status,
                                      void* stream) {
    MVP_ABI_BEGIN
    const char* fn = "mvp_trajectory_fit_cov";
    const FitObs o = fit_parse(fn, kpts, T, P, V, cams, n_cams, cam_idx, n_cam_idx, mask, weights, gauss, min_conf,
                               cov_floor, huber_delta);
    const FitPlan pl = fit_plan(fn, T, P, chunk);
    const CovPlan cp = cov_plan(pl.sp, P, pl.bytes);
    MVP_REQUIRE(std::isfinite(lambda_smooth) && lambda_smooth > 0, "%s: lambda_smooth=%g must be finite and > 0", fn,
                lambda_smooth);
    MVP_REQUIRE(workspace_bytes >= cp.bytes, "%s: workspace_bytes=%lld < %lld needed (T=%d, P=%d, chunk=%d)", fn,
                (long long)workspace_bytes, (long long)cp.bytes, T, P, pl.sp.chunk);
    MVP_REQUIRE(kpts && cams && xyz && workspace && out_cov, "%s: null device pointer", fn);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
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
    double* x64 = reinterpret_cast<double*>(ws + pl.off_x);
    double* c2 = reinterpret_cast<double*>(ws + pl.off_c2);
    double* part = reinterpret_cast<double*>(ws + pl.off_part);
    FitCovArgs a{};
    a.T = T, a.P = P, a.chunk = pl.sp.chunk, a.n_chunks = pl.sp.n_chunks, a.n_seps = pl.sp.n_seps;
    a.n_lanes = pl.sp.n_lanes, a.n_blocks = pl.sp.n_blocks;
    a.lambda = lambda_smooth;
    a.fac = reinterpret_cast<double*>(ws + pl.sp.off_fac);
    a.schur = reinterpret_cast<double*>(ws + pl.sp.off_schur);
    a.red = reinterpret_cast<double*>(ws + pl.sp.off_red);
    a.usol = reinterpret_cast<double*>(ws + pl.sp.off_usol);
    a.cnt = reinterpret_cast<int*>(ws + pl.sp.off_cnt);
    a.bad = reinterpret_cast<int*>(ws + pl.sp.off_bad);
    a.fail = reinterpret_cast<int*>(ws + pl.sp.off_fail);
    a.piv = reinterpret_cast<double*>(ws + cp.off_piv);
    a.covred = reinterpret_cast<double*>(ws + cp.off_covred);
    a.H = reinterpret_cast<double*>(ws + pl.off_H);
    a.g = reinterpret_cast<double*>(ws + pl.off_g);
    a.invalid = ch.done;
    a.out_cov = out_cov;
    a.out_cross = out_cross;
    a.out_status = out_status;
    FitTerms ta{};
    ta.o = o;
    ta.x32 = xyz;   // the given state itself: no chain flag is read
    ta.lambda = lambda_smooth;
    ta.H = reinterpret_cast<double*>(ws + pl.off_H);
    ta.g = reinterpret_cast<double*>(ws + pl.off_g);
    const dim3 flat(tri_grid(fn, (int64_t)T * P)), blk(kBlock);
    const dim3 chain_grid((unsigned)((P + kSmBlock - 1) / kSmBlock)), lane_grid((unsigned)pl.sp.n_blocks), sm_blk(kSmBlock);
    MVP_HIP(hipMemsetAsync(a.cnt, 0, (size_t)P * 8, s));
    hipLaunchKernelGGL(fit_prepare_kernel, flat, blk, 0, s, o, xyz, x64, c2);
    MVP_HIP(hipGetLastError());
    hipLaunchKernelGGL(fit_sum_kernel, dim3((unsigned)pl.sum_blocks), dim3(kFitRows * 64), 0, s, c2, T, P,
                       (const int*)nullptr, part);
    hipLaunchKernelGGL(fit_decide_kernel, chain_grid, sm_blk, 0, s, ch, part, pl.n_tiles, P, 0, 0, 1.0, a.bad);
    MVP_HIP(hipGetLastError());
    hipLaunchKernelGGL(fit_terms_kernel<true>, flat, blk, 0, s, ta);
    MVP_HIP(hipGetLastError());
    hipLaunchKernelGGL(fit_cov_eliminate_kernel, lane_grid, sm_blk, 0, s, a);
    hipLaunchKernelGGL(fit_cov_reduce_kernel, chain_grid, sm_blk, 0, s, a);
    hipLaunchKernelGGL(fit_cov_kernel, lane_grid, sm_blk, 0, s, a);
    MVP_HIP(hipGetLastError());
    MVP_ABI_END
}

extern "C" int mvp_trajectory_fit(const float* kpts, int T, int P, int V, const double* cams, int n_cams,
                                  const int* cam_idx, int n_cam_idx, const float* xyz0, const uint8_t* mask,
                                  int weights, const double* gauss, float min_conf, float cov_floor,
                                  double huber_delta, double lambda_smooth, int max_iter, double tol, int chunk,
                                  void* workspace, int64_t workspace_bytes, float* out_xyz, float* out_resid,
                                  uint8_t* out_nviews, double* out_cost, uint8_t* out_status, void* stream) {
    MVP_ABI_BEGIN
    const char* fn = "mvp_trajectory_fit";
    const FitObs o = fit_parse(fn, kpts, T, P, V, cams, n_cams, cam_idx, n_cam_idx, mask, weights, gauss, min_conf,
                               cov_floor, huber_delta);
    const FitPlan pl = fit_plan(fn, T, P, chunk);
    MVP_REQUIRE(std::isfinite(lambda_smooth) && lambda_smooth > 0, "%s: lambda_smooth=%g must be finite and > 0", fn,
                lambda_smooth);
    MVP_REQUIRE(max_iter >= 0 && max_iter <= 63, "%s: max_iter=%d (0..63)", fn, max_iter);
    MVP_REQUIRE(std::isfinite(tol) && tol > 0, "%s: tol=%g (finite, > 0)", fn, tol);
    MVP_REQUIRE(workspace_bytes >= pl.bytes, "%s: workspace_bytes=%lld < %lld needed (T=%d, P=%d, chunk=%d)", fn,
                (long long)workspace_bytes, (long long)pl.bytes, T, P, pl.sp.chunk);
    MVP_REQUIRE(kpts && cams && xyz0 && workspace && out_xyz, "%s: null device pointer", fn);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    const int64_t n = (int64_t)T * P;
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
    double* x64 = reinterpret_cast<double*>(ws + pl.off_x);
    double* c2 = reinterpret_cast<double*>(ws + pl.off_c2);
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
    FitTerms ta{};
    ta.o = o;
    ta.x64 = x64;
    ta.ch = ch;
    ta.lambda = lambda_smooth;
    ta.H = reinterpret_cast<double*>(ws + pl.off_H);
    ta.g = reinterpret_cast<double*>(ws + pl.off_g);
    ta.c2 = c2;
    const dim3 flat(tri_grid(fn, n)), blk(kBlock);
    const dim3 sum_grid((unsigned)pl.sum_blocks), sum_blk(kFitRows * 64);
    const dim3 chain_grid((unsigned)((P + kSmBlock - 1) / kSmBlock)), lane_grid((unsigned)pl.sp.n_blocks), sm_blk(kSmBlock);
    auto sum_decide = [&](int mode) {
        hipLaunchKernelGGL(fit_sum_kernel, sum_grid, sum_blk, 0, s, c2, T, P, mode == 0 ? (const int*)nullptr : ch.done,
                           part);
        hipLaunchKernelGGL(fit_decide_kernel, chain_grid, sm_blk, 0, s, ch, part, pl.n_tiles, P, mode, max_iter, tol,
                           sa.bad);
        MVP_HIP(hipGetLastError());
    };
    MVP_HIP(hipMemsetAsync(sa.cnt, 0, (size_t)P * 8, s));
    hipLaunchKernelGGL(fit_prepare_kernel, flat, blk, 0, s, o, xyz0, x64, c2);
    MVP_HIP(hipGetLastError());
    sum_decide(0);
    ta.trial = 0;
    hipLaunchKernelGGL(fit_terms_kernel<true>, flat, blk, 0, s, ta);
    sum_decide(1);
    for (int it = 0; it < max_iter; it++) {
        hipLaunchKernelGGL(fit_eliminate_kernel, lane_grid, sm_blk, 0, s, sa);
        hipLaunchKernelGGL(fit_reduce_kernel, chain_grid, sm_blk, 0, s, sa);
        hipLaunchKernelGGL(fit_backsub_kernel, lane_grid, sm_blk, 0, s, sa);
        ta.trial = 1;
        hipLaunchKernelGGL(fit_terms_kernel<false>, flat, blk, 0, s, ta);
        sum_decide(2);
        if (it + 1 < max_iter) {
            ta.trial = 0;
            hipLaunchKernelGGL(fit_terms_kernel<true>, flat, blk, 0, s, ta);
            MVP_HIP(hipGetLastError());
        }
    }
    hipLaunchKernelGGL(fit_output_kernel, flat, blk, 0, s, o, xyz0, x64, ch, out_xyz, out_resid, out_nviews, out_cost,
                       out_status);
    MVP_HIP(hipGetLastError());
    MVP_ABI_END
}
