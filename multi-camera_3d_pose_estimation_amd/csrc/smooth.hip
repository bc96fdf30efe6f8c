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
//
// The three sweeps' per-lane code, their kernels (solve_eliminate_kernel<A>, solve_reduce_kernel<A>,
// solve_backsub_kernel<A>) and the plan are in smooth_solver.h, templated on the frame source A (the
// trajectory fit runs them over an information-form buffer); here: the smoother's sources,
// (xyz, cov, valid) -> (W, z) and the outputs, and the C entry points.
//
// mvp_trajectory_smooth_cov runs the same eliminate and reduce over the same frames with the
// inverse pivots kept, the reduced system's selected inverse behind the reduce, and the covariance
// sweep (smooth_solver.h: reduce_cov_chain, cov_lane) where the smoother has its
// backsub: the diagonal and lag-1 blocks of the inverse of the smoother's matrix.
#include "smooth_solver.h"

namespace {

// The smoother's frames: (xyz, cov, valid) in, xyz / resid / observed / status out, around the
// fields of SolveCore (by name: the kernels' argument block keeps the layout it always had).
struct SmoothSrc {
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

// The bytes of frame (t, p) as they lie in memory: loaded one sweep step ahead of their use, so
// that the step does not wait for them.
struct RawFrame {
    float x[3], c[6];
    uint8_t v;
};

MVP_SMOOTH_HD RawFrame load_raw(const SmoothSrc& a, int t, int p) {
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
MVP_SMOOTH_HD bool frame_weight(const SmoothSrc& a, const RawFrame& f, double (&W)[6], double (&z)[3]) {
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

// A failed chain's frame: the input bits, NaN resid.
MVP_SMOOTH_HD void write_failed(const SmoothSrc& a, int t, int p) {
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

MVP_SMOOTH_HD void write_frame(const SmoothSrc& a, int t, int p, const RawFrame& f, double x0, double x1, double x2) {
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

// The frame source of smooth_solver.h over those functions.
struct SmoothArgs : SmoothSrc {
    using Raw = RawFrame;
    using Out = RawFrame;
    static constexpr bool kInfoForm = false;
    MVP_SMOOTH_HD NoDamp damp(int) const { return NoDamp{}; }
    MVP_SMOOTH_HD bool skip(int) const { return false; }
    MVP_SMOOTH_HD RawFrame load_raw(int t, int p) const { return ::load_raw(*this, t, p); }
    MVP_SMOOTH_HD RawFrame load_out(int t, int p) const { return ::load_raw(*this, t, p); }
    MVP_SMOOTH_HD bool frame_weight(const RawFrame& f, double (&W)[6], double (&z)[3]) const {
        return ::frame_weight(*this, f, W, z);
    }
    MVP_SMOOTH_HD void finish(int p, int cnt, int bad) const {
        const int failed = (cnt < 2 || bad) ? 1 : 0;
        fail[p] = failed;
        if (out_status) out_status[p] = failed ? 0x80 : 0;
    }
    MVP_SMOOTH_HD bool failed(int p) const { return fail[p] != 0; }
    MVP_SMOOTH_HD void write_failed(int t, int p) const { ::write_failed(*this, t, p); }
    MVP_SMOOTH_HD void write_frame(int t, int p, const RawFrame& f, double x0, double x1, double x2) const {
        ::write_frame(*this, t, p, f, x0, x1, x2);
    }
};

// The source of mvp_trajectory_smooth_cov: the same frames and weights, the inverse pivots kept,
// and the covariance outputs where the smoother has its own (which stay null: no backsub runs).
struct SmoothCovArgs : SmoothSrc, CovCore {
    using Raw = RawFrame;
    static constexpr bool kInfoForm = false;
    static constexpr bool kKeepPivot = true;
    MVP_SMOOTH_HD NoDamp damp(int) const { return NoDamp{}; }
    MVP_SMOOTH_HD bool skip(int) const { return false; }
    MVP_SMOOTH_HD RawFrame load_raw(int t, int p) const { return ::load_raw(*this, t, p); }
    MVP_SMOOTH_HD bool frame_weight(const RawFrame& f, double (&W)[6], double (&z)[3]) const {
        return ::frame_weight(*this, f, W, z);
    }
    MVP_SMOOTH_HD void finish(int p, int cnt, int bad) const {
        const int failed = (cnt < 2 || bad) ? 1 : 0;
        fail[p] = failed;
        if (out_status) out_status[p] = failed ? 0x80 : 0;
    }
    MVP_SMOOTH_HD bool failed(int p) const { return fail[p] != 0; }
};

// The three launches of smooth_solver.h over a bound source, the counts the eliminate lanes add up
// zeroed first.
template <class A>
void launch_solve(const A& a, hipStream_t s) {
    const dim3 lane_grid((unsigned)a.n_blocks), chain_grid((unsigned)((a.P + kSmBlock - 1) / kSmBlock)), blk(kSmBlock);
    MVP_HIP(hipMemsetAsync(a.cnt, 0, (size_t)a.P * 8, s));
    hipLaunchKernelGGL(solve_eliminate_kernel<A>, lane_grid, blk, 0, s, a);
    MVP_HIP(hipGetLastError());
    hipLaunchKernelGGL(solve_reduce_kernel<A>, chain_grid, blk, 0, s, a);
    MVP_HIP(hipGetLastError());
    hipLaunchKernelGGL(solve_backsub_kernel<A>, lane_grid, blk, 0, s, a);
    MVP_HIP(hipGetLastError());
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
    bind_core(a, ws, pl, T, P, lambda_smooth);
    a.w0 = 1.0 / ((double)sigma0 * (double)sigma0);
    a.cov_floor = (double)cov_floor;
    a.out_xyz = out_xyz;
    a.out_resid = out_resid;
    a.out_observed = out_observed;
    a.out_status = out_status;
    launch_solve(a, (hipStream_t)stream);
    MVP_ABI_END
}

// The posterior covariance of the same model: eliminate (pivots kept), reduce + the reduced
// system's selected inverse, then the covariance sweep where the smoother has its backsub.
extern "C" int mvp_trajectory_smooth_cov_plan(int T, int P, int chunk, int* chunk_used, int* n_chunks,
                                              int64_t* workspace_bytes) {
    MVP_ABI_BEGIN
    const SmoothPlan pl = smooth_plan("mvp_trajectory_smooth_cov_plan", T, P, chunk);
    const CovPlan cp = cov_plan(pl, P, pl.bytes);
    if (chunk_used) *chunk_used = pl.chunk;
    if (n_chunks) *n_chunks = pl.n_chunks;
    if (workspace_bytes) *workspace_bytes = cp.bytes;
    MVP_ABI_END
}

extern "C" int mvp_trajectory_smooth_cov(const float* xyz, const float* cov, const uint8_t* valid, int T, int P,
                                         double lambda_smooth, float sigma0, float cov_floor, int chunk, void* workspace,
                                         int64_t workspace_bytes, float* out_cov, float* out_cross, uint8_t* out_status,
                                         void* stream) {
    MVP_ABI_BEGIN
    const char* fn = "mvp_trajectory_smooth_cov";
    const SmoothPlan pl = smooth_plan(fn, T, P, chunk);
    const CovPlan cp = cov_plan(pl, P, pl.bytes);
    MVP_REQUIRE(std::isfinite(lambda_smooth) && lambda_smooth > 0, "%s: lambda_smooth=%g must be finite and > 0", fn,
                lambda_smooth);
    MVP_REQUIRE(std::isfinite(sigma0) && sigma0 > 0, "%s: sigma0=%g must be finite and > 0", fn, (double)sigma0);
    MVP_REQUIRE(cov_floor >= 0, "%s: cov_floor=%g must be >= 0", fn, (double)cov_floor);
    MVP_REQUIRE(workspace_bytes >= cp.bytes, "%s: workspace_bytes=%lld < %lld needed (T=%d, P=%d, chunk=%d)", fn,
                (long long)workspace_bytes, (long long)cp.bytes, T, P, pl.chunk);
    MVP_REQUIRE(xyz && out_cov && workspace, "%s: null device pointer", fn);
    char* ws = static_cast<char*>(workspace);
    SmoothCovArgs a{};
    a.xyz = xyz;
    a.cov = cov;
    a.valid = valid;
    bind_core(a, ws, pl, T, P, lambda_smooth);
    a.w0 = 1.0 / ((double)sigma0 * (double)sigma0);
    a.cov_floor = (double)cov_floor;
    a.out_status = out_status;
    bind_cov(a, ws, cp, out_cov, out_cross);
    launch_solve(a, (hipStream_t)stream);
    MVP_ABI_END
}
