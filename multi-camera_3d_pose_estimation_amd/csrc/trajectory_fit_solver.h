// The trajectory fit's side of the partition solver (smooth_solver.h): the per-chain state, the
// frame source that reads the information-form buffer and writes the trial state, and the
// workspace plan of the trajectory fit and the skeleton fit with the carving of its chain block.
// Apart from trajectory_fit_kernels.h, so that a host program can run the sweeps lane by lane
// (tools/solver_host_check.cpp, tools/cov_host_check.cpp) without compiling the fit's kernels.
#pragma once
#include "smooth_solver.h"

namespace {

constexpr int kFitTile = 256;   // frames per workgroup of the sum kernel
constexpr int kFitRows = 4;     // its rows of 64 lanes (lanes along p)

// The per-chain state of a fit, all [P].
struct FitChain {
    double* mu;
    double* f;        // the state's cost
    double* fseed;
    int* cur;         // which of the two buffers of x64 holds the state
    int* done;
    int* status;      // the status byte
    int* relin;       // the state moved: linearise again
    int* rej;         // a pivot of the last solve was not > 0
};

// The solver's frames.
struct FitRaw {
    double h[6], b[3];
};
struct FitX {
    double x[3];
};

struct FitSolveArgs : SolveCore {
    const double* H;    // [T][P][6]
    const double* g;    // [T][P][3], the right-hand side
    double* x64;        // [2][T][P][3]
    FitChain ch;
    using Raw = FitRaw;
    using Out = FitX;
    static constexpr bool kInfoForm = true;
    MVP_SMOOTH_HD double damp(int p) const { return 1.0 + ch.mu[p]; }
    MVP_SMOOTH_HD bool skip(int p) const { return ch.done[p] != 0; }
    MVP_SMOOTH_HD FitRaw load_raw(int t, int p) const {
        const int64_t e = (int64_t)t * P + p;
        FitRaw f;
#pragma unroll
        for (int k = 0; k < 6; k++) f.h[k] = H[6 * e + k];
#pragma unroll
        for (int k = 0; k < 3; k++) f.b[k] = g[3 * e + k];
        return f;
    }
    // every frame has a block, if a zero one: nothing is counted
    MVP_SMOOTH_HD bool frame_weight(const FitRaw& f, double (&W)[6], double (&z)[3]) const {
#pragma unroll
        for (int k = 0; k < 6; k++) W[k] = f.h[k];
#pragma unroll
        for (int k = 0; k < 3; k++) z[k] = f.b[k];
        return false;
    }
    MVP_SMOOTH_HD void finish(int p, int, int bad_pivot) const { ch.rej[p] = bad_pivot; }
    MVP_SMOOTH_HD bool failed(int) const { return false; }
    MVP_SMOOTH_HD void write_failed(int, int) const {}
    MVP_SMOOTH_HD FitX load_out(int t, int p) const {
        const int64_t e = (int64_t)ch.cur[p] * T * P + (int64_t)t * P + p;
        FitX f;
#pragma unroll
        for (int k = 0; k < 3; k++) f.x[k] = x64[3 * e + k];
        return f;
    }
    // the trial state X + δ, into the chain's other buffer
    MVP_SMOOTH_HD void write_frame(int t, int p, const FitX& f, double d0, double d1, double d2) const {
        const int64_t e = (int64_t)(ch.cur[p] ^ 1) * T * P + (int64_t)t * P + p;
        x64[3 * e + 0] = f.x[0] + d0;
        x64[3 * e + 1] = f.x[1] + d1;
        x64[3 * e + 2] = f.x[2] + d2;
    }
};

// The frames of mvp_trajectory_fit_lag: the same buffers, and the data block between frames t and
// t+1 in Cx [T][P][6] (row T-1 zero).  A frame's record carries the block that ends in it.
struct FitLagRaw {
    double h[6], b[3], c[6];
};

struct FitLagSolveArgs : FitSolveArgs {
    const double* Cx;   // [T][P][6]
    using Raw = FitLagRaw;
    static constexpr bool kHasCross = true;
    MVP_SMOOTH_HD FitLagRaw load_raw(int t, int p) const {
        const int64_t e = (int64_t)t * P + p;
        FitLagRaw f;
#pragma unroll
        for (int k = 0; k < 6; k++) f.h[k] = H[6 * e + k];
#pragma unroll
        for (int k = 0; k < 3; k++) f.b[k] = g[3 * e + k];
#pragma unroll
        for (int k = 0; k < 6; k++) f.c[k] = t > 0 ? Cx[6 * (e - P) + k] : 0.0;
        return f;
    }
    MVP_SMOOTH_HD bool frame_weight(const FitLagRaw& f, double (&W)[6], double (&z)[3]) const {
#pragma unroll
        for (int k = 0; k < 6; k++) W[k] = f.h[k];
#pragma unroll
        for (int k = 0; k < 3; k++) z[k] = f.b[k];
        return false;
    }
    MVP_SMOOTH_HD void cross(const FitLagRaw& f, double (&C)[6]) const {
#pragma unroll
        for (int k = 0; k < 6; k++) C[k] = f.c[k];
    }
};

// The frames of mvp_trajectory_fit_cov: the same information-form buffer at a given state, no
// Marquardt factor, the inverse pivots kept; reduce_cov_chain and cov_lane then give Σ = A⁻¹.
struct FitCovArgs : SolveCore, CovCore {
    const double* H;     // [T][P][6]
    const double* g;     // [T][P][3] (the eliminate sweep carries a right-hand side; nothing reads its result)
    const int* invalid;  // [P] the validity pass's verdict
    int* fail;           // [P]
    uint8_t* out_status; // [P] or null
    using Raw = FitRaw;
    static constexpr bool kInfoForm = true;
    static constexpr bool kKeepPivot = true;
    MVP_SMOOTH_HD NoDamp damp(int) const { return NoDamp{}; }
    MVP_SMOOTH_HD bool skip(int) const { return false; }
    MVP_SMOOTH_HD FitRaw load_raw(int t, int p) const {
        const int64_t e = (int64_t)t * P + p;
        FitRaw f;
#pragma unroll
        for (int k = 0; k < 6; k++) f.h[k] = H[6 * e + k];
#pragma unroll
        for (int k = 0; k < 3; k++) f.b[k] = g[3 * e + k];
        return f;
    }
    MVP_SMOOTH_HD bool frame_weight(const FitRaw& f, double (&W)[6], double (&z)[3]) const {
#pragma unroll
        for (int k = 0; k < 6; k++) W[k] = f.h[k];
#pragma unroll
        for (int k = 0; k < 3; k++) z[k] = f.b[k];
        return false;
    }
    MVP_SMOOTH_HD void finish(int p, int, int bad_pivot) const {
        const int failed = (invalid[p] || bad_pivot) ? 1 : 0;
        fail[p] = failed;
        if (out_status) out_status[p] = failed ? 0x80 : 0;
    }
    MVP_SMOOTH_HD bool failed(int p) const { return fail[p] != 0; }
};

// The workspace of a fit behind its solver's: the chains' state, the groups' where chains decide
// together (G of them; the skeleton fit), the two state buffers, the linearisation, the frames'
// n_costs cost terms and their sums per tile.
struct FitPlan {
    SmoothPlan sp;
    int n_tiles;
    int64_t sum_blocks;   // the sum kernel's workgroups: frame tiles x tiles of 64 chains
    int64_t off_chain, off_group, off_x, off_H, off_g, off_cost, off_part, bytes;
};

constexpr int64_t kFitGroupBytes = 5 * 8 + 2 * 4;   // per group: 5 doubles, 2 ints (skeleton_fit.hip's SkGroup)

inline FitPlan fit_plan(const char* fn, int T, int P, int chunk, int n_costs = 2, int G = 0) {
    FitPlan pl;
    pl.sp = smooth_plan(fn, T, P, chunk);
    MVP_REQUIRE((int64_t)T * P < (1LL << 31), "%s: T·P=%lld must be < 2^31", fn, (long long)T * P);
    const int64_t n = (int64_t)T * P;
    pl.n_tiles = (T + kFitTile - 1) / kFitTile;
    pl.sum_blocks = (int64_t)pl.n_tiles * ((P + 63) / 64);
    MVP_REQUIRE(pl.sum_blocks < (1LL << 31), "%s: too many tiles (T=%d, P=%d)", fn, T, P);
    int64_t b = pl.sp.bytes;
    pl.off_chain = b;
    b = align256(b + (int64_t)P * (3 * 8 + 5 * 4));
    pl.off_group = b;
    b = align256(b + G * kFitGroupBytes);
    pl.off_x = b;
    b = align256(b + 2 * n * 3 * 8);
    pl.off_H = b;
    b = align256(b + n * 6 * 8);
    pl.off_g = b;
    b = align256(b + n * 3 * 8);
    pl.off_cost = b;
    b = align256(b + n * n_costs * 8);
    pl.off_part = b;
    b = align256(b + (int64_t)pl.n_tiles * P * n_costs * 8);
    pl.bytes = b;
    return pl;
}

// What mvp_trajectory_fit_lag adds behind the fit's workspace: the blocks between neighbouring
// frames and the tiles' sums of the offset derivative, [tile][P][kLagViews][2].
constexpr int kLagViews = 8;   // the most views a call lists (tri_common.h's kMaxCams)

struct LagPlan {
    int64_t off_C, off_dpart, bytes;
};

inline LagPlan lag_plan(const FitPlan& pl, int T, int P) {
    LagPlan lp;
    int64_t b = pl.bytes;
    lp.off_C = b;
    b = align256(b + (int64_t)T * P * 6 * 8);
    lp.off_dpart = b;
    b = align256(b + (int64_t)pl.n_tiles * P * kLagViews * 2 * 8);
    lp.bytes = b;
    return lp;
}

// The chains' state in the plan's chain block c.
inline FitChain bind_chain(char* c, int P) {
    FitChain ch;
    ch.mu = reinterpret_cast<double*>(c);
    ch.f = ch.mu + P;
    ch.fseed = ch.f + P;
    ch.cur = reinterpret_cast<int*>(ch.fseed + P);
    ch.done = ch.cur + P;
    ch.status = ch.done + P;
    ch.relin = ch.status + P;
    ch.rej = ch.relin + P;
    return ch;
}

}  // namespace
