// Left/right label swaps per camera (mvp_label_swap_*; the problem is stated in include/mvpose.h;
// no reference counterpart: the reference takes the detector's joint labels on trust) for gfx950.
//
// For every frame, listed view and unit of symmetric joint pairs the labels are either kept or
// exchanged; the cameras must agree with each other (epipolar tables) and each camera with its own
// previous frame (motion tables).  Stream-ordered launches, no atomics, arithmetic in fp64:
//
//   fundamental, undistort   sync_common.h, as for mvp_epipolar_lag_cost: F_ab of every pair of
//                listed views, and the f32 undistorted pixel of every keypoint (NaN = not usable)
//                into a workspace plane [view][frame·J + joint] of float2.
//   costs        one lane per (frame, unit).  Per view: the complete pairs, the motion sums keep /
//                change against the previous frame, the prior; per view pair: same / cross.  The
//                symmetric pairs of the unit are visited in ascending order, so every sum has one
//                order.  The products (motion_weight, swap_prior_px²) are done here.
//   solve        one wavefront per unit, frames in sequence.  State s = 64·r + lane: bits 0-5 of s
//                are the lane, bits 6-7 the register r (1, 2 or 4 registers of G and of flip per
//                lane).  A frame's five table rows are loaded one entry per lane, eight frames
//                ahead of their use, and handed out as wave-uniform values by v_readlane.  The pass of
//                view a exchanges G and flip with state s xor 2^a: a cross-lane permute for a < 6,
//                a register exchange for a >= 6; no LDS and no barrier in the recursion.  bp[t] is
//                written as 2^nv contiguous bytes.  With nv < 6 the lanes 2^nv and up repeat the
//                states of the first 2^nv lanes, so neither the loads nor the store sit behind a
//                branch and the wait for the next frame's rows leaves the store in flight.
//                The backtrack follows in the same launch: the
//                wave re-reads bp in chunks of at most 16 KiB into LDS and lane 0 walks a chunk
//                there, so the dependent chain runs at LDS latency and memory is read in bulk.
//                The solver only adds and compares (contraction is off): its bits are those of
//                any implementation that adds in the stated order.
//   apply        one lane per (frame, joint, row) of kpts, per (frame, column, joint) of the
//                optional [T][V][J][C] float64 array: a gather from the joint or its partner.
//
// Register / LDS figures and the measurements are in DESIGN.md §4.18.
#pragma clang fp contract(off)

#include "sync_common.h"

#include <cmath>

namespace {

constexpr int kLsWave = 64;
constexpr int kLsMaxPairs = 64;            // symmetric joint pairs
constexpr int kLsChunkBytes = 16 * 1024;   // of bp staged in LDS by the backtrack
constexpr int kLsChunkFrames = 256;        // at most; fewer when 2^nv > 64
constexpr int kLsAhead = 8;                // frames whose table rows the solver keeps in flight

struct LsPairs {
    int l[kLsMaxPairs], r[kLsMaxPairs];
    unsigned char unit[kLsMaxPairs];
    int ns;
};

inline int64_t ls_bp_stride(int T, int nv) { return sy_align256((int64_t)T << nv); }

struct LsPlan {
    int n_pairs;
    int64_t off_und, off_f, bytes;
};

// The checks shared by plan, costs and apply; fills `sp` when the lists are given.
inline void ls_check_shape(const char* fn, int T, int J, int nv, int NS, int U) {
    MVP_REQUIRE(T >= 1, "%s: T=%d < 1", fn, T);
    MVP_REQUIRE(J >= 2, "%s: J=%d < 2", fn, J);
    MVP_REQUIRE((int64_t)T * J < (1LL << 31), "%s: T*J=%lld too large", fn, (long long)T * J);
    MVP_REQUIRE(nv >= 2 && nv <= kMaxCams, "%s: n_cam_idx=%d (2..%d)", fn, nv, kMaxCams);
    MVP_REQUIRE(NS >= 1 && NS <= kLsMaxPairs && 2 * (int64_t)NS <= J, "%s: n_pairs=%d (1..%d, 2*n_pairs <= J=%d)", fn,
                NS, kLsMaxPairs, J);
    MVP_REQUIRE(U >= 1 && U <= NS, "%s: n_units=%d (1..n_pairs=%d)", fn, U, NS);
}

inline LsPairs ls_parse_pairs(const char* fn, int J, const int* pairs, int NS, const int* unit, int U) {
    MVP_REQUIRE(pairs && unit, "%s: pairs or unit is NULL", fn);
    LsPairs sp{};
    sp.ns = NS;
    bool used[kLsMaxPairs] = {};
    for (int k = 0; k < NS; k++) {
        const int l = pairs[2 * k], r = pairs[2 * k + 1];
        MVP_REQUIRE(l >= 0 && l < J && r >= 0 && r < J, "%s: pairs[%d]=(%d, %d) out of range (J=%d)", fn, k, l, r, J);
        MVP_REQUIRE(l != r, "%s: pairs[%d]=(%d, %d) names one joint twice", fn, k, l, r);
        for (int q = 0; q < k; q++)
            MVP_REQUIRE(l != sp.l[q] && l != sp.r[q] && r != sp.l[q] && r != sp.r[q],
                        "%s: pairs[%d]=(%d, %d) repeats a joint of pairs[%d]", fn, k, l, r, q);
        MVP_REQUIRE(unit[k] >= 0 && unit[k] < U, "%s: unit[%d]=%d out of range (n_units=%d)", fn, k, unit[k], U);
        sp.l[k] = l;
        sp.r[k] = r;
        sp.unit[k] = (unsigned char)unit[k];
        used[unit[k]] = true;
    }
    for (int u = 0; u < U; u++) MVP_REQUIRE(used[u], "%s: unit %d has no pair (n_units=%d)", fn, u, U);
    return sp;
}

inline LsPlan ls_plan(const char* fn, int T, int J, int nv, int NS, int U) {
    ls_check_shape(fn, T, J, nv, NS, U);
    LsPlan pl;
    pl.n_pairs = nv * (nv - 1) / 2;
    int64_t b = 0;
    pl.off_und = b;
    b = sy_align256(b + (int64_t)nv * T * J * 8);
    pl.off_f = b;
    b = sy_align256(b + (int64_t)pl.n_pairs * 9 * 8);
    const int64_t bp = (int64_t)U * ls_bp_stride(T, nv);   // the solver's use of the same workspace
    pl.bytes = b > bp ? b : bp;
    return pl;
}

// ------------------------------------------------------------------ costs
struct LsCostArgs {
    const float* kpts;   // [T][J][3][V]
    const float2* und;   // [nv][T·J]
    const double* fmat;  // [NP][9]
    double *same, *cross, *keep, *change, *prior;
    int* n;              // [T][U][nv] or null
    int T, J, V, U, nv, n_pairs;
    double tau2, mu2, w, prior2;
    CamIdx ci;
    LsPairs sp;
};

// d² of x_a against x_b, and whether it counts (denominator non-zero, d² finite)
__device__ __forceinline__ bool ls_sampson(const double (&la)[4], double xb, double yb, double gb, double& d2) {
#pragma clang fp contract(fast)
    const double num = xb * la[0] + yb * la[1] + la[2];
    const double den = la[3] + gb;
    d2 = num * num * rcp_nr(den);
    return den != 0.0 && __builtin_isfinite(d2);
}

__global__ __launch_bounds__(kBlock) void ls_cost_kernel(LsCostArgs g) {
#pragma clang fp contract(fast)
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= (int64_t)g.T * g.U) return;
    const int t = (int)(e / g.U), u = (int)(e - (int64_t)t * g.U);
    const int J = g.J, V = g.V, nv = g.nv, ns = g.sp.ns;
    const int64_t n = (int64_t)g.T * J;
    const int64_t f0 = (int64_t)t * J;   // the frame's first keypoint
    for (int a = 0; a < nv; a++) {
        const float2* ua = g.und + a * n + f0;
        const int col = g.ci.v[a];
        int cnt = 0;
        double keep = 0.0, change = 0.0;
        for (int k = 0; k < ns; k++) {
            if (g.sp.unit[k] != u) continue;
            const int l = g.sp.l[k], r = g.sp.r[k];
            if (isnan(ua[l].x) || isnan(ua[r].x)) continue;   // not usable, or no ideal pixel (mvpose.h)
            cnt++;
            if (t == 0 || isnan(ua[l - J].x) || isnan(ua[r - J].x)) continue;
            const float* kl = g.kpts + (f0 + l) * 3 * V + col;
            const float* kr = g.kpts + (f0 + r) * 3 * V + col;
            const int64_t back = (int64_t)J * 3 * V;
            const double lx = kl[0], ly = kl[V], rx = kr[0], ry = kr[V];
            const double plx = kl[-back], ply = kl[V - back], prx = kr[-back], pry = kr[V - back];
            const double dll = (lx - plx) * (lx - plx) + (ly - ply) * (ly - ply);
            const double drr = (rx - prx) * (rx - prx) + (ry - pry) * (ry - pry);
            const double dlr = (lx - prx) * (lx - prx) + (ly - pry) * (ly - pry);
            const double drl = (rx - plx) * (rx - plx) + (ry - ply) * (ry - ply);
            keep += (dll < g.mu2 ? dll : g.mu2) + (drr < g.mu2 ? drr : g.mu2);
            change += (dlr < g.mu2 ? dlr : g.mu2) + (drl < g.mu2 ? drl : g.mu2);
        }
        const int64_t o = e * nv + a;
        g.keep[o] = g.w * keep;
        g.change[o] = g.w * change;
        g.prior[o] = g.prior2 * (double)cnt;
        if (g.n) g.n[o] = cnt;
    }
    int p = 0;
    for (int a = 0; a < nv; a++)
        for (int b = a + 1; b < nv; b++, p++) {
            const double* F = g.fmat + 9 * p;
            const double f00 = F[0], f01 = F[1], f02 = F[2], f10 = F[3], f11 = F[4], f12 = F[5], f20 = F[6],
                         f21 = F[7], f22 = F[8];
            const float2* ua = g.und + a * n + f0;
            const float2* ub = g.und + b * n + f0;
            double same = 0.0, cross = 0.0;
            for (int k = 0; k < ns; k++) {
                if (g.sp.unit[k] != u) continue;
                const float2 al = ua[g.sp.l[k]], ar = ua[g.sp.r[k]], bl = ub[g.sp.l[k]], br = ub[g.sp.r[k]];
                // the lines F x_a with l0² + l1², and (Fᵀ x_b)₀² + (Fᵀ x_b)₁²
                double line[2][4], gb[2], xb[2], yb[2];
                const float2 pa[2] = {al, ar}, pb[2] = {bl, br};
#pragma unroll
                for (int i = 0; i < 2; i++) {
                    const double x = pa[i].x, y = pa[i].y;
                    line[i][0] = f00 * x + f01 * y + f02;
                    line[i][1] = f10 * x + f11 * y + f12;
                    line[i][2] = f20 * x + f21 * y + f22;
                    line[i][3] = line[i][0] * line[i][0] + line[i][1] * line[i][1];
                    xb[i] = pb[i].x;
                    yb[i] = pb[i].y;
                    const double g0 = f00 * xb[i] + f10 * yb[i] + f20, g1 = f01 * xb[i] + f11 * yb[i] + f21;
                    gb[i] = g0 * g0 + g1 * g1;
                }
                double dll, drr, dlr, drl;
                bool ok = ls_sampson(line[0], xb[0], yb[0], gb[0], dll);
                ok &= ls_sampson(line[1], xb[1], yb[1], gb[1], drr);
                ok &= ls_sampson(line[0], xb[1], yb[1], gb[1], dlr);
                ok &= ls_sampson(line[1], xb[0], yb[0], gb[0], drl);
                if (!ok) continue;   // an unusable keypoint is NaN and lands here too
                same += (dll < g.tau2 ? dll : g.tau2) + (drr < g.tau2 ? drr : g.tau2);
                cross += (dlr < g.tau2 ? dlr : g.tau2) + (drl < g.tau2 ? drl : g.tau2);
            }
            g.same[e * g.n_pairs + p] = same;
            g.cross[e * g.n_pairs + p] = cross;
        }
}

// ------------------------------------------------------------------ solve
struct LsSolveArgs {
    const double *same, *cross, *keep, *change, *prior;   // [T][U][NP] x2, [T][U][nv] x3
    unsigned char* bp;    // [U][stride]: unit u's [T][2^nv] bytes
    unsigned char* swap;  // [T][U]
    double* cost;         // [U] or null
    int64_t stride;
    int T, U, nv, n_pairs;
};

// lane l's value as a wave-uniform one
__device__ __forceinline__ double ls_read_lane(double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// One frame's rows, entry i in lane i (NP <= 28 and nv <= 8 entries).
struct LsRow {
    double same, cross, keep, change, prior;
};

__device__ __forceinline__ LsRow ls_load_row(const LsSolveArgs& g, int64_t tu, int lane) {
    // lanes past a row's end re-read its entry 0: loads without a branch around them
    const int64_t ip = tu * g.n_pairs + (lane < g.n_pairs ? lane : 0), iv = tu * g.nv + (lane < g.nv ? lane : 0);
    return LsRow{g.same[ip], g.cross[ip], g.keep[iv], g.change[iv], g.prior[iv]};
}

template <int NR>
__global__ __launch_bounds__(kLsWave) void ls_solve_kernel(LsSolveArgs g) {
    __shared__ __attribute__((aligned(16))) unsigned char s_bp[kLsChunkBytes];
    const int lane = threadIdx.x;
    const int u = blockIdx.x;
    const int nv = g.nv, T = g.T, U = g.U;
    const int S = 1 << nv;
    // nv < 6: lanes S and up repeat the states of lanes 0 .. S-1 (a pass pairs lanes inside one group
    // of S, so every group computes the same values) and store the same bytes to the same addresses:
    // no branch around the store, so the wait for the next frame's rows need not wait for the store
    const int s0 = lane & (S - 1);
    unsigned char* bp = g.bp + (int64_t)u * g.stride;
    double G[NR];
    int flip[NR];
    // the rows of the next kLsAhead frames are in flight while a frame is worked on: the loop below is
    // unrolled by kLsAhead so that the ring stays in registers (past the end, frame T-1 is re-read)
    LsRow ring[kLsAhead];
#pragma unroll
    for (int d = 0; d < kLsAhead; d++) ring[d] = ls_load_row(g, (int64_t)(d < T ? d : T - 1) * U + u, lane);
    for (int t0 = 0; t0 < T; t0 += kLsAhead) {
#pragma unroll
      for (int d = 0; d < kLsAhead; d++) {
        const int t = t0 + d;
        if (t >= T) break;
        const LsRow row = ring[d];
        ring[d] = ls_load_row(g, (int64_t)(t + kLsAhead < T ? t + kLsAhead : T - 1) * U + u, lane);
        // E(t, s): the prior of the set bits, views ascending, then the view pairs ascending
        double E[NR];
#pragma unroll
        for (int r = 0; r < NR; r++) E[r] = 0.0;
        for (int a = 0; a < nv; a++) {
            const double pr = ls_read_lane(row.prior, a);
#pragma unroll
            for (int r = 0; r < NR; r++)
                if (((r * kLsWave + s0) >> a) & 1) E[r] += pr;
        }
        int p = 0;
        for (int a = 0; a < nv; a++)
            for (int b = a + 1; b < nv; b++, p++) {
                const double sm = ls_read_lane(row.same, p), cr = ls_read_lane(row.cross, p);
#pragma unroll
                for (int r = 0; r < NR; r++) {
                    const int s = r * kLsWave + s0;
                    E[r] += (((s >> a) ^ (s >> b)) & 1) ? cr : sm;
                }
            }
        if (t == 0) {
#pragma unroll
            for (int r = 0; r < NR; r++) {
                G[r] = E[r];
                flip[r] = 0;
            }
        } else {
#pragma unroll
            for (int r = 0; r < NR; r++) flip[r] = 0;
            // bits held by the lane: the partner state is another lane's
            const int na = nv < 6 ? nv : 6;
            for (int a = 0; a < na; a++) {
                const double kp = ls_read_lane(row.keep, a), ch = ls_read_lane(row.change, a);
#pragma unroll
                for (int r = 0; r < NR; r++) {
                    const double go = __shfl_xor(G[r], 1 << a);
                    const int fo = __shfl_xor(flip[r], 1 << a);
                    const double k = G[r] + kp, c = go + ch;
                    const bool take = c < k;
                    G[r] = take ? c : k;
                    flip[r] = take ? (fo | (1 << a)) : flip[r];
                }
            }
            // bits held by the register index: the partner state is this lane's register r xor 2^(a-6)
#pragma unroll
            for (int h = 1; h < NR; h <<= 1) {
                const int a = h == 1 ? 6 : 7;
                const double kp = ls_read_lane(row.keep, a), ch = ls_read_lane(row.change, a);
                double Gn[NR];
                int fn[NR];
#pragma unroll
                for (int r = 0; r < NR; r++) {
                    const double k = G[r] + kp, c = G[r ^ h] + ch;
                    const bool take = c < k;
                    Gn[r] = take ? c : k;
                    fn[r] = take ? (flip[r ^ h] | (1 << a)) : flip[r];
                }
#pragma unroll
                for (int r = 0; r < NR; r++) {
                    G[r] = Gn[r];
                    flip[r] = fn[r];
                }
            }
#pragma unroll
            for (int r = 0; r < NR; r++) G[r] += E[r];
        }
#pragma unroll
        for (int r = 0; r < NR; r++) bp[((int64_t)t << nv) + r * kLsWave + s0] = (unsigned char)flip[r];
      }
    }

    // the smallest state that attains min D_{T-1}
    const double inf = __builtin_inf();
    double mn = inf;
#pragma unroll
    for (int r = 0; r < NR; r++) mn = G[r] < mn ? G[r] : mn;
    for (int off = kLsWave / 2; off; off >>= 1) {
        const double o = __shfl_xor(mn, off);
        mn = o < mn ? o : mn;
    }
    int s = 0;
    bool found = false;
#pragma unroll
    for (int r = 0; r < NR; r++) {
        const unsigned long long at = __ballot(G[r] == mn);
        if (!found && at) {
            s = r * kLsWave + __builtin_ctzll(at);   // the lowest lane that holds it is in the first group
            found = true;
        }
    }
    if (lane == 0 && g.cost) g.cost[u] = mn;

    // backtrack: bp written by all lanes above is read back by all lanes below
    __threadfence();
    __syncthreads();
    const int C = kLsChunkBytes >> nv < kLsChunkFrames ? kLsChunkBytes >> nv : kLsChunkFrames;
    for (int t0 = (T - 1) / C * C; t0 >= 0; t0 -= C) {
        const int nf = T - t0 < C ? T - t0 : C;
        const int words = (nf << nv) / 4;   // 2^nv >= 4
        const uint32_t* src = reinterpret_cast<const uint32_t*>(bp + ((int64_t)t0 << nv));
        uint32_t* dst = reinterpret_cast<uint32_t*>(s_bp);
        for (int w = lane; w < words; w += kLsWave) dst[w] = src[w];
        __syncthreads();
        if (lane == 0)
            for (int t = t0 + nf - 1; t >= t0; t--) {
                g.swap[(int64_t)t * U + u] = (unsigned char)s;
                s ^= s_bp[((t - t0) << nv) + s];   // bp[0] is zero
            }
        __syncthreads();
    }
}

// ------------------------------------------------------------------ apply
struct LsApplyArgs {
    const unsigned char* swap;   // [T][U]
    int T, J, V, C, U;
    signed char bit[64];         // column -> its position in cam_idx, -1: not listed
    LsPairs sp;
};

// (partner, unit) of joint j, partner = -1 when j is in no pair
__device__ __forceinline__ int ls_partner(const LsPairs& sp, int j, int& unit) {
    int partner = -1;
    unit = 0;
    for (int k = 0; k < sp.ns; k++) {
        const int l = sp.l[k], r = sp.r[k];
        if (j == l || j == r) {
            partner = j == l ? r : l;
            unit = sp.unit[k];
        }
    }
    return partner;
}

__global__ __launch_bounds__(kBlock) void ls_apply_kpts_kernel(LsApplyArgs g, const uint32_t* __restrict__ in,
                                                               uint32_t* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;   // (t, j, row)
    if (e >= (int64_t)g.T * g.J * 3) return;
    const int64_t tj = e / 3;
    const int row = (int)(e - tj * 3);
    const int64_t t = tj / g.J;
    const int j = (int)(tj - t * g.J);
    int unit;
    const int partner = ls_partner(g.sp, j, unit);
    const int mask = partner >= 0 ? g.swap[t * g.U + unit] : 0;
    const int64_t from = ((t * g.J + partner) * 3 + row) * g.V;
    for (int col = 0; col < g.V; col++) {
        const int b = g.bit[col];
        const bool sw = b >= 0 && ((mask >> b) & 1);
        out[e * g.V + col] = in[(sw ? from : e * g.V) + col];
    }
}

__global__ __launch_bounds__(kBlock) void ls_apply_gauss_kernel(LsApplyArgs g, const double* __restrict__ in,
                                                                double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;   // (t, col, j)
    if (e >= (int64_t)g.T * g.V * g.J) return;
    const int64_t tv = e / g.J;
    const int j = (int)(e - tv * g.J);
    const int64_t t = tv / g.V;
    const int col = (int)(tv - t * g.V);
    int unit;
    const int partner = ls_partner(g.sp, j, unit);
    const int b = g.bit[col];
    const bool sw = partner >= 0 && b >= 0 && ((g.swap[t * g.U + unit] >> b) & 1);
    const int64_t from = sw ? tv * g.J + partner : e;
    const unsigned long long* src = reinterpret_cast<const unsigned long long*>(in) + from * g.C;
    unsigned long long* dst = reinterpret_cast<unsigned long long*>(out) + e * g.C;
    for (int c = 0; c < g.C; c++) dst[c] = src[c];
}

}  // namespace

extern "C" int mvp_label_swap_plan(int T, int J, int n_cam_idx, int n_pairs, int n_units, int64_t* workspace_bytes) {
    MVP_ABI_BEGIN
    const LsPlan pl = ls_plan("mvp_label_swap_plan", T, J, n_cam_idx, n_pairs, n_units);
    if (workspace_bytes) *workspace_bytes = pl.bytes;
    MVP_ABI_END
}

extern "C" int mvp_label_swap_costs(const float* kpts, int T, int J, int V, const double* cams, int n_cams,
                                    const int* cam_idx, int n_cam_idx, const int* pairs, int n_pairs, const int* unit,
                                    int n_units, float min_conf, float trunc_px, float motion_trunc_px,
                                    float motion_weight, float swap_prior_px, void* workspace, int64_t workspace_bytes,
                                    double* out_same, double* out_cross, double* out_keep, double* out_change,
                                    double* out_prior, int32_t* out_n, void* stream) {
    MVP_ABI_BEGIN
    const char* fn = "mvp_label_swap_costs";
    const LsPlan pl = ls_plan(fn, T, J, n_cam_idx, n_pairs, n_units);
    const CamIdx ci = tri_parse_args(fn, (int64_t)T * J, V, n_cams, cam_idx, n_cam_idx);
    const LsPairs sp = ls_parse_pairs(fn, J, pairs, n_pairs, unit, n_units);
    MVP_REQUIRE(!std::isnan(min_conf), "%s: min_conf is NaN", fn);
    MVP_REQUIRE(std::isfinite(trunc_px) && trunc_px > 0.f, "%s: trunc_px=%g (finite, > 0)", fn, (double)trunc_px);
    MVP_REQUIRE(std::isfinite(motion_trunc_px) && motion_trunc_px > 0.f, "%s: motion_trunc_px=%g (finite, > 0)", fn,
                (double)motion_trunc_px);
    MVP_REQUIRE(std::isfinite(motion_weight) && motion_weight >= 0.f, "%s: motion_weight=%g (finite, >= 0)", fn,
                (double)motion_weight);
    MVP_REQUIRE(std::isfinite(swap_prior_px) && swap_prior_px >= 0.f, "%s: swap_prior_px=%g (finite, >= 0)", fn,
                (double)swap_prior_px);
    const int64_t need = pl.off_f + sy_align256((int64_t)pl.n_pairs * 72);
    MVP_REQUIRE(workspace_bytes >= need, "%s: workspace_bytes=%lld < %lld needed (T=%d, J=%d, n_cam_idx=%d)", fn,
                (long long)workspace_bytes, (long long)need, T, J, n_cam_idx);
    MVP_REQUIRE(kpts && cams && workspace && out_same && out_cross && out_keep && out_change && out_prior,
                "%s: null device pointer", fn);
    const int64_t n = (int64_t)T * J;
    SyncPairs pr{};
    const int np = sync_list_pairs(n_cam_idx, pr);
    char* ws = static_cast<char*>(workspace);
    LsCostArgs g{};
    g.kpts = kpts;
    g.und = reinterpret_cast<float2*>(ws + pl.off_und);
    g.fmat = reinterpret_cast<double*>(ws + pl.off_f);
    g.same = out_same;
    g.cross = out_cross;
    g.keep = out_keep;
    g.change = out_change;
    g.prior = out_prior;
    g.n = out_n;
    g.T = T;
    g.J = J;
    g.V = V;
    g.U = n_units;
    g.nv = n_cam_idx;
    g.n_pairs = np;
    g.tau2 = (double)trunc_px * (double)trunc_px;
    g.mu2 = (double)motion_trunc_px * (double)motion_trunc_px;
    g.w = (double)motion_weight;
    g.prior2 = (double)swap_prior_px * (double)swap_prior_px;
    g.ci = ci;
    g.sp = sp;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(sync_fundamental_kernel, dim3(1), dim3(64), 0, s, cams, ci, pr, np,
                       reinterpret_cast<double*>(ws + pl.off_f));
    MVP_HIP(hipGetLastError());
    hipLaunchKernelGGL(sync_undistort_kernel, dim3(tri_grid(fn, n), (unsigned)n_cam_idx), dim3(kBlock), 0, s, kpts, n, V,
                       cams, n_cams, ci, min_conf, reinterpret_cast<float2*>(ws + pl.off_und));
    MVP_HIP(hipGetLastError());
    hipLaunchKernelGGL(ls_cost_kernel, dim3(tri_grid(fn, (int64_t)T * n_units)), dim3(kBlock), 0, s, g);
    MVP_HIP(hipGetLastError());
    MVP_ABI_END
}

// The solver's argument checks; returns the bytes of one unit's bp.
static int64_t ls_solve_stride(const char* fn, int T, int n_units, int n_cam_idx) {
    MVP_REQUIRE(T >= 1, "%s: T=%d < 1", fn, T);
    MVP_REQUIRE(n_cam_idx >= 2 && n_cam_idx <= kMaxCams, "%s: n_cam_idx=%d (2..%d)", fn, n_cam_idx, kMaxCams);
    MVP_REQUIRE(n_units >= 1 && n_units <= kLsMaxPairs, "%s: n_units=%d (1..%d)", fn, n_units, kLsMaxPairs);
    return ls_bp_stride(T, n_cam_idx);
}

extern "C" int mvp_label_swap_solve_plan(int T, int n_units, int n_cam_idx, int64_t* workspace_bytes) {
    MVP_ABI_BEGIN
    const int64_t stride = ls_solve_stride("mvp_label_swap_solve_plan", T, n_units, n_cam_idx);
    if (workspace_bytes) *workspace_bytes = (int64_t)n_units * stride;
    MVP_ABI_END
}

extern "C" int mvp_label_swap_solve(const double* same, const double* cross, const double* keep, const double* change,
                                    const double* prior, int T, int n_units, int n_cam_idx, void* workspace,
                                    int64_t workspace_bytes, uint8_t* out_swap, double* out_cost, void* stream) {
    MVP_ABI_BEGIN
    const char* fn = "mvp_label_swap_solve";
    LsSolveArgs g{};
    g.stride = ls_solve_stride(fn, T, n_units, n_cam_idx);
    const int64_t need = (int64_t)n_units * g.stride;
    MVP_REQUIRE(workspace_bytes >= need, "%s: workspace_bytes=%lld < %lld needed (T=%d, n_units=%d, n_cam_idx=%d)", fn,
                (long long)workspace_bytes, (long long)need, T, n_units, n_cam_idx);
    MVP_REQUIRE(same && cross && keep && change && prior && workspace && out_swap, "%s: null device pointer", fn);
    g.same = same;
    g.cross = cross;
    g.keep = keep;
    g.change = change;
    g.prior = prior;
    g.bp = static_cast<unsigned char*>(workspace);
    g.swap = out_swap;
    g.cost = out_cost;
    g.T = T;
    g.U = n_units;
    g.nv = n_cam_idx;
    g.n_pairs = n_cam_idx * (n_cam_idx - 1) / 2;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)n_units), block(kLsWave);
    if (n_cam_idx <= 6)
        hipLaunchKernelGGL(ls_solve_kernel<1>, grid, block, 0, s, g);
    else if (n_cam_idx == 7)
        hipLaunchKernelGGL(ls_solve_kernel<2>, grid, block, 0, s, g);
    else
        hipLaunchKernelGGL(ls_solve_kernel<4>, grid, block, 0, s, g);
    MVP_HIP(hipGetLastError());
    MVP_ABI_END
}

extern "C" int mvp_label_swap_apply(const float* kpts, const double* gauss, int T, int J, int V, int C,
                                    const int* cam_idx, int n_cam_idx, const int* pairs, int n_pairs, const int* unit,
                                    int n_units, const uint8_t* swap, float* out_kpts, double* out_gauss, void* stream) {
    MVP_ABI_BEGIN
    const char* fn = "mvp_label_swap_apply";
    ls_check_shape(fn, T, J, n_cam_idx, n_pairs, n_units);
    MVP_REQUIRE(V >= 2 && V <= 64, "%s: V=%d out of range", fn, V);
    MVP_REQUIRE(cam_idx != nullptr, "%s: cam_idx is NULL", fn);
    LsApplyArgs g{};
    for (int c = 0; c < 64; c++) g.bit[c] = -1;
    for (int i = 0; i < n_cam_idx; i++) {
        MVP_REQUIRE(cam_idx[i] >= 0 && cam_idx[i] < V, "%s: cam_idx[%d]=%d out of range (V=%d)", fn, i, cam_idx[i], V);
        MVP_REQUIRE(g.bit[cam_idx[i]] < 0, "%s: cam_idx[%d]=%d is listed twice", fn, i, cam_idx[i]);
        g.bit[cam_idx[i]] = (signed char)i;
    }
    g.sp = ls_parse_pairs(fn, J, pairs, n_pairs, unit, n_units);
    MVP_REQUIRE((gauss == nullptr) == (out_gauss == nullptr), "%s: gauss and out_gauss go together", fn);
    MVP_REQUIRE(gauss == nullptr || C >= 1, "%s: C=%d < 1", fn, C);
    MVP_REQUIRE(kpts && out_kpts && swap, "%s: null device pointer", fn);
    MVP_REQUIRE(kpts != out_kpts && (gauss == nullptr || gauss != out_gauss), "%s: the outputs must not be the inputs", fn);
    g.swap = swap;
    g.T = T;
    g.J = J;
    g.V = V;
    g.C = C;
    g.U = n_units;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(ls_apply_kpts_kernel, dim3(tri_grid(fn, (int64_t)T * J * 3)), dim3(kBlock), 0, s, g,
                       reinterpret_cast<const uint32_t*>(kpts), reinterpret_cast<uint32_t*>(out_kpts));
    MVP_HIP(hipGetLastError());
    if (gauss) {
        hipLaunchKernelGGL(ls_apply_gauss_kernel, dim3(tri_grid(fn, (int64_t)T * V * J)), dim3(kBlock), 0, s, g, gauss,
                           out_gauss);
        MVP_HIP(hipGetLastError());
    }
    MVP_ABI_END
}
