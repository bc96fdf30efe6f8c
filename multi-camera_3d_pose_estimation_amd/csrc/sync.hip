// Epipolar lag-cost scan (mvp_epipolar_lag_cost; the problem is stated in include/mvpose.h; no
// reference counterpart: the reference synchronises by an audio clap and a typed frame number)
// for gfx950.
//
// For every pair (a, b) of listed views and every lag l in [-L, L] the truncated Sampson
// distances of a's keypoints at frame t against b's at frame t + l are summed over all frames and
// joints.  Four stream-ordered launches, arithmetic in fp64:
//
//   fundamental  one lane per pair: F_ab = K_b⁻ᵀ [t]ₓ R K_a⁻¹ from the packed camera records.
//   undistort    one lane per (view, frame, joint): the f32 undistorted pixel every triangulator
//                uses (undistort_point), once, into a workspace plane [view][frame·J + joint] of
//                float2; an unusable keypoint is stored as NaN, so the scan needs no flags: a NaN
//                poisons d², and a term whose d² is not finite is skipped.
//   scan         one workgroup per (time tile, lag chunk, pair).  It stages the tile's frames of
//                view a in LDS as the epipolar line of each keypoint, (F x_a, |F x_a|²₀₁) = 32 B,
//                and view b's frames [t0 + l0, t0 + B + l0 + n_lags - 1) as (f32 pixel,
//                |Fᵀ x_b|²₀₁) = 16 B: each keypoint of b is read from memory once per tile and
//                used by up to 2L+1 lags, and everything that depends on one view only is
//                computed once per staged keypoint, not once per lag.  What is left per (keypoint,
//                lag) is x_b · (F x_a), one addition for the denominator and the division (a
//                v_rcp_f64 with two Newton steps: ~1 ulp, a zero or non-finite denominator gives a
//                non-finite d², which is skipped).  The halo can be longer than the tile.  A lane
//                owns one lag and every S-th keypoint of the tile (S = 256 / lags in the chunk):
//                the a-side read is a broadcast, the b-side reads of neighbouring lags are J·16
//                bytes apart, and the lane's sum and count stay in registers until the tile is
//                done.  The S partial sums of a lag are then added in LDS in slice order and
//                written to [pair][tile][lag].
//   reduce       one workgroup per (lag, pair): each lane adds the tiles tid, tid + 256, ... in
//                that order, then a fixed binary tree in LDS.
// No atomics anywhere: the same inputs give the same bits on every call.  The first two launches
// are in sync_common.h: mvp_associate_views (associate.hip) starts with the same two.
//
// Tile: B frames of a, and as many lags per chunk as fit in 60 KiB of LDS beside them (J = 17:
// B = 32, up to 130 lags, so L = 60 is one chunk of 121; 58 752 B + 3 KiB, two workgroups per CU).
// Register / LDS / occupancy figures and the measurements are in DESIGN.md §4.10.
#pragma clang fp contract(off)

#include "sync_common.h"

namespace {

constexpr int kSyBlock = 256;
constexpr int kSyMaxTile = 64;            // frames of view a per workgroup
constexpr int kSyLdsBytes = 60 * 1024;    // the two staged tiles; 4 KiB beside them for the block reduction
constexpr int kSyMaxJoints = 1024;        // a frame of a's lines and one of b (6 units) must fit in the LDS budget

struct SyncPlan {
    int tile, lag_chunk, n_tiles, n_lags, n_chunks, n_pairs;
    int64_t off_und, off_f, off_psum, off_pcnt, bytes;
};

// Frames are counted in units of J·8 bytes: a frame of view a costs 4 such units (its lines are
// 32 B per keypoint), a frame of b two.  The tile takes at most 6/14 of the budget, the rest holds
// the lags of a chunk.
inline SyncPlan sync_plan(const char* fn, int T, int J, int nv, int L) {
    MVP_REQUIRE(T >= 1, "%s: T=%d < 1", fn, T);
    MVP_REQUIRE(J >= 1 && J <= kSyMaxJoints, "%s: J=%d (1..%d)", fn, J, kSyMaxJoints);
    MVP_REQUIRE(nv >= 2 && nv <= kMaxCams, "%s: n_cam_idx=%d (2..%d)", fn, nv, kMaxCams);
    MVP_REQUIRE(L >= 0 && L < T, "%s: max_lag=%d must satisfy 0 <= max_lag < T=%d", fn, L, T);
    MVP_REQUIRE((int64_t)T * J < (1LL << 31), "%s: T*J=%lld too large", fn, (long long)T * J);
    SyncPlan pl;
    const int units = kSyLdsBytes / (8 * J);
    int B = units / 14;
    B = B < 1 ? 1 : B > kSyMaxTile ? kSyMaxTile : B;
    B = B > T ? T : B;
    pl.tile = B;
    pl.n_lags = 2 * L + 1;
    int lc = (units - 6 * B) / 2 + 1;
    lc = lc > kSyBlock ? kSyBlock : lc;
    pl.lag_chunk = lc > pl.n_lags ? pl.n_lags : lc;
    pl.n_tiles = (T + B - 1) / B;
    pl.n_chunks = (pl.n_lags + pl.lag_chunk - 1) / pl.lag_chunk;
    pl.n_pairs = nv * (nv - 1) / 2;
    MVP_REQUIRE(pl.n_chunks <= 65535, "%s: max_lag=%d needs %d lag chunks (at most 65535)", fn, L, pl.n_chunks);
    int64_t b = 0;
    pl.off_und = b;
    b = sy_align256(b + (int64_t)nv * T * J * 8);
    pl.off_f = b;
    b = sy_align256(b + (int64_t)pl.n_pairs * 9 * 8);
    pl.off_psum = b;
    b = sy_align256(b + (int64_t)pl.n_pairs * pl.n_tiles * pl.n_lags * 8);
    pl.off_pcnt = b;
    b = sy_align256(b + (int64_t)pl.n_pairs * pl.n_tiles * pl.n_lags * 4);
    pl.bytes = b;
    return pl;
}

// A staged keypoint of view b: its f32 pixel and (Fᵀ x_b)₀² + (Fᵀ x_b)₁².
struct __attribute__((aligned(16))) SyncB {
    float x, y;
    double w;
};

struct ScanArgs {
    const float2* und;   // [nv][T·J]
    const double* fmat;  // [n_pairs][9]
    double* psum;        // [n_pairs][n_tiles][n_lags]
    int* pcnt;
    int T, J, L, tile, lag_chunk, n_tiles, n_lags;
    double tau2;
    SyncPairs pr;
};

// LDS bytes of the two staged tiles, rounded up to 16: a's lines (32 B per keypoint of a full tile)
// and b's entries (16 B) of tile + lag_chunk - 1 frames.  The block reduction's 3 KiB follow.
__host__ __device__ inline size_t scan_lds_tiles(int tile, int lag_chunk, int J) {
    return ((size_t)tile * J * 32 + (size_t)(tile + lag_chunk - 1) * J * 16 + 15) / 16 * 16;
}

__global__ __launch_bounds__(kSyBlock) void sync_scan_kernel(ScanArgs g) {
#pragma clang fp contract(fast)
    // everything in the dynamic region, every piece 16-byte aligned: [a's lines | b's pixels | sums | counts]
    extern __shared__ __attribute__((aligned(16))) char sy_smem[];
    const int tid = threadIdx.x;
    const int tile = blockIdx.x, chunk = blockIdx.y, pair = blockIdx.z;
    const int J = g.J;
    const int t0 = tile * g.tile;
    const int na = (g.T - t0 < g.tile ? g.T - t0 : g.tile) * J;        // a's keypoints in the tile
    const int k0 = chunk * g.lag_chunk;                                // first lag index of the chunk
    const int nl = g.n_lags - k0 < g.lag_chunk ? g.n_lags - k0 : g.lag_chunk;
    const int nb = na + (nl - 1) * J;                                  // b's keypoints staged
    const int64_t n = (int64_t)g.T * J;
    double4* sa = reinterpret_cast<double4*>(sy_smem);                 // [na] (l0, l1, l2, l0² + l1²)
    SyncB* sb = reinterpret_cast<SyncB*>(sy_smem + (size_t)g.tile * J * 32);   // [nb]
    double* s_sum = reinterpret_cast<double*>(sy_smem + scan_lds_tiles(g.tile, g.lag_chunk, J));
    int* s_cnt = reinterpret_cast<int*>(s_sum + kSyBlock);
    const double* F = g.fmat + 9 * pair;
    const double f00 = F[0], f01 = F[1], f02 = F[2], f10 = F[3], f11 = F[4], f12 = F[5], f20 = F[6], f21 = F[7],
                 f22 = F[8];
    const float2* ua = g.und + (int64_t)g.pr.a[pair] * n + (int64_t)t0 * J;
    for (int e = tid; e < na; e += kSyBlock) {
        const float2 p = ua[e];
        const double x = p.x, y = p.y;
        const double l0 = f00 * x + f01 * y + f02, l1 = f10 * x + f11 * y + f12, l2 = f20 * x + f21 * y + f22;
        sa[e] = make_double4(l0, l1, l2, l0 * l0 + l1 * l1);
    }
    // b's frame of staged row r is t0 + (k0 - L) + r; frames outside the recording are NaN
    const int64_t b0 = ((int64_t)t0 + k0 - g.L) * J;
    const float2* ub = g.und + (int64_t)g.pr.b[pair] * n;
    const float qnan = __builtin_nanf("");
    for (int e = tid; e < nb; e += kSyBlock) {
        const int64_t q = b0 + e;
        const float2 p = (q >= 0 && q < n) ? ub[q] : make_float2(qnan, qnan);
        const double x = p.x, y = p.y;
        const double g0 = f00 * x + f10 * y + f20, g1 = f01 * x + f11 * y + f21;
        sb[e] = SyncB{p.x, p.y, g0 * g0 + g1 * g1};
    }
    __syncthreads();
    const int slices = kSyBlock / nl;
    const int lag = tid % nl, slice = tid / nl;
    double sum = 0.0;
    int cnt = 0;
    if (slice < slices) {
        const SyncB* sbl = sb + lag * J;
#pragma unroll 4
        for (int e = slice; e < na; e += slices) {
            const double4 a = sa[e];
            const SyncB b = sbl[e];
            const double num = (double)b.x * a.x + (double)b.y * a.y + a.z;
            const double den = a.w + b.w;
            const double d2 = num * num * rcp_nr(den);
            const bool ok = den != 0.0 && __builtin_isfinite(d2);
            sum += ok ? (d2 < g.tau2 ? d2 : g.tau2) : 0.0;
            cnt += ok ? 1 : 0;
        }
    }
    s_sum[tid] = sum;
    s_cnt[tid] = cnt;
    __syncthreads();
    if (tid < nl) {
        double s = 0.0;
        int c = 0;
        for (int k = 0; k < slices; k++) {
            s += s_sum[k * nl + tid];
            c += s_cnt[k * nl + tid];
        }
        const int64_t o = ((int64_t)pair * g.n_tiles + tile) * g.n_lags + k0 + tid;
        g.psum[o] = s;
        g.pcnt[o] = c;
    }
}

__global__ __launch_bounds__(kSyBlock) void sync_reduce_kernel(const double* __restrict__ psum,
                                                               const int* __restrict__ pcnt, int n_tiles, int n_lags,
                                                               double* __restrict__ out_sum,
                                                               int64_t* __restrict__ out_cnt) {
    __shared__ double s_sum[kSyBlock];
    __shared__ int64_t s_cnt[kSyBlock];
    const int tid = threadIdx.x;
    const int lag = blockIdx.x, pair = blockIdx.y;
    double s = 0.0;
    int64_t c = 0;
    for (int t = tid; t < n_tiles; t += kSyBlock) {
        const int64_t o = ((int64_t)pair * n_tiles + t) * n_lags + lag;
        s += psum[o];
        c += pcnt[o];
    }
    s_sum[tid] = s;
    s_cnt[tid] = c;
    __syncthreads();
    for (int w = kSyBlock / 2; w > 0; w >>= 1) {
        if (tid < w) {
            s_sum[tid] += s_sum[tid + w];
            s_cnt[tid] += s_cnt[tid + w];
        }
        __syncthreads();
    }
    if (tid == 0) {
        out_sum[(int64_t)pair * n_lags + lag] = s_sum[0];
        out_cnt[(int64_t)pair * n_lags + lag] = s_cnt[0];
    }
}

}  // namespace

extern "C" int mvp_epipolar_lag_cost_plan(int T, int J, int n_cam_idx, int max_lag, int* tile_out,
                                          int64_t* workspace_bytes) {
    MVP_ABI_BEGIN
    const SyncPlan pl = sync_plan("mvp_epipolar_lag_cost_plan", T, J, n_cam_idx, max_lag);
    if (tile_out) *tile_out = pl.tile;
    if (workspace_bytes) *workspace_bytes = pl.bytes;
    MVP_ABI_END
}

extern "C" int mvp_epipolar_lag_cost(const float* kpts, int T, int J, int V, const double* cams, int n_cams,
                                     const int* cam_idx, int n_cam_idx, int max_lag, float min_conf, float trunc_px,
                                     void* workspace, int64_t workspace_bytes, double* out_sum, int64_t* out_cnt,
                                     void* stream) {
    MVP_ABI_BEGIN
    const char* fn = "mvp_epipolar_lag_cost";
    MVP_REQUIRE(T >= 1 && J >= 1, "%s: T=%d, J=%d must be >= 1", fn, T, J);
    const CamIdx ci = tri_parse_args(fn, (int64_t)T * J, V, n_cams, cam_idx, n_cam_idx);
    const SyncPlan pl = sync_plan(fn, T, J, n_cam_idx, max_lag);
    MVP_REQUIRE(!std::isnan(min_conf), "%s: min_conf is NaN", fn);
    MVP_REQUIRE(std::isfinite(trunc_px) && trunc_px > 0.f, "%s: trunc_px=%g (finite, > 0)", fn, (double)trunc_px);
    MVP_REQUIRE(workspace_bytes >= pl.bytes, "%s: workspace_bytes=%lld < %lld needed (T=%d, J=%d, n_cam_idx=%d, max_lag=%d)",
                fn, (long long)workspace_bytes, (long long)pl.bytes, T, J, n_cam_idx, max_lag);
    MVP_REQUIRE(kpts && cams && workspace && out_sum && out_cnt, "%s: null device pointer", fn);
    const int64_t n = (int64_t)T * J;
    SyncPairs pr{};
    const int np = sync_list_pairs(n_cam_idx, pr);
    char* ws = static_cast<char*>(workspace);
    float2* und = reinterpret_cast<float2*>(ws + pl.off_und);
    double* fmat = reinterpret_cast<double*>(ws + pl.off_f);
    ScanArgs g{};
    g.und = und;
    g.fmat = fmat;
    g.psum = reinterpret_cast<double*>(ws + pl.off_psum);
    g.pcnt = reinterpret_cast<int*>(ws + pl.off_pcnt);
    g.T = T;
    g.J = J;
    g.L = max_lag;
    g.tile = pl.tile;
    g.lag_chunk = pl.lag_chunk;
    g.n_tiles = pl.n_tiles;
    g.n_lags = pl.n_lags;
    g.tau2 = (double)trunc_px * (double)trunc_px;
    g.pr = pr;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(sync_fundamental_kernel, dim3(1), dim3(64), 0, s, cams, ci, pr, np, fmat);
    MVP_HIP(hipGetLastError());
    hipLaunchKernelGGL(sync_undistort_kernel, dim3(tri_grid(fn, n), (unsigned)n_cam_idx), dim3(kBlock), 0, s, kpts, n, V,
                       cams, n_cams, ci, min_conf, und);
    MVP_HIP(hipGetLastError());
    const size_t lds = scan_lds_tiles(pl.tile, pl.lag_chunk, J) + kSyBlock * 12;
    hipLaunchKernelGGL(sync_scan_kernel, dim3((unsigned)pl.n_tiles, (unsigned)pl.n_chunks, (unsigned)np), dim3(kSyBlock),
                       lds, s, g);
    MVP_HIP(hipGetLastError());
    hipLaunchKernelGGL(sync_reduce_kernel, dim3((unsigned)pl.n_lags, (unsigned)np), dim3(kSyBlock), 0, s, g.psum, g.pcnt,
                       pl.n_tiles, pl.n_lags, out_sum, out_cnt);
    MVP_HIP(hipGetLastError());
    MVP_ABI_END
}
