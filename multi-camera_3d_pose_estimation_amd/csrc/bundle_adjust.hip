// Bundle adjustment of the extrinsics over the 2D keypoints (mvp_bundle_adjust_plan / _system /
// mvp_bundle_adjust; the problem is stated in include/mvpose.h; no reference counterpart) for gfx950.
//
// Levenberg-Marquardt on the Schur complement of the points: the 6F camera unknowns are solved from
// S·δc = b with S = blockdiag(U*) − Σ_p Y_p·Y_pᵀ, Y_p = [W_pi·L⁻ᵀ]_i (6F x 3), V*_p = L·Lᵀ.
// Stream-ordered launches, arithmetic in fp64, FMA contraction on (no bit contract):
//
//   prepare    one lane per point: the used views (refine_common.h), the active test at the seed,
//              the f64 copy of the seed, and how many active points observe each view.
//   linearise  workgroups of one wavefront (as many per CU as its LDS holds, at most one per SIMD),
//              grid-stride over the points, one lane per point.  One LDS image serves in turn A
//              beside B and then Y.  A lane walks its views twice in rolled loops (camera records
//              through wave-uniform addresses).  Walk 1: V_p, g_p, the cost, g_c into lane-private
//              LDS columns, and for every free view the images A = J_cᵀ·W̃ and B = J_cᵀ (rows
//              6·slot.., k = (component, lane)); then U += A·Bᵀ by v_mfma_f64_16x16x4_f64 over the
//              upper 16x16 tiles.  The views share the k columns, so only the diagonal 6x6 blocks of
//              the product are U_i; the rest is never read.  (A·Bᵀ and not a square root of W̃: a
//              weight need not be positive.)  Walk 2, after the 3x3 Cholesky: Y_p's rows and, in
//              padding row 6F, the row (L⁻¹·g_p)ᵀ, so that column 6F of Σ Y·Yᵀ is b's correction;
//              Σ Y·Yᵀ by the same MFMA loop, A and B fragments being the same registers.  The
//              accumulators live in registers across the whole grid-stride loop; a workgroup writes
//              ONE partial record.
//   solve      one workgroup: partial records summed in index order (no atomics: the same inputs
//              give the same bits), damping and prior, Cholesky of S, δc, the trial cameras.
//   points     one lane per point: δX_p from δc with W_pi recomputed, the trial point, and the
//              trial cost into per-workgroup partials.
//   decide     one workgroup: accept / reject / stop, lambda, the state's buffer index.
// mvp_bundle_adjust enqueues prepare, max_iter x (linearise, solve, points, decide), a last
// linearise with lambda = 0 for the covariance, and the output kernels; a flag in the device state
// turns the launches after the end into early returns.  Nothing is decided on the host.
//
// Register / LDS figures and the measurements are in DESIGN.md §4.12.
#pragma clang fp contract(off)

#include "refine_common.h"

namespace {

constexpr int kBaWave = 64;
constexpr int kBaCus = 256;         // linearise workgroups: this many times what a CU's LDS holds,
constexpr int kBaLinGrid = 4 * kBaCus;   // at most 4 (one per SIMD)
constexpr int kBaLdsPerCu = 160 * 1024;
constexpr int kBaPtGrid = 1024;     // points-kernel workgroups at most
constexpr int kBaStride = 260;      // LDS image row stride in doubles: 256 + 4, so that a fragment's
                                    // 16 rows x 4 k fall on 2 x 32 distinct 8-byte banks
constexpr int kBaColB = 128;        // the B image's first column (A: 0..127, Y: 0..191)

// LDS bytes of a linearise workgroup with F free views: the image, g_c, the final reduction.
__host__ __device__ constexpr int ba_lin_lds(int F) {
    return (16 * ((6 * F + 16) / 16) * kBaStride + 6 * F * kBaWave + 4 * kBaWave) * 8;
}
constexpr int kBaMaxRows = 48;
constexpr int kBaMaxN6 = 42;
constexpr int kBaSolveBlock = 1024;   // the one-workgroup kernels that sum the partial records

typedef double ba_v4d __attribute__((ext_vector_type(4)));

__host__ __device__ constexpr int ba_tiles(int nr) { return nr * (nr + 1) / 2; }
__host__ __device__ constexpr int ba_rec_doubles(int nr) { return 2 * ba_tiles(nr) * 256 + 16 * nr + 4; }

struct BaState {
    double lambda, f_cur, f_seed, pad0;
    int cur, done, status, trials, accepted, reject, pad1, pad2;
    int view_cnt[8];
    double dc[kBaMaxRows];
    double cam[2][kMaxCams][MVP_CAM_DOUBLES];   // [cur ^ 0 = state, cur ^ 1 = trial][camera]
};

struct BaViews {
    ViewList vl;         // the listed cameras
    unsigned free_mask;  // bit j: view j is optimised
    int F;
};

struct BaPlan {
    int F, nr, rec, lin_grid, pt_grid;
    int64_t off_state, off_used, off_x, off_part, off_tpart, bytes;
};

inline int64_t ba_align256(int64_t b) { return (b + 255) & ~(int64_t)255; }

inline BaPlan ba_plan(const char* fn, int64_t n, int nv, unsigned free_mask) {
    MVP_REQUIRE(n >= 1 && n < (1LL << 31), "%s: n_points=%lld (1..2^31-1)", fn, (long long)n);
    MVP_REQUIRE(nv >= 2 && nv <= kMaxCams, "%s: n_cam_idx=%d (2..%d)", fn, nv, kMaxCams);
    MVP_REQUIRE(free_mask != 0 && (free_mask >> nv) == 0, "%s: free_mask=0x%x must be non-zero with no bit at or above n_cam_idx=%d",
                fn, free_mask, nv);
    BaPlan pl;
    pl.F = __builtin_popcount(free_mask);
    MVP_REQUIRE(pl.F <= nv - 1, "%s: free_mask=0x%x frees every listed view; at least one must stay fixed", fn, free_mask);
    pl.nr = (6 * pl.F + 1 + 15) / 16;
    pl.rec = ba_rec_doubles(pl.nr);
    const int per_cu = std::max(1, std::min(4, kBaLdsPerCu / ba_lin_lds(pl.F)));
    pl.lin_grid = (int)std::min<int64_t>((n + kBaWave - 1) / kBaWave, (int64_t)per_cu * kBaCus);
    pl.pt_grid = (int)std::min<int64_t>((n + kBlock - 1) / kBlock, kBaPtGrid);
    int64_t b = 0;
    pl.off_state = b;
    b = ba_align256(b + (int64_t)sizeof(BaState));
    pl.off_used = b;
    b = ba_align256(b + n);
    pl.off_x = b;
    b = ba_align256(b + 2 * n * 3 * 8);
    pl.off_part = b;
    b = ba_align256(b + (int64_t)kBaLinGrid * pl.rec * 8);
    pl.off_tpart = b;
    b = ba_align256(b + (int64_t)kBaPtGrid * 8);
    pl.bytes = b;
    return pl;
}

// ------------------------------------------------------------------------------- prepare
__global__ __launch_bounds__(kBlock) void ba_prepare_kernel(ReprojObs a, const double* __restrict__ cams, BaViews vw,
                                                            const float* __restrict__ xyz0,
                                                            uint8_t* __restrict__ used_out, double* __restrict__ x0,
                                                            int* __restrict__ view_cnt) {
#pragma clang fp contract(fast)
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool valid = p < a.n;
    const int64_t pc = valid ? p : 0;
    const unsigned allowed = reproj_allowed(a, pc);
    const float s0 = xyz0[3 * pc + 0], s1 = xyz0[3 * pc + 1], s2 = xyz0[3 * pc + 2];
    const double X[3] = {(double)s0, (double)s1, (double)s2};
    unsigned used = 0;
    bool front = true;
#pragma unroll 1
    for (int j = 0; j < vw.vl.nv; j++) {
        const int col = vw.vl.col(j);
        double zx, zy, wxx, wxy, wyy;
        const bool ok = reproj_observe(a, pc, col, (allowed >> j) & 1u, zx, zy, wxx, wxy, wyy);
        const RefineCam c = refine_cam(cams + col * MVP_CAM_DOUBLES);
        const double Pz = c.R[6] * X[0] + c.R[7] * X[1] + c.R[8] * X[2] + c.T[2];
        used |= (ok ? 1u : 0u) << j;
        front = front && (!ok || Pz > 0);
    }
    const bool active = valid && __popc(used) >= 2 && isfinite(s0) && isfinite(s1) && isfinite(s2) && front;
    used = active ? used : 0u;
    if (valid) {
        used_out[p] = (uint8_t)used;
        if (x0) {
            x0[3 * p + 0] = X[0];
            x0[3 * p + 1] = X[1];
            x0[3 * p + 2] = X[2];
        }
    }
    if (view_cnt) {
#pragma unroll 1
        for (int j = 0; j < vw.vl.nv; j++) {
            const unsigned long long b = __ballot((used >> j) & 1u);
            if ((threadIdx.x & 63) == 0 && b) atomicAdd(view_cnt + j, (int)__builtin_popcountll(b));
        }
    }
}

// ------------------------------------------------------------------------------- linearise
struct BaLinArgs {
    ReprojObs obs;       // hub: the Huber delta
    BaViews vw;
    const BaState* st;        // null: mvp_bundle_adjust_system (cams, xyz32 and lambda below)
    const double* cams;
    const float* xyz32;
    const double* x64;        // [2][n][3] with st
    const uint8_t* used;
    double* part;             // [gridDim][rec]
    double lambda;
    int final_pass;           // with st: run although done, with lambda = 0
};

// acc[tile] += A_img(rows of tile ti)·B_img(rows of tile tj)ᵀ over k = 0..4·ksteps−1, upper tiles.
// Fragments of v_mfma_f64_16x16x4_f64: A[lane & 15][k = lane >> 4], B[k = lane >> 4][lane & 15].
template <int NR, bool SAME>
__device__ __forceinline__ void ba_mfma(const double* a_img, int sa, const double* b_img, int sb, int ksteps,
                                        ba_v4d (&acc)[ba_tiles(NR)], int lane) {
    const int r = lane & 15, kq = lane >> 4;
#pragma unroll 2
    for (int ks = 0; ks < ksteps; ks++) {
        double fa[NR], fb[NR];
#pragma unroll
        for (int t = 0; t < NR; t++) {
            fa[t] = a_img[(16 * t + r) * sa + 4 * ks + kq];
            fb[t] = SAME ? fa[t] : b_img[(16 * t + r) * sb + 4 * ks + kq];
        }
        int idx = 0;
#pragma unroll
        for (int ti = 0; ti < NR; ti++)
#pragma unroll
            for (int tj = ti; tj < NR; tj++, idx++)
                acc[idx] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[ti], fb[tj], acc[idx], 0, 0, 0);
    }
}

template <int F>
__global__ __launch_bounds__(kBaWave) void ba_linearise_kernel(BaLinArgs g) {
#pragma clang fp contract(fast)
    constexpr int n6 = 6 * F, NR = (n6 + 16) / 16, NT = ba_tiles(NR), ROWS = 16 * NR;
    // one image, three tenants in turn: A (columns 0..127) beside B (128..255), then Y (0..191)
    __shared__ double s_y[ROWS * kBaStride];
    __shared__ double s_gc[n6 * kBaWave];       // g_c, [row][lane]
    double* const s_b = s_y + kBaColB;
    __shared__ double s_red[4][kBaWave];
    const int lane = threadIdx.x;
    if (g.st && g.st->done && !g.final_pass) return;
    const int cur = g.st ? g.st->cur : 0;
    const double* __restrict__ cam_base = g.st ? &g.st->cam[cur][0][0] : g.cams;
    const double lambda = g.st ? (g.final_pass ? 0.0 : g.st->lambda) : g.lambda;
    const double damp = 1.0 + lambda;
    const int64_t n = g.obs.n;
    for (int e = lane; e < ROWS * kBaStride; e += kBaWave) s_y[e] = 0.0;
    for (int e = lane; e < n6 * kBaWave; e += kBaWave) s_gc[e] = 0.0;
    __syncthreads();
    ba_v4d accY[NT], accU[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) accY[t] = accU[t] = ba_v4d{0.0, 0.0, 0.0, 0.0};
    double cost = 0.0;
    int n_active = 0, n_used = 0, n_bad = 0;

#pragma unroll 1
    for (int64_t base = (int64_t)blockIdx.x * kBaWave; base < n; base += (int64_t)gridDim.x * kBaWave) {
        const int64_t p = base + lane;
        const int64_t pc = p < n ? p : 0;
        const unsigned used = p < n ? (unsigned)g.used[pc] : 0u;
        const bool active = used != 0u;
        double X[3];
        if (g.st) {
            const double* xp = g.x64 + ((int64_t)cur * n + pc) * 3;
            X[0] = xp[0], X[1] = xp[1], X[2] = xp[2];
        } else {
            X[0] = (double)g.xyz32[3 * pc + 0], X[1] = (double)g.xyz32[3 * pc + 1], X[2] = (double)g.xyz32[3 * pc + 2];
        }
        // walk 1: V_p, g_p, cost, g_c and the A / B images
        double Vp[6] = {0, 0, 0, 0, 0, 0}, gp[3] = {0, 0, 0};
#pragma unroll 1
        for (int j = 0; j < g.vw.vl.nv; j++) {
            const int col = g.vw.vl.col(j);
            const bool u = (used >> j) & 1u;
            double zx, zy, wxx, wxy, wyy;
            reproj_observe(g.obs, pc, col, u, zx, zy, wxx, wxy, wyy);
            const RefineCam c = refine_cam(cam_base + col * MVP_CAM_DOUBLES);
            const ReprojView o = reproj_view(c, X, zx, zy, wxx, wxy, wyy, g.obs.hub);
            double jx0[3], jx1[3], jc0[6], jc1[6];
            reproj_jx_jc(c, o.w, jx0, jx1, jc0, jc1);
            reproj_add_normal(jx0, jx1, o.w00, o.w01, o.w11, o.r0, o.r1, u, gp, Vp);
            cost += u ? o.rho : 0.0;
            n_used += u ? 1 : 0;
            if ((g.vw.free_mask >> j) & 1u) {   // wave-uniform
                const int row0 = 6 * __builtin_popcount(g.vw.free_mask & ((1u << j) - 1u));
#pragma unroll
                for (int k = 0; k < 6; k++) {
                    const double a0 = jc0[k] * o.w00 + jc1[k] * o.w01, a1 = jc0[k] * o.w01 + jc1[k] * o.w11;
                    s_y[(row0 + k) * kBaStride + lane] = u ? a0 : 0.0;
                    s_y[(row0 + k) * kBaStride + kBaWave + lane] = u ? a1 : 0.0;
                    s_b[(row0 + k) * kBaStride + lane] = u ? jc0[k] : 0.0;
                    s_b[(row0 + k) * kBaStride + kBaWave + lane] = u ? jc1[k] : 0.0;
                    s_gc[(row0 + k) * kBaWave + lane] += u ? a0 * o.r0 + a1 * o.r1 : 0.0;
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 4; c++) s_y[n6 * kBaStride + c * kBaWave + lane] = 0.0;   // row 6F held (L⁻¹·g_p)ᵀ
        n_active += active ? 1 : 0;
        __syncthreads();
        ba_mfma<NR, false>(s_y, kBaStride, s_b, kBaStride, 2 * kBaWave / 4, accU, lane);
        __syncthreads();

        // V* = L·Lᵀ; z = L⁻¹·g_p
        const double A[6] = {Vp[0] * damp, Vp[1], Vp[2], Vp[3] * damp, Vp[4], Vp[5] * damp};
        double L[6];
        const bool pd = chol3(A, L);
        const bool good = active && pd;
        const double fill = active ? __builtin_nan("") : 0.0;   // a failed pivot shows in S and b
        n_bad += (active && !pd) ? 1 : 0;
        const double i0 = 1.0 / L[0], i3 = 1.0 / L[3], i5 = 1.0 / L[5];
        {
            const double z0 = gp[0] * i0;
            const double z1 = (gp[1] - L[1] * z0) * i3;
            const double z2 = (gp[2] - L[2] * z0 - L[4] * z1) * i5;
            s_y[n6 * kBaStride + lane] = good ? z0 : fill;
            s_y[n6 * kBaStride + kBaWave + lane] = good ? z1 : fill;
            s_y[n6 * kBaStride + 2 * kBaWave + lane] = good ? z2 : fill;
        }
        // walk 2: the free views' rows of Y_p = W_pi·L⁻ᵀ
#pragma unroll 1
        for (int j = 0; j < g.vw.vl.nv; j++) {
            if (!((g.vw.free_mask >> j) & 1u)) continue;
            const int row0 = 6 * __builtin_popcount(g.vw.free_mask & ((1u << j) - 1u));
            const int col = g.vw.vl.col(j);
            const bool u = (used >> j) & 1u;
            double zx, zy, wxx, wxy, wyy;
            reproj_observe(g.obs, pc, col, u, zx, zy, wxx, wxy, wyy);
            const RefineCam c = refine_cam(cam_base + col * MVP_CAM_DOUBLES);
            const ReprojView o = reproj_view(c, X, zx, zy, wxx, wxy, wyy, g.obs.hub);
            double jx0[3], jx1[3], jc0[6], jc1[6];
            reproj_jx_jc(c, o.w, jx0, jx1, jc0, jc1);
#pragma unroll
            for (int k = 0; k < 6; k++) {
                const double a0 = jc0[k] * o.w00 + jc1[k] * o.w01, a1 = jc0[k] * o.w01 + jc1[k] * o.w11;
                const double w0 = a0 * jx0[0] + a1 * jx1[0];
                const double w1 = a0 * jx0[1] + a1 * jx1[1];
                const double w2 = a0 * jx0[2] + a1 * jx1[2];
                const double y0 = w0 * i0;
                const double y1 = (w1 - L[1] * y0) * i3;
                const double y2 = (w2 - L[2] * y0 - L[4] * y1) * i5;
                s_y[(row0 + k) * kBaStride + lane] = u ? (pd ? y0 : fill) : 0.0;
                s_y[(row0 + k) * kBaStride + kBaWave + lane] = u ? (pd ? y1 : fill) : 0.0;
                s_y[(row0 + k) * kBaStride + 2 * kBaWave + lane] = u ? (pd ? y2 : fill) : 0.0;
            }
        }
        __syncthreads();
        ba_mfma<NR, true>(s_y, kBaStride, s_y, kBaStride, 3 * kBaWave / 4, accY, lane);
        __syncthreads();
    }

    // the workgroup's partial record: Y tiles, U tiles, g_c, {cost, active points, used views, bad pivots}
    double* __restrict__ rec = g.part + (int64_t)blockIdx.x * ba_rec_doubles(NR);
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int e = ((lane >> 4) + 4 * r) * 16 + (lane & 15);
            rec[t * 256 + e] = accY[t][r];
            rec[(NT + t) * 256 + e] = accU[t][r];
        }
    s_red[0][lane] = cost;
    s_red[1][lane] = (double)n_active;
    s_red[2][lane] = (double)n_used;
    s_red[3][lane] = (double)n_bad;
    __syncthreads();
    if (lane < ROWS) {
        double s = 0.0;
        if (lane < n6)
            for (int l = 0; l < kBaWave; l++) s += s_gc[lane * kBaWave + l];
        rec[2 * NT * 256 + lane] = s;
    }
    if (lane < 4) {
        double s = 0.0;
        for (int l = 0; l < kBaWave; l++) s += s_red[lane][l];
        rec[2 * NT * 256 + ROWS + lane] = s;
    }
}

// ------------------------------------------------------------------------------- reduced system
// Sum of the partial records in index order into s_sum[rec] (all threads; ends on a barrier).
__device__ __forceinline__ void ba_sum_partials(const double* __restrict__ part, int n_part, int rec, double* s_sum) {
    for (int e = threadIdx.x; e < rec; e += blockDim.x) {
        double s = 0.0;
#pragma unroll 8   // eight loads in flight; the additions stay in index order
        for (int w = 0; w < n_part; w++) s += part[(int64_t)w * rec + e];
        s_sum[e] = s;
    }
    __syncthreads();
}

// Element (a, b), a <= b, of the summed upper tiles that start at s_tiles.
__device__ __forceinline__ double ba_tile_at(const double* s_tiles, int nr, int a, int b) {
    const int ti = a >> 4, tj = b >> 4;
    const int idx = ti * nr - ti * (ti - 1) / 2 + (tj - ti);
    return s_tiles[idx * 256 + (a & 15) * 16 + (b & 15)];
}

// S (n6 x n6, row stride ld, full symmetric) and b from the summed record; tdiff: T_i − T_i⁰ of the
// free views (3 per slot) or null.  All threads; ends on a barrier.
__device__ __forceinline__ void ba_build_system(const double* s_sum, int nr, int F, double lambda, double inv_s2,
                                                const double* tdiff, double* S, int ld, double* b) {
#pragma clang fp contract(fast)
    const int n6 = 6 * F, nt = ba_tiles(nr);
    for (int e = threadIdx.x; e < n6 * n6; e += blockDim.x) {
        const int a = e / n6, c = e - a * n6;
        const int lo = a < c ? a : c, hi = a < c ? c : a;
        double u = (lo / 6 == hi / 6) ? ba_tile_at(s_sum + nt * 256, nr, lo, hi) : 0.0;
        if (a == c) u = u + lambda * u + ((a % 6) >= 3 ? inv_s2 : 0.0);
        S[a * ld + c] = u - ba_tile_at(s_sum, nr, lo, hi);
    }
    for (int a = threadIdx.x; a < n6; a += blockDim.x) {
        double gc = s_sum[2 * nt * 256 + a];
        if (tdiff && (a % 6) >= 3) gc += tdiff[3 * (a / 6) + (a % 6) - 3] * inv_s2;
        b[a] = ba_tile_at(s_sum, nr, a, n6) - gc;
    }
    __syncthreads();
}

// In-place Cholesky of the n x n matrix S (row stride ld) by one thread; false on a pivot that is
// not > 0.  The lower triangle holds L.
__device__ bool ba_chol(double* S, int ld, int n) {
#pragma clang fp contract(fast)
    bool ok = true;
    for (int j = 0; j < n; j++) {
        double d = S[j * ld + j];
        for (int k = 0; k < j; k++) d -= S[j * ld + k] * S[j * ld + k];
        ok = ok && (d > 0);
        const double l = sqrt(d), il = 1.0 / l;
        S[j * ld + j] = l;
        for (int i = j + 1; i < n; i++) {
            double v = S[i * ld + j];
            for (int k = 0; k < j; k++) v -= S[i * ld + k] * S[j * ld + k];
            S[i * ld + j] = v * il;
        }
    }
    return ok;
}

// x <- (L·Lᵀ)⁻¹ x by one thread; x's elements are xs apart.
__device__ void ba_chol_solve(const double* L, int ld, int n, double* x, int xs) {
#pragma clang fp contract(fast)
    for (int i = 0; i < n; i++) {
        double v = x[i * xs];
        for (int k = 0; k < i; k++) v -= L[i * ld + k] * x[k * xs];
        x[i * xs] = v / L[i * ld + i];
    }
    for (int i = n - 1; i >= 0; i--) {
        double v = x[i * xs];
        for (int k = i + 1; k < n; k++) v -= L[k * ld + i] * x[k * xs];
        x[i * xs] = v / L[i * ld + i];
    }
}

__global__ __launch_bounds__(kBaSolveBlock) void ba_assemble_kernel(const double* __restrict__ part, int n_part, int nr, int F,
                                                             double lambda, double inv_s2, double* __restrict__ out_S,
                                                             double* __restrict__ out_b, double* __restrict__ out_cost,
                                                             int64_t* __restrict__ out_counts) {
    __shared__ double s_sum[ba_rec_doubles(3)];
    const int nt = ba_tiles(nr);
    ba_sum_partials(part, n_part, ba_rec_doubles(nr), s_sum);
    ba_build_system(s_sum, nr, F, lambda, inv_s2, nullptr, out_S, 6 * F, out_b);
    if (threadIdx.x == 0) {
        const double* sc = s_sum + 2 * nt * 256 + 16 * nr;
        out_cost[0] = sc[0];
        out_counts[0] = (int64_t)sc[1];
        out_counts[1] = (int64_t)sc[2];
    }
}

// The prior's cost ½·Σ|T_i − T_i⁰|²/σ² over the free views, cam: [camera][MVP_CAM_DOUBLES].
__device__ __forceinline__ double ba_prior_cost(const double* cam, const double* __restrict__ cams0, BaViews vw,
                                                double inv_s2) {
#pragma clang fp contract(fast)
    double s = 0.0;
    for (int j = 0; j < vw.vl.nv; j++) {
        if (!((vw.free_mask >> j) & 1u)) continue;
        const int col = vw.vl.col(j);
        for (int k = 0; k < 3; k++) {
            const double d = cam[col * MVP_CAM_DOUBLES + 23 + k] - cams0[col * MVP_CAM_DOUBLES + 23 + k];
            s += d * d;
        }
    }
    return 0.5 * s * inv_s2;
}

// ------------------------------------------------------------------------------- init / solve / decide
__global__ void ba_init_kernel(BaState* st, const double* __restrict__ cams, int n_cams, BaViews vw) {
    for (int e = threadIdx.x; e < n_cams * MVP_CAM_DOUBLES; e += blockDim.x) {
        (&st->cam[0][0][0])[e] = cams[e];
        (&st->cam[1][0][0])[e] = cams[e];
    }
    if (threadIdx.x == 0) {
        bool starved = false;
        for (int j = 0; j < vw.vl.nv; j++) starved = starved || (((vw.free_mask >> j) & 1u) && st->view_cnt[j] < 3);
        st->lambda = 1e-3;
        st->f_cur = st->f_seed = 0.0;
        st->cur = 0;
        st->done = starved ? 1 : 0;
        st->status = starved ? 3 : 1;
        st->trials = st->accepted = st->reject = 0;
    }
}

__global__ __launch_bounds__(kBaSolveBlock) void ba_solve_kernel(BaState* st, const double* __restrict__ part, int n_part,
                                                          int nr, BaViews vw, const double* __restrict__ cams0,
                                                          double inv_s2) {
#pragma clang fp contract(fast)
    __shared__ double s_sum[ba_rec_doubles(3)];
    __shared__ double s_S[kBaMaxN6 * (kBaMaxN6 + 1)], s_bv[kBaMaxRows], s_td[3 * kMaxCams];
    if (st->done) return;
    const int F = vw.F, n6 = 6 * F, nt = ba_tiles(nr), ld = kBaMaxN6 + 1;
    const int cur = st->cur;
    const double* camc = &st->cam[cur][0][0];
    double* camt = &st->cam[cur ^ 1][0][0];
    ba_sum_partials(part, n_part, ba_rec_doubles(nr), s_sum);
    if (threadIdx.x == 0) {
        int slot = 0;
        for (int j = 0; j < vw.vl.nv; j++) {
            if (!((vw.free_mask >> j) & 1u)) continue;
            const int col = vw.vl.col(j);
            for (int k = 0; k < 3; k++)
                s_td[3 * slot + k] = camc[col * MVP_CAM_DOUBLES + 23 + k] - cams0[col * MVP_CAM_DOUBLES + 23 + k];
            slot++;
        }
    }
    __syncthreads();
    ba_build_system(s_sum, nr, F, st->lambda, inv_s2, s_td, s_S, ld, s_bv);
    if (threadIdx.x != 0) return;
    const double* sc = s_sum + 2 * nt * 256 + 16 * nr;
    if (st->trials == 0) {
        const double f0 = sc[0] + ba_prior_cost(camc, cams0, vw, inv_s2);
        st->f_cur = f0;
        st->f_seed = f0;
    }
    bool ok = !(sc[3] > 0);
    ok = ba_chol(s_S, ld, n6) && ok;
    ba_chol_solve(s_S, ld, n6, s_bv, 1);
    for (int a = 0; a < n6; a++) ok = ok && isfinite(s_bv[a]);
    st->reject = ok ? 0 : 1;
    for (int a = 0; a < kBaMaxRows; a++) st->dc[a] = (ok && a < n6) ? s_bv[a] : 0.0;
    // trial cameras: R <- exp([δw]×)·R, T <- T + δu
    int slot = 0;
    for (int j = 0; j < vw.vl.nv; j++) {
        if (!((vw.free_mask >> j) & 1u)) continue;
        const int col = vw.vl.col(j);
        const double* dc = st->dc + 6 * slot;
        const double* Rc = camc + col * MVP_CAM_DOUBLES + 14;
        double* Rt = camt + col * MVP_CAM_DOUBLES + 14;
        const double wx = dc[0], wy = dc[1], wz = dc[2];
        const double th2 = wx * wx + wy * wy + wz * wz, th = sqrt(th2);
        const bool small = th < 1e-12;
        const double ka = small ? 1.0 : sin(th) / th, kb = small ? 0.0 : (1.0 - cos(th)) / th2;
        const double K1[9] = {0, -wz, wy, wz, 0, -wx, -wy, wx, 0};
        double E[9];
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) {
                double k2 = 0.0;
                for (int m = 0; m < 3; m++) k2 += K1[3 * r + m] * K1[3 * m + c];
                E[3 * r + c] = (r == c ? 1.0 : 0.0) + ka * K1[3 * r + c] + kb * k2;
            }
        double Rn[9];
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) Rn[3 * r + c] = E[3 * r] * Rc[c] + E[3 * r + 1] * Rc[3 + c] + E[3 * r + 2] * Rc[6 + c];
        for (int k = 0; k < 9; k++) Rt[k] = Rn[k];
        for (int k = 0; k < 3; k++) camt[col * MVP_CAM_DOUBLES + 23 + k] = camc[col * MVP_CAM_DOUBLES + 23 + k] + dc[3 + k];
        slot++;
    }
}

struct BaPtArgs {
    ReprojObs obs;       // hub: the Huber delta
    BaViews vw;
    const BaState* st;
    double* x64;
    const uint8_t* used;
    double* tpart;   // [gridDim]
};

__global__ __launch_bounds__(kBlock) void ba_points_kernel(BaPtArgs g) {
#pragma clang fp contract(fast)
    __shared__ double s_red[kBlock];
    if (g.st->done) return;
    const int cur = g.st->cur;
    const double* __restrict__ camc = &g.st->cam[cur][0][0];
    const double* __restrict__ camt = &g.st->cam[cur ^ 1][0][0];
    const double* __restrict__ dcv = g.st->dc;
    const double damp = 1.0 + g.st->lambda;
    const int64_t n = g.obs.n;
    const double dinf = (double)INFINITY;
    double cost = 0.0;
#pragma unroll 1
    for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < n; p += (int64_t)gridDim.x * kBlock) {
        const unsigned used = g.used[p];
        const double* xp = g.x64 + ((int64_t)cur * n + p) * 3;
        double* xt = g.x64 + ((int64_t)(cur ^ 1) * n + p) * 3;
        const double X[3] = {xp[0], xp[1], xp[2]};
        if (used == 0u) {
            xt[0] = X[0], xt[1] = X[1], xt[2] = X[2];
            continue;
        }
        // rhs = g_p + Σ W_piᵀ·δc_i = Σ J_Xᵀ·W̃·(r + J_c·δc_i)
        double Vp[6] = {0, 0, 0, 0, 0, 0}, rhs[3] = {0, 0, 0};
#pragma unroll 1
        for (int j = 0; j < g.vw.vl.nv; j++) {
            const int col = g.vw.vl.col(j);
            const bool u = (used >> j) & 1u;
            double zx, zy, wxx, wxy, wyy;
            reproj_observe(g.obs, p, col, u, zx, zy, wxx, wxy, wyy);
            const RefineCam c = refine_cam(camc + col * MVP_CAM_DOUBLES);
            const ReprojView o = reproj_view(c, X, zx, zy, wxx, wxy, wyy, g.obs.hub);
            double jx0[3], jx1[3], jc0[6], jc1[6];
            reproj_jx_jc(c, o.w, jx0, jx1, jc0, jc1);
            double t0 = o.r0, t1 = o.r1;
            if ((g.vw.free_mask >> j) & 1u) {
                const double* dc = dcv + 6 * __builtin_popcount(g.vw.free_mask & ((1u << j) - 1u));
#pragma unroll
                for (int k = 0; k < 6; k++) {
                    t0 += jc0[k] * dc[k];
                    t1 += jc1[k] * dc[k];
                }
            }
            reproj_add_normal(jx0, jx1, o.w00, o.w01, o.w11, -t0, -t1, u, rhs, Vp);   // rhs −= J_Xᵀ·W̃·t, bit for bit
        }
        const double A[6] = {Vp[0] * damp, Vp[1], Vp[2], Vp[3] * damp, Vp[4], Vp[5] * damp};
        double L[6], dX[3];
        chol3(A, L);   // a failed pivot was counted by the linearise kernel: the trial is rejected
        chol3_solve(L, rhs, dX);
        const double Xn[3] = {X[0] + dX[0], X[1] + dX[1], X[2] + dX[2]};
        xt[0] = Xn[0], xt[1] = Xn[1], xt[2] = Xn[2];
        // the trial cost
        double fp = 0.0;
        bool front = true;
#pragma unroll 1
        for (int j = 0; j < g.vw.vl.nv; j++) {
            const int col = g.vw.vl.col(j);
            const bool u = (used >> j) & 1u;
            double zx, zy, wxx, wxy, wyy;
            reproj_observe(g.obs, p, col, u, zx, zy, wxx, wxy, wyy);
            const RefineCam c = refine_cam(camt + col * MVP_CAM_DOUBLES);
            const ReprojView o = reproj_view(c, Xn, zx, zy, wxx, wxy, wyy, g.obs.hub);
            fp += u ? o.rho : 0.0;
            front = front && (!u || o.front);
        }
        cost += front ? fp : dinf;
    }
    s_red[threadIdx.x] = cost;
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) s_red[threadIdx.x] += s_red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) g.tpart[blockIdx.x] = s_red[0];
}

__global__ __launch_bounds__(kBlock) void ba_decide_kernel(BaState* st, const double* __restrict__ tpart, int n_part,
                                                           BaViews vw, const double* __restrict__ cams0, double inv_s2,
                                                           double tol, int max_iter) {
#pragma clang fp contract(fast)
    __shared__ double s_red[kBlock];
    if (st->done) return;
    double s = 0.0;
    for (int e = threadIdx.x; e < n_part; e += kBlock) s += tpart[e];
    s_red[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x != 0) return;
    double ft = 0.0;
    for (int e = 0; e < kBlock; e++) ft += s_red[e];
    const int cur = st->cur;
    ft += ba_prior_cost(&st->cam[cur ^ 1][0][0], cams0, vw, inv_s2);
    const double f = st->f_cur;
    const bool accept = !st->reject && isfinite(ft) && ft <= f;
    st->trials += 1;
    bool done = false;
    if (accept) {
        const bool conv = (f - ft) <= tol * f;
        st->cur = cur ^ 1;
        st->f_cur = ft;
        st->lambda = fmax(st->lambda * 0.1, 1e-12);
        st->accepted += 1;
        if (conv) done = true, st->status = 0;
        // the other buffer becomes the trial buffer: the fixed cameras there are the input's already
    } else {
        st->lambda = st->lambda * 10.0;
        if (st->lambda > 1e12) done = true, st->status = 2;
    }
    if (!done && st->trials >= max_iter) done = true, st->status = 1;
    st->done = done ? 1 : 0;
}

// ------------------------------------------------------------------------------- outputs
__global__ __launch_bounds__(kBaSolveBlock) void ba_final_kernel(BaState* st, const double* __restrict__ part, int n_part,
                                                          int nr, BaViews vw, const double* __restrict__ cams0,
                                                          int n_cams, double inv_s2, double* __restrict__ out_cams,
                                                          double* __restrict__ out_cov, double* __restrict__ out_info) {
#pragma clang fp contract(off)
    __shared__ double s_sum[ba_rec_doubles(3)];
    __shared__ double s_S[kBaMaxN6 * (kBaMaxN6 + 1)], s_bv[kBaMaxRows], s_td[3 * kMaxCams];
    __shared__ double s_inv[kBaMaxN6 * (kBaMaxN6 + 1)];
    __shared__ int s_ok;
    const int F = vw.F, n6 = 6 * F, nt = ba_tiles(nr), ld = kBaMaxN6 + 1;
    const int cur = st->cur;
    const double* camc = &st->cam[cur][0][0];
    ba_sum_partials(part, n_part, ba_rec_doubles(nr), s_sum);
    for (int e = threadIdx.x; e < 3 * kMaxCams; e += blockDim.x) s_td[e] = 0.0;   // b is not read here
    __syncthreads();
    ba_build_system(s_sum, nr, F, 0.0, inv_s2, s_td, s_S, ld, s_bv);
    const double* sc = s_sum + 2 * nt * 256 + 16 * nr;
    if (threadIdx.x == 0) {
        s_ok = (ba_chol(s_S, ld, n6) && !(sc[3] > 0)) ? 1 : 0;
        double f_seed = st->f_seed, f_final = st->f_cur;
        if (st->trials == 0) f_seed = f_final = sc[0] + ba_prior_cost(camc, cams0, vw, inv_s2);
        out_info[0] = f_seed;
        out_info[1] = f_final;
        out_info[2] = (double)st->trials;
        out_info[3] = (double)st->accepted;
        out_info[4] = (double)st->status;
        out_info[5] = st->lambda;
        out_info[6] = sc[1];
        out_info[7] = sc[2];
    }
    __syncthreads();
    if (out_cov && (int)threadIdx.x < n6) {
        // column threadIdx.x of S⁻¹
        double* x = s_inv + threadIdx.x;
        for (int a = 0; a < n6; a++) x[a * ld] = a == (int)threadIdx.x ? 1.0 : 0.0;
        ba_chol_solve(s_S, ld, n6, x, ld);
        for (int a = 0; a < n6; a++) out_cov[a * n6 + threadIdx.x] = s_ok ? x[a * ld] : __builtin_nan("");
    }
    // the cameras: the input's records, the free views' R, T from the state, P = K·[R|T] by the
    // loops of mvp_camera_pack (no contraction)
    for (int e = threadIdx.x; e < n_cams * MVP_CAM_DOUBLES; e += blockDim.x) out_cams[e] = cams0[e];
    __syncthreads();
    if ((int)threadIdx.x < vw.vl.nv && ((vw.free_mask >> threadIdx.x) & 1u)) {
        const int col = vw.vl.col(threadIdx.x);
        double* o = out_cams + col * MVP_CAM_DOUBLES;
        const double* c = camc + col * MVP_CAM_DOUBLES;
        for (int k = 14; k < 26; k++) o[k] = c[k];
        double Rt[3][4];
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) Rt[i][j] = c[14 + i * 3 + j];
            Rt[i][3] = c[23 + i];
        }
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 4; j++) {
                double acc = c[i * 3 + 0] * Rt[0][j];
                acc += c[i * 3 + 1] * Rt[1][j];
                acc += c[i * 3 + 2] * Rt[2][j];
                o[26 + i * 4 + j] = acc;
            }
    }
}

__global__ __launch_bounds__(kBlock) void ba_output_kernel(const BaState* st, const double* __restrict__ x64,
                                                           const uint8_t* __restrict__ used,
                                                           const float* __restrict__ xyz0, int64_t n,
                                                           float* __restrict__ out_xyz, uint8_t* __restrict__ out_status) {
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    const bool active = used[p] != 0;
    const double* xp = x64 + ((int64_t)st->cur * n + p) * 3;
#pragma unroll
    for (int k = 0; k < 3; k++) out_xyz[3 * p + k] = active ? (float)xp[k] : xyz0[3 * p + k];
    if (out_status) out_status[p] = active ? (uint8_t)0 : (uint8_t)0x80;
}

// ------------------------------------------------------------------------------- host side
struct BaCall {
    BaPlan pl;
    BaViews vw;
    ReprojObs obs;
    double inv_s2;
};

inline BaCall ba_parse(const char* fn, const float* kpts, int64_t n, int V, int n_cams, const int* cam_idx, int nv,
                       unsigned free_mask, const uint8_t* mask, int weights, const double* gauss, int J, float min_conf,
                       float cov_floor, double huber_delta, double sigma, int64_t workspace_bytes) {
    BaCall c{};
    const CamIdx ci = tri_parse_args(fn, n, V, n_cams, cam_idx, nv);
    c.pl = ba_plan(fn, n, nv, free_mask);
    c.obs = reproj_parse_obs(fn, kpts, n, V, mask, weights, gauss, J, min_conf, cov_floor, huber_delta);
    MVP_REQUIRE(!std::isnan(sigma), "%s: trans_prior_sigma is NaN", fn);
    MVP_REQUIRE(workspace_bytes >= c.pl.bytes, "%s: workspace_bytes=%lld < %lld needed (n_points=%lld, free_mask=0x%x)", fn,
                (long long)workspace_bytes, (long long)c.pl.bytes, (long long)n, free_mask);
    c.vw = BaViews{view_list(ci, nv), free_mask, c.pl.F};
    c.inv_s2 = sigma > 0 ? 1.0 / (sigma * sigma) : 0.0;
    return c;
}

inline void ba_launch_linearise(const BaCall& c, const BaLinArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)c.pl.lin_grid), block(kBaWave);
    switch (c.pl.F) {
        case 1: hipLaunchKernelGGL(ba_linearise_kernel<1>, grid, block, 0, s, a); break;
        case 2: hipLaunchKernelGGL(ba_linearise_kernel<2>, grid, block, 0, s, a); break;
        case 3: hipLaunchKernelGGL(ba_linearise_kernel<3>, grid, block, 0, s, a); break;
        case 4: hipLaunchKernelGGL(ba_linearise_kernel<4>, grid, block, 0, s, a); break;
        case 5: hipLaunchKernelGGL(ba_linearise_kernel<5>, grid, block, 0, s, a); break;
        case 6: hipLaunchKernelGGL(ba_linearise_kernel<6>, grid, block, 0, s, a); break;
        default: hipLaunchKernelGGL(ba_linearise_kernel<7>, grid, block, 0, s, a); break;
    }
    MVP_HIP(hipGetLastError());
}

}  // namespace

extern "C" int mvp_bundle_adjust_plan(int64_t n_points, int n_cam_idx, unsigned int free_mask, int64_t* workspace_bytes) {
    MVP_ABI_BEGIN
    const BaPlan pl = ba_plan("mvp_bundle_adjust_plan", n_points, n_cam_idx, free_mask);
    if (workspace_bytes) *workspace_bytes = pl.bytes;
    MVP_ABI_END
}

extern "C" int mvp_bundle_adjust_system(const float* kpts, int64_t n_points, int V, const double* cams, int n_cams,
                                        const int* cam_idx, int n_cam_idx, unsigned int free_mask, const float* xyz,
                                        const uint8_t* mask, int weights, const double* gauss, int J, float min_conf,
                                        float cov_floor, double huber_delta, double trans_prior_sigma, double lambda,
                                        void* workspace, int64_t workspace_bytes, double* out_S, double* out_b,
                                        double* out_cost, int64_t* out_counts, void* stream) {
    MVP_ABI_BEGIN
    const char* fn = "mvp_bundle_adjust_system";
    const BaCall c = ba_parse(fn, kpts, n_points, V, n_cams, cam_idx, n_cam_idx, free_mask, mask, weights, gauss, J,
                              min_conf, cov_floor, huber_delta, trans_prior_sigma, workspace_bytes);
    MVP_REQUIRE(std::isfinite(lambda) && lambda >= 0, "%s: lambda=%g (finite, >= 0)", fn, lambda);
    MVP_REQUIRE(kpts && cams && xyz && workspace && out_S && out_b && out_cost && out_counts, "%s: null device pointer", fn);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    uint8_t* used = reinterpret_cast<uint8_t*>(ws + c.pl.off_used);
    double* part = reinterpret_cast<double*>(ws + c.pl.off_part);
    hipLaunchKernelGGL(ba_prepare_kernel, dim3(tri_grid(fn, n_points)), dim3(kBlock), 0, s, c.obs, cams, c.vw, xyz, used,
                       (double*)nullptr, (int*)nullptr);
    MVP_HIP(hipGetLastError());
    BaLinArgs a{};
    a.obs = c.obs;
    a.vw = c.vw;
    a.st = nullptr;
    a.cams = cams;
    a.xyz32 = xyz;
    a.used = used;
    a.part = part;
    a.lambda = lambda;
    ba_launch_linearise(c, a, s);
    hipLaunchKernelGGL(ba_assemble_kernel, dim3(1), dim3(kBaSolveBlock), 0, s, part, c.pl.lin_grid, c.pl.nr, c.pl.F, lambda,
                       c.inv_s2, out_S, out_b, out_cost, out_counts);
    MVP_HIP(hipGetLastError());
    MVP_ABI_END
}

extern "C" int mvp_bundle_adjust(const float* kpts, int64_t n_points, int V, const double* cams, int n_cams,
                                 const int* cam_idx, int n_cam_idx, unsigned int free_mask, const float* xyz0,
                                 const uint8_t* mask, int weights, const double* gauss, int J, float min_conf,
                                 float cov_floor, double huber_delta, double trans_prior_sigma, int max_iter, double tol,
                                 void* workspace, int64_t workspace_bytes, double* out_cams, float* out_xyz,
                                 uint8_t* out_point_status, double* out_cam_cov, double* out_info, void* stream) {
    MVP_ABI_BEGIN
    const char* fn = "mvp_bundle_adjust";
    const BaCall c = ba_parse(fn, kpts, n_points, V, n_cams, cam_idx, n_cam_idx, free_mask, mask, weights, gauss, J,
                              min_conf, cov_floor, huber_delta, trans_prior_sigma, workspace_bytes);
    MVP_REQUIRE(max_iter >= 0 && max_iter <= 63, "%s: max_iter=%d (0..63)", fn, max_iter);
    MVP_REQUIRE(std::isfinite(tol) && tol > 0, "%s: tol=%g (finite, > 0)", fn, tol);
    MVP_REQUIRE(kpts && cams && xyz0 && workspace && out_cams && out_xyz && out_info, "%s: null device pointer", fn);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    BaState* st = reinterpret_cast<BaState*>(ws + c.pl.off_state);
    uint8_t* used = reinterpret_cast<uint8_t*>(ws + c.pl.off_used);
    double* x64 = reinterpret_cast<double*>(ws + c.pl.off_x);
    double* part = reinterpret_cast<double*>(ws + c.pl.off_part);
    double* tpart = reinterpret_cast<double*>(ws + c.pl.off_tpart);
    MVP_HIP(hipMemsetAsync(st, 0, sizeof(BaState), s));
    hipLaunchKernelGGL(ba_prepare_kernel, dim3(tri_grid(fn, n_points)), dim3(kBlock), 0, s, c.obs, cams, c.vw, xyz0, used,
                       x64, &st->view_cnt[0]);
    MVP_HIP(hipGetLastError());
    hipLaunchKernelGGL(ba_init_kernel, dim3(1), dim3(kBlock), 0, s, st, cams, n_cams, c.vw);
    MVP_HIP(hipGetLastError());
    BaLinArgs a{};
    a.obs = c.obs;
    a.vw = c.vw;
    a.st = st;
    a.cams = cams;
    a.x64 = x64;
    a.used = used;
    a.part = part;
    BaPtArgs pa{c.obs, c.vw, st, x64, used, tpart};
    for (int it = 0; it < max_iter; it++) {
        ba_launch_linearise(c, a, s);
        hipLaunchKernelGGL(ba_solve_kernel, dim3(1), dim3(kBaSolveBlock), 0, s, st, part, c.pl.lin_grid, c.pl.nr, c.vw, cams,
                           c.inv_s2);
        hipLaunchKernelGGL(ba_points_kernel, dim3((unsigned)c.pl.pt_grid), dim3(kBlock), 0, s, pa);
        hipLaunchKernelGGL(ba_decide_kernel, dim3(1), dim3(kBlock), 0, s, st, tpart, c.pl.pt_grid, c.vw, cams, c.inv_s2,
                           tol, max_iter);
        MVP_HIP(hipGetLastError());
    }
    a.final_pass = 1;
    ba_launch_linearise(c, a, s);
    hipLaunchKernelGGL(ba_final_kernel, dim3(1), dim3(kBaSolveBlock), 0, s, st, part, c.pl.lin_grid, c.pl.nr, c.vw, cams, n_cams,
                       c.inv_s2, out_cams, out_cam_cov, out_info);
    hipLaunchKernelGGL(ba_output_kernel, dim3(tri_grid(fn, n_points)), dim3(kBlock), 0, s, st, x64, used, xyz0, n_points,
                       out_xyz, out_point_status);
    MVP_HIP(hipGetLastError());
    MVP_ABI_END
}
