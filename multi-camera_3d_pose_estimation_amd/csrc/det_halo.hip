// Person detector, the halo-tile convs (3x3/s1, 32 or 64 input channels, <= 64 couts): one tile
// per workgroup, and the persistent form with the weights resident in LDS.  Launched by
// detnet.cpp through det_launch_halo with the variant mvp_det_create selected (det_select.h).
#include "det_common.h"

namespace mvp {
namespace {

// 3x3/s1 convs with one 32-channel input chunk (the 320x320 stem / stage-1 planes, 24 -> 32
// padded channels): im2col re-DMAs every input pixel once per tap while a tap's K work is a
// single chunk, so the GEMM kernel (det_gemm.hip) is DMA-issue bound there.  Here a tile is 2 output
// rows x 64 columns of one frame; its 4 x 66 input halo (64 B per pixel) and all 9 taps'
// weights arrive in one DMA phase, and the taps are LDS offsets.  Same swizzled row-major
// images as the GEMM kernel (row = halo pixel / cout, 4 16-B chunks per row); the
// workgroup then runs its 9 K-steps without another barrier (3 workgroups per CU hide the
// DMA).  One chunk: K order (tap, channel) as the GEMM kernel, identical sums; two chunks
// (64 channels, one DMA + compute phase each): chunk-major K order, equal to f32 rounding.
// TR output rows per tile (2 or 4): wave (wp, wc) computes rows wp, wp + 2, ... of cout half
// wc.  4 rows spread each tile's weight DMA over twice the pixels (62.5 KB of LDS, 2
// workgroups per CU, against 54 KB and 3 for 2 rows); the K order per output is the same.
// LT > 0 (round 6): only the first LT 16-cout tiles carry real channels (RTMDet-m's 48-channel
// stem / stage-1 convs stored as 64: the last tile's weights and biases are zero, so its outputs
// are SiLU(0) = +0).  Each of the 4 waves then takes one output row of a 4-row tile and all LT
// tiles (12 MFMAs per tap instead of 16: the zero tile is not multiplied) and stores zeros for
// the padding couts — the real couts' K order and epilogue are unchanged: bit-identical.
template <int BN, int NCK, int TR = 2, int LT = 0>  // NCK 32-channel input chunks, one DMA + compute phase each
__global__ __launch_bounds__(256, TR == 2 ? 3 : 2) void det_conv_halo_kernel(GParams p) {
    constexpr bool ROWS = LT > 0;
    static_assert(!ROWS || (TR % 4 == 0 && LT < BN / 16), "live-tile halo: 4-row tiles");
    constexpr int TW = 64, HW_ = TW + 2, HP = (TR + 2) * HW_;  // halo pixels
    constexpr int RS = ROWS ? 4 : 2;                           // row stride between a wave's rows
    constexpr int NRW = TR / RS;                               // output rows per wave
    constexpr int A_SLOTS = 9 * 4 * BN, A_R64 = A_SLOTS / 64;
    constexpr int B_R64 = (HP * 4 + 63) / 64;
    constexpr int WCT = ROWS ? LT : BN / 32;                   // 16-cout tiles per wave
    __shared__ __attribute__((aligned(1024))) uint8_t lds[(A_SLOTS + B_R64 * 64) * 16];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wp = ROWS ? wave : wave & 1, wc = ROWS ? 0 : wave >> 1;  // output row of the tile, cout half
    const int tiles_w = (p.W + TW - 1) / TW, tiles_h = (p.H + TR - 1) / TR;
    const int per = tiles_w * tiles_h;
    const int n = blockIdx.x / per, t = blockIdx.x - n * per;
    const int ho0 = (t / tiles_w) * TR, wo0 = (t - (t / tiles_w) * tiles_w) * TW;
    auto swz = [](int r) { return (-(r >> 2)) & 3; };
    const uint16_t* xb = p.x + (size_t)n * p.H * p.W * p.xs;
    const int kg = lane >> 4, r16 = lane & 15;
    const int soff = r16 * 64 + ((kg ^ swz(r16)) * 16);
    f32x4 acc[NRW][4][WCT];
#pragma unroll
    for (int rw = 0; rw < NRW; rw++)
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int c = 0; c < WCT; c++) acc[rw][i][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int q = 0; q < NCK; q++) {
    if (q > 0) __builtin_amdgcn_s_barrier();  // every wave is done with chunk q-1's images
    // weights: slot s of tap tp = tp * 4BN + 4co + (kg ^ swz(co))
    for (int r = wave; r < A_R64; r += 4) {
        const int sl = r * 64 + lane, tp = sl / (4 * BN), rem = sl - tp * (4 * BN);
        const int co = rem >> 2, kq = (rem & 3) ^ swz(co);
        glds16_det(p.w + (size_t)co * (288 * NCK) + tp * (32 * NCK) + q * 32 + kq * 8, lds + r * 64 * 16);
    }
    // input halo: slot s = 4hp + (kg ^ swz(hp)), hp = halo row * 66 + halo col
    for (int r = wave; r < B_R64; r += 4) {
        const int sl = r * 64 + lane, hp = sl >> 2, kq = (sl & 3) ^ swz(hp);
        const int hy = hp / HW_, hx = hp - hy * HW_;
        const int gy = ho0 + hy - 1, gx = wo0 + hx - 1;
        const bool in = hp < HP && (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W;
        const void* src = in ? (const void*)(xb + ((size_t)gy * p.W + gx) * p.xs + q * 32 + kq * 8)
                             : (const void*)(p.zero + (sl & 1023) * 8);
        glds16_det(src, lds + (A_SLOTS + r * 64) * 16);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
#pragma unroll
    for (int tp = 0; tp < 9; tp++) {
        const int dy = tp / 3, dx = tp % 3;
        bf16x8 a[WCT], b[NRW][4];
#pragma unroll
        for (int c = 0; c < WCT; c++)
            a[c] = *reinterpret_cast<const bf16x8*>(lds + tp * 4 * BN * 16 + (wc * (BN / 2) + c * 16) * 64 + soff);
#pragma unroll
        for (int rw = 0; rw < NRW; rw++)
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int hp = (wp + RS * rw + dy) * HW_ + i * 16 + r16 + dx;
                b[rw][i] = *reinterpret_cast<const bf16x8*>(lds + A_SLOTS * 16 + hp * 64 + ((kg ^ swz(hp)) * 16));
            }
#pragma unroll
        for (int rw = 0; rw < NRW; rw++)
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int c = 0; c < WCT; c++)
                    acc[rw][i][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[c], b[rw][i], acc[rw][i][c], 0, 0, 0);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
#pragma unroll
    for (int rw = 0; rw < NRW; rw++) {
    const int ho = ho0 + wp + RS * rw;
    if (ho >= p.H) break;
    if constexpr (ROWS) {   // the zero tiles' couts
#pragma unroll
        for (int c = LT; c < BN / 16; c++) {
            const int co = c * 16 + kg * 4;
            if (co >= p.N) continue;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int wo = wo0 + i * 16 + r16;
                if (wo >= p.W) continue;
                *reinterpret_cast<uint2*>(p.y + (((long)n * p.H + ho) * p.W + wo) * p.ys + co) = uint2{0u, 0u};
            }
        }
    }
#pragma unroll
    for (int c = 0; c < WCT; c++) {
        const int co = wc * (BN / 2) + c * 16 + kg * 4;
        if (co >= p.N) continue;
        const float4 bb = *reinterpret_cast<const float4*>(p.bias + co);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int wo = wo0 + i * 16 + r16;
            if (wo >= p.W) continue;
            const long m = ((long)n * p.H + ho) * p.W + wo;
            const f32x4 ac = acc[rw][i][c];
            float v[4] = {ac[0] + bb.x, ac[1] + bb.y, ac[2] + bb.z, ac[3] + bb.w};
            if (p.act == 2)
#pragma unroll
                for (int e = 0; e < 4; e++) v[e] = act_f(v[e], 2);
            if (p.res) {
                const uint2 r = *reinterpret_cast<const uint2*>(p.res + m * p.rs + co);
                v[0] += bf(r.x & 0xffff), v[1] += bf(r.x >> 16), v[2] += bf(r.y & 0xffff), v[3] += bf(r.y >> 16);
            }
            if (p.act == 1)
#pragma unroll
                for (int e = 0; e < 4; e++) v[e] = fmaxf(v[e], 0.f);
            *reinterpret_cast<uint2*>(p.y + m * p.ys + co) =
                uint2{tobf(v[0]) | (tobf(v[1]) << 16), tobf(v[2]) | (tobf(v[3]) << 16)};
        }
    }
    }
}

// Persistent halo conv (round 6) for the 64-cout 3x3/s1 convs with one or two input chunks (the
// 320x320 stem.2 and the 160x160 stage-1 block conv1s: ~6.6 ms of the 512-frame forward).
// det_conv_halo_kernel re-DMAs the conv's whole weight set (36 KB per chunk) with every
// 256-pixel tile: 60 % of its LDS-DMA bytes, and without them the forward ran 3.2 ms faster
// (timing diagnostic, profiles/r06_det_halo_pers.txt).  Here one workgroup per CU (8 waves)
// keeps the weights of every chunk resident in LDS for the launch and walks 8-row x 64-column
// tiles (a contiguous per-XCD range, so neighbouring tiles' halo rows meet in that L2); each
// (tile, chunk) step's 10 x 66 halo arrives by LDS-DMA into one of two buffers while the
// previous step computes.  Wave w computes output row w of the tile for the LT live 16-cout
// tiles (4 pixel fragments each); the padding couts are stored as zeros (their weights and
// biases are zero).  The DMA and the stores are asm the compiler does not track (no vmcnt it
// would put in front of LDS reads); the kernel counts its own waits.  Same operand images and
// K order (chunk, tap, channel) as det_conv_halo_kernel: bit-identical.
template <int BN_, int NCK, int LT>
struct HaloPersCfg {
    static constexpr int BN = BN_, TR = 8, TW = 64, HW_ = TW + 2, HP = (TR + 2) * HW_;
    static constexpr int NWV = 8, NT = 64 * NWV;
    static constexpr int A_SLOTS = 9 * 4 * BN;              // one chunk's weights, [tap][cout][4]
    static constexpr int B_R64 = (HP * 4 + 63) / 64;        // halo DMA rounds (1 KiB each)
    static constexpr int BUF = B_R64 * 64 * 16;             // one halo buffer
    static constexpr int OFF_B = NCK * A_SLOTS * 16;
    static constexpr int LDS = OFF_B + 2 * BUF;
    static_assert(LDS <= 160 * 1024, "halo pers: LDS budget");
    static_assert(LT >= 1 && LT <= BN / 16 && (BN == 32 || BN == 64), "live tiles");
};

template <int BN_, int NCK, int LT>
__global__ __launch_bounds__(512, 1) void det_conv_halo_pers_kernel(GParams p) {
    using G = HaloPersCfg<BN_, NCK, LT>;
    constexpr int BN = G::BN, TR = G::TR, TW = G::TW, HW_ = G::HW_, NWV = G::NWV;
    extern __shared__ __attribute__((aligned(1024))) uint8_t lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    auto swz = [](int r) { return (-(r >> 2)) & 3; };
    const int tiles_w = (p.W + TW - 1) / TW, tiles_h = (p.H + TR - 1) / TR, per = tiles_w * tiles_h;
    const long T = p.M / ((long)p.H * p.W) * per;
    const int NG = gridDim.x, xcd = blockIdx.x & 7, loc = blockIdx.x >> 3;
    const int gx = NG / 8 + (xcd < (NG & 7) ? 1 : 0);
    const long qx = T >> 3, rx = T & 7;
    const long x0 = xcd < rx ? xcd * (qx + 1) : rx * (qx + 1) + (xcd - rx) * qx;
    const long x1 = x0 + qx + (xcd < rx ? 1 : 0);
    const long n_tiles = x1 - x0 > loc ? (x1 - x0 - loc + gx - 1) / gx : 0;
    if (n_tiles == 0) return;  // workgroup-uniform
    const long S = n_tiles * NCK;
    // the weights of every chunk, once: slot s of chunk q = tap * 4BN + 4co + (kq ^ swz(co))
    for (int i = tid; i < NCK * G::A_SLOTS; i += G::NT) {
        const int q = i / G::A_SLOTS, sl = i - q * G::A_SLOTS, tp = sl / (4 * BN), rem = sl - tp * (4 * BN);
        const int co = rem >> 2, kq = (rem & 3) ^ swz(co);
        *reinterpret_cast<uint4*>(lds + i * 16) =
            *reinterpret_cast<const uint4*>(p.w + (size_t)co * (288 * NCK) + tp * (32 * NCK) + q * 32 + kq * 8);
    }
    const int kg = lane >> 4, r16 = lane & 15;
    // the lane's biases, complete before the loop (a load the compiler still counted as pending
    // there would put a vmcnt wait, covering the next step's DMA, into every epilogue)
    f32x4 bb[LT];
#pragma unroll
    for (int c = 0; c < LT; c++) {
        bb[c] = *reinterpret_cast<const f32x4*>(p.bias + c * 16 + kg * 4);
        asm volatile("" : "+v"(bb[c]));
    }
    auto tile_of = [&](long t, int& n, int& ho0, int& wo0) {
        const long lt = x0 + loc + t * gx;
        n = (int)(lt / per);
        const int r = (int)(lt - (long)n * per), th = r / tiles_w;
        ho0 = th * TR;
        wo0 = (r - th * tiles_w) * TW;
    };
    auto issue = [&](long st, int buf) {
        const long t = st / NCK;
        const int q = (int)(st - t * NCK);
        int n, ho0, wo0;
        tile_of(t, n, ho0, wo0);
        const uint16_t* xb = p.x + (size_t)n * p.H * p.W * p.xs;
#pragma unroll
        for (int j = 0; j < (G::B_R64 + NWV - 1) / NWV; j++) {
            const int r = wave + NWV * j;
            if (r < G::B_R64) {  // wave-uniform
                const int sl = r * 64 + lane, hp = sl >> 2, kq = (sl & 3) ^ swz(hp);
                const int hy = hp / HW_, hx = hp - hy * HW_;
                const int gy = ho0 + hy - 1, gx2 = wo0 + hx - 1;
                const bool in = hp < G::HP && (unsigned)gy < (unsigned)p.H && (unsigned)gx2 < (unsigned)p.W;
                const void* src = in ? (const void*)(xb + ((size_t)gy * p.W + gx2) * p.xs + q * 32 + kq * 8)
                                     : (const void*)(p.zero + (sl & 1023) * 8);
                glds16_raw(src, (uint32_t)(G::OFF_B + buf * G::BUF + r * 1024));
            }
        }
    };
    constexpr int kStores = 4 * (BN / 16);  // per wave and tile: 4 fragments x every 16-cout tile
    const int soff = r16 * 64 + ((kg ^ swz(r16)) * 16);
    f32x4 acc[4][LT];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int c = 0; c < LT; c++) acc[i][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    issue(0, 0);
    __syncthreads();  // the weights (plain stores) are visible
    int st_after = 0;  // store instructions issued since the last DMA issue
    for (long st = 0; st < S; st++) {
        const int buf = (int)(st & 1);
        wait_vm(st_after);  // this wave's DMA of step st landed (only the later stores may be pending)
        __builtin_amdgcn_s_barrier();  // every wave's; the other buffer is free
        asm volatile("" ::: "memory");
        if (st + 1 < S) {
            issue(st + 1, buf ^ 1);
            st_after = 0;
        }
        const long t = st / NCK;
        const int q = (int)(st - t * NCK);
        const uint8_t* wa = lds + q * G::A_SLOTS * 16;
        const uint8_t* hb = lds + G::OFF_B + buf * G::BUF;
#pragma unroll
        for (int tp = 0; tp < 9; tp++) {
            const int dy = tp / 3, dx = tp % 3;
            bf16x8 a[LT], b[4];
#pragma unroll
            for (int c = 0; c < LT; c++) a[c] = *reinterpret_cast<const bf16x8*>(wa + tp * 4 * BN * 16 + (c * 16) * 64 + soff);
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int hp = (wave + dy) * HW_ + i * 16 + r16 + dx;
                b[i] = *reinterpret_cast<const bf16x8*>(hb + hp * 64 + ((kg ^ swz(hp)) * 16));
            }
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int c = 0; c < LT; c++) acc[i][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[c], b[i], acc[i][c], 0, 0, 0);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (q + 1 < NCK) continue;
        // ---- the tile's epilogue: row `wave` of the tile, every 16-cout tile (zeros past LT)
        int n, ho0, wo0;
        tile_of(t, n, ho0, wo0);
        const int ho = ho0 + wave;
        const uint16_t* yb = p.y + (((size_t)n * p.H + (ho < p.H ? ho : 0)) * p.W + wo0) * p.ys;
        const i32x4 yr = make_rsrc(yb, (int)std::min<long>((long)TW * p.ys * 2, 0x7fffffffL));
#pragma unroll
        for (int c = 0; c < BN / 16; c++) {
            const int co = c * 16 + kg * 4;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int wo = wo0 + i * 16 + r16;
                u32x2 o = {0u, 0u};
                if (c < LT) {
                    const f32x4 ac = acc[i][c < LT ? c : 0];
                    const f32x4 bc = bb[c < LT ? c : 0];
                    float v[4] = {ac[0] + bc[0], ac[1] + bc[1], ac[2] + bc[2], ac[3] + bc[3]};
#pragma unroll
                    for (int e = 0; e < 4; e++) v[e] = act_f(v[e], p.act);
                    o = u32x2{tobf(v[0]) | (tobf(v[1]) << 16), tobf(v[2]) | (tobf(v[3]) << 16)};
                }
                const bool ok = ho < p.H && wo < p.W && co < p.N;
                buffer_store_u2v(o, yr, ok ? ((i * 16 + r16) * p.ys + co) * 2 : 0x7ff00000);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int c = 0; c < LT; c++) acc[i][c] = f32x4{0.f, 0.f, 0.f, 0.f};
        st_after = kStores;
    }
}

}  // namespace

namespace {
// the conv's cout tile (npad 32 | 64) and 32-channel input chunks (cin 32 | 64), as constants:
// f(det_int<BN>, det_int<NCK>)
template <typename F>
void by_npad_cin(int npad, int cin, F&& f) {
    if (cin == 64 && npad == 64) f(det_int<64>{}, det_int<2>{});
    else if (cin == 64) f(det_int<32>{}, det_int<2>{});
    else if (npad == 64) f(det_int<64>{}, det_int<1>{});
    else f(det_int<32>{}, det_int<1>{});
}

// persistent, weights resident (det_conv_halo_pers_kernel)
template <int BN, int NCK, int LT>
void launch_halo_pers(const GParams& p, int n, hipStream_t s) {
    using G = HaloPersCfg<BN, NCK, LT>;
    det_dyn_lds<det_conv_halo_pers_kernel<BN, NCK, LT>>(G::LDS);
    const long grid = det_pers_grid((long)n * ((p.H + 7) / 8) * ((p.W + 63) / 64));
    hipLaunchKernelGGL((det_conv_halo_pers_kernel<BN, NCK, LT>), dim3((unsigned)grid), dim3(512), G::LDS, s, p);
}
}  // namespace

void det_launch_halo(const GParams& p, int n, DetKernel variant, hipStream_t s) {
    const int tr = variant == DK_HALO_2ROW ? 2 : DET_HALO_TR;
    const long tiles = (long)n * ((p.H + tr - 1) / tr) * ((p.W + 63) / 64);
    by_npad_cin(p.npad, p.cin, [&](auto bn, auto nck) {
        constexpr int BN = decltype(bn)::value, NCK = decltype(nck)::value;
        auto go = [&](auto kern) { hipLaunchKernelGGL(kern, dim3((unsigned)tiles), dim3(256), 0, s, p); };
        if (variant == DK_HALO_2ROW) {
            go(det_conv_halo_kernel<BN, NCK, 2>);
        } else if (variant == DK_HALO) {
            go(det_conv_halo_kernel<BN, NCK, DET_HALO_TR>);
        } else if constexpr (BN == 64) {  // the variants select_det_conv gives the 64-cout convs only
            if (variant == DK_HALO_PERS_LT3) launch_halo_pers<64, NCK, 3>(p, n, s);
            else if (variant == DK_HALO_PERS_LT4) launch_halo_pers<64, NCK, 4>(p, n, s);
            else go(det_conv_halo_kernel<64, NCK, DET_HALO_TR, 3>);  // DK_HALO_LIVE3
        } else if constexpr (NCK == 1) {
            launch_halo_pers<32, 1, 2>(p, n, s);  // DK_HALO_PERS_LT2
        }
    });
    MVP_HIP(hipGetLastError());
}

}  // namespace mvp
