// Person detector, the band-halo conv (3x3/s1, >= 96 input channels, 80x80 / 40x40 planes) and
// its weight image.  Launched by detnet.cpp through det_launch_band for the ops selected
// onto it (det_select.h), whose weights detnet.cpp packs.
#include "det_common.h"

namespace mvp {
namespace {

// 3x3/s1 convs with >= 3 input chunks on the 80x80 and 40x40 planes (the CSPNeXt stage-3
// blocks, the neck's 40x40 blocks and out_convs, the head's stacked convs: ~18 of the 38.9
// GMAC per frame).  The im2col GEMM (det_gemm.hip) re-DMAs every input pixel once per tap, 20 KB per
// 786 K MAC (39 MAC/B from L2), which bounds it near a quarter of the MFMA peak.  Here a work
// item is a band of TR output rows x the whole width (320 pixels: 4 x 80 or 8 x 40) of one
// frame and 64 couts; per 32-channel input chunk its (TR + 2) x (W + 2) input halo (64 B per
// pixel, zero borders) and the chunk's weights for all 9 taps ([tap][cout][4 chunks], a
// contiguous 36 KB slice of the packed image, det_pack_band_weights) arrive by one round of
// LDS-DMA into one of two buffers while the previous chunk computes (~88 MAC per byte moved),
// and the taps are address offsets into the halo.  4 waves, each 80 output pixels (5
// fragments of 16) x the 64 couts (4 tiles): every A fragment read feeds 5 MFMAs, every B
// fragment 4 (v_mfma_f32_16x16x32_bf16).  Persistent workgroups, one per CU (137 KB of LDS),
// walk their items chunk by chunk with the next step's DMA in flight.  XCD-aware: the
// workgroups of one XCD (blockIdx % 8) form groups of n_nb (couts / 64) that take the same
// band together, one cout block each, so a band's input comes from HBM once into that XCD's
// L2.  Same swizzled row images as the GEMM kernel (a row = cout or halo pixel, its four 16-B
// channel chunks at 4r + (kg ^ swz(r))).  K order (chunk, tap, channel): equal to the GEMM
// kernel's (tap, chunk, channel) sums to f32 rounding.
template <int W, int TR>
struct BandCfg {
    static constexpr int HWD = W + 2, HP = (TR + 2) * HWD;  // halo row pitch, halo pixels
    static constexpr int P = TR * W;                        // output pixels per item
    static constexpr int A_SLOTS = 9 * 4 * kBandBN;         // [tap][cout][4]
    static constexpr int A_R64 = A_SLOTS / 64;
    static constexpr int B_R64 = (HP * 4 + 63) / 64;
    static constexpr int BUF = (A_SLOTS + B_R64 * 64) * 16;
    static constexpr int LDS = 2 * BUF;
    static constexpr int FPW = P / 64;                      // 16-pixel fragments per wave (4 waves)
    static_assert(P == 320 && FPW == 5, "band: 320-pixel items");
    static_assert(LDS <= 160 * 1024, "band: LDS budget");
};

// (Measured and dropped: a plane-major halo — [4 channel chunks][halo pixel] 16-B slots, tap
// offsets as immediates, no swizzle, 16-B DMA pieces — 23.80 vs 23.32 ms per 128-frame forward,
// gpurun_out/detband4: four times the DMA pieces cost more than the address arithmetic saved.)
// NWV waves: 4 (one per SIMD, each 80 pixels x the 64 couts) or 8 (two per SIMD, each 80 pixels
// x 32 couts: more LDS reads, but a second wave to hide each one's waits).
// (Measured and dropped, round 6: the 20x20 planes as whole-frame items of 400 pixels = 5 pixel
// groups x 2 cout groups, 10 waves: 24 % of the MFMA peak against the GEMM kernel's 31 % there —
// the SIMDs hold 3, 3, 2, 2 waves — 5.58 vs 4.47 ms for the 8 convs, profiles/r06_det_folds.txt.)
template <int W, int TR, int NWV>
__global__ __launch_bounds__(64 * NWV, 1) void det_conv_band_kernel(GParams p, const uint16_t* __restrict__ wband) {
    using C = BandCfg<W, TR>;
    constexpr int FP = C::FPW;
    constexpr int CT = 4 * 4 / NWV;  // 16-cout tiles per wave
    static_assert(NWV == 4 || NWV == 8, "band: 4 or 8 waves");
    extern __shared__ __attribute__((aligned(1024))) uint8_t lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wp = wave & 3, wc = wave >> 2;  // pixel group, cout group
    auto swz = [](int r) { return (-(r >> 2)) & 3; };
    // item assignment (see above): WG b on XCD b % 8, group g of n_nb consecutive slots
    const int n_nb = p.n_nb, nck = p.cin / 32;
    const int G = gridDim.x, b = blockIdx.x;
    const int xcd = b & 7, sl = b >> 3, spx = G >> 3;
    const int ng = spx / n_nb;
    if (sl >= ng * n_nb) return;  // whole workgroup: uniform
    const int nb = sl % n_nb, g = sl / n_nb;
    const int tpi = p.H / TR;  // bands per frame
    const int tiles = (int)(p.M / ((long)p.H * W)) * tpi;
    const int n_items = tiles > (g * 8 + xcd) ? (tiles - (g * 8 + xcd) + ng * 8 - 1) / (ng * 8) : 0;
    if (n_items == 0) return;
    const int steps = n_items * nck;
    auto item_tile = [&](int k) { return (k * ng + g) * 8 + xcd; };
    // DMA of step st (chunk c of item k) into buffer buf, in 9 parts: part j = this wave's
    // weight round j (9 per wave) and halo round j (<= 8 per wave).  The parts are issued one
    // per tap in the middle of the previous step's MFMAs, so their address arithmetic rides in
    // the MFMA shadow; the halo rounds use per-item source offsets (hoff, recomputed when the
    // next step starts a new item: -1 = outside the frame, the zero region).
    constexpr int HR = (C::B_R64 + NWV - 1) / NWV;  // halo rounds per wave (some waves one fewer)
    constexpr int AR = (C::A_R64 + NWV - 1) / NWV;  // weight rounds per wave (some waves one fewer)
    constexpr int NPART = AR > HR ? AR : HR;         // DMA parts per wave and step
    static_assert(NPART <= 9, "band: DMA parts");
    int hoff[HR];
    const uint16_t* xframe = p.x;
    auto set_item = [&](int k) {
        const int t = item_tile(k), n = t / tpi, row0 = (t - n * tpi) * TR;
        xframe = p.x + (size_t)n * p.H * W * p.xs;
#pragma unroll
        for (int j = 0; j < HR; j++) {
            const int s2 = (wave + NWV * j) * 64 + lane, hp = s2 >> 2, kq = (s2 & 3) ^ swz(hp);
            const int hy = hp / C::HWD, hx = hp - hy * C::HWD;
            const int gy = row0 + hy - 1, gx = hx - 1;
            const bool in = hp < C::HP && (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)W;
            hoff[j] = in ? (gy * W + gx) * p.xs + kq * 8 : -1;
        }
    };
    auto issue_part = [&](int st, int buf, int j) {
        const int k = st / nck, c = st - k * nck;
        uint8_t* base = lds + buf * C::BUF;
        const int r = wave + NWV * j;
        if (j < AR && r < C::A_R64)
            glds16_det(wband + ((size_t)(nb * nck + c) * C::A_SLOTS + r * 64 + lane) * 8, base + r * 64 * 16);
        if (j < HR && r < C::B_R64) {
            const int s2 = r * 64 + lane;
            const void* src = hoff[j] >= 0 ? (const void*)(xframe + hoff[j] + c * 32)
                                           : (const void*)(p.zero + (s2 & 1023) * 8);
            glds16_det(src, base + (C::A_SLOTS + s2) * 16);
        }
    };
    const int kg = lane >> 4, r16 = lane & 15;
    const int soffA = (r16 * 4 + (kg ^ swz(r16))) * 16;
    int hb[FP];  // halo index of tap (0, 0) for this lane's pixel of each fragment
#pragma unroll
    for (int i = 0; i < FP; i++) {
        const int px = wp * (FP * 16) + i * 16 + r16, pr = px / W, pc = px - pr * W;
        hb[i] = pr * C::HWD + pc;
    }
    f32x4 acc[FP][CT];
    // one chunk's 9 taps from LDS buffer `base`, with the DMA parts of step `nst` in its first
    // taps (nst < 0: none); tap t + 1's fragments are read in the middle of tap t's MFMAs (two
    // register sets).
    auto compute = [&](const uint8_t* base, int nst, int nbuf) {
        bf16x8 fa[2][CT], fbv[2][FP];
        auto load_a = [&](int tp, int sl) {
#pragma unroll
            for (int ct = 0; ct < CT; ct++)
                fa[sl][ct] =
                    *reinterpret_cast<const bf16x8*>(base + (tp * 4 * kBandBN + (wc * CT + ct) * 64) * 16 + soffA);
        };
        auto load_b = [&](int tp, int sl) {
            const int toff = (tp / 3) * C::HWD + (tp % 3);
#pragma unroll
            for (int i = 0; i < FP; i++) {
                const int hp = hb[i] + toff;
                fbv[sl][i] = *reinterpret_cast<const bf16x8*>(base + (C::A_SLOTS + hp * 4 + (kg ^ swz(hp))) * 16);
            }
        };
        load_b(0, 0);
        load_a(0, 0);
        // per tap: 8 MFMAs, then tap t + 1's 9 fragment reads and this tap's DMA part, then the
        // other 12 MFMAs: the compiler's wait before the next tap (it can only wait for every
        // outstanding LDS read while LDS-DMA is in flight) then covers reads 12 MFMAs old
#pragma unroll
        for (int tp = 0; tp < 9; tp++) {
            const int sl = tp & 1;
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int ct = 0; ct < CT; ct++)
                    acc[i][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[sl][ct], fbv[sl][i], acc[i][ct], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if (tp + 1 < 9) {
                load_b(tp + 1, sl ^ 1);
                load_a(tp + 1, sl ^ 1);
            }
            // the next step's DMA in the first 5 taps (2 parts each): it lands well before the
            // step's vmcnt wait
            if constexpr (NPART > 5) {  // 2 parts per tap
                if (nst >= 0 && 2 * tp < NPART) issue_part(nst, nbuf, 2 * tp);
                if (nst >= 0 && 2 * tp + 1 < NPART) issue_part(nst, nbuf, 2 * tp + 1);
            } else {
                if (nst >= 0 && tp < NPART) issue_part(nst, nbuf, tp);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 2; i < FP; i++)
#pragma unroll
                for (int ct = 0; ct < CT; ct++)
                    acc[i][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[sl][ct], fbv[sl][i], acc[i][ct], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    set_item(0);
#pragma unroll
    for (int j = 0; j < NPART; j++) issue_part(0, 0, j);
    int buf = 0, st = 0;
    for (int k = 0; k < n_items; k++) {
#pragma unroll
        for (int i = 0; i < FP; i++)
#pragma unroll
            for (int ct = 0; ct < CT; ct++) acc[i][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < nck; c++, st++) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's DMA of step st (and stores)
            __builtin_amdgcn_s_barrier();                         // every wave's; buffer buf ^ 1 is free
            asm volatile("" ::: "memory");
            const bool more = st + 1 < steps;
            if (more && c + 1 == nck) set_item(k + 1);  // the next step starts item k + 1
            compute(lds + buf * C::BUF, more ? st + 1 : -1, buf ^ 1);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            buf ^= 1;
        }
        // epilogue of item k: lane holds couts 16 ct + 4 kg + j of its pixel
        const int t = item_tile(k), n = t / tpi, row0 = (t - n * tpi) * TR;
#pragma unroll
        for (int ct = 0; ct < CT; ct++) {
            const int co = nb * kBandBN + (wc * CT + ct) * 16 + kg * 4;
            if (co >= p.N) continue;
            const float4 bv = *reinterpret_cast<const float4*>(p.bias + co);
#pragma unroll
            for (int i = 0; i < FP; i++) {
                const int px = wp * (FP * 16) + i * 16 + r16, pr = px / W, pc = px - pr * W;
                const long m = ((long)n * p.H + row0 + pr) * W + pc;
                const f32x4 ac = acc[i][ct];
                float v[4] = {ac[0] + bv.x, ac[1] + bv.y, ac[2] + bv.z, ac[3] + bv.w};
                if (p.act == 2)
#pragma unroll
                    for (int e = 0; e < 4; e++) v[e] = act_f(v[e], 2);
                if (p.res) {
                    const uint2 rr = *reinterpret_cast<const uint2*>(p.res + m * p.rs + co);
                    v[0] += bf(rr.x & 0xffff), v[1] += bf(rr.x >> 16), v[2] += bf(rr.y & 0xffff),
                        v[3] += bf(rr.y >> 16);
                }
                if (p.act == 1)
#pragma unroll
                    for (int e = 0; e < 4; e++) v[e] = fmaxf(v[e], 0.f);
                *reinterpret_cast<uint2*>(p.y + m * p.ys + co) =
                    uint2{tobf(v[0]) | (tobf(v[1]) << 16), tobf(v[2]) | (tobf(v[3]) << 16)};
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// band weight image: [nb][chunk][tap][cout 64][4 swizzled 16-B chunks] from w [npad][3][3][cin];
// couts past npad (the last block of a 96-cout conv) are zero rows
__global__ __launch_bounds__(256) void det_pack_band_kernel(const uint16_t* __restrict__ w, uint16_t* __restrict__ img,
                                                          int npad, int cin) {
    const int nck = cin / 32;
    const int rows = (npad + kBandBN - 1) / kBandBN * kBandBN;
    const long n = (long)rows * 9 * cin / 8;  // 16-B slots
    for (long d = blockIdx.x * 256L + threadIdx.x; d < n; d += (long)gridDim.x * 256) {
        const int q = (int)(d & 3);
        const long r = d >> 2;                  // (nb, chunk, tap, co)
        const int co = (int)(r % kBandBN);
        const long r2 = r / kBandBN;
        const int tp = (int)(r2 % 9);
        const long r3 = r2 / 9;
        const int c = (int)(r3 % nck), nb = (int)(r3 / nck);
        const int kg = q ^ ((-(co >> 2)) & 3);
        const int row = nb * kBandBN + co;
        *reinterpret_cast<uint4*>(img + d * 8) =
            row < npad ? *reinterpret_cast<const uint4*>(w + ((size_t)row * 9 + tp) * cin + c * 32 + kg * 8)
                       : uint4{0u, 0u, 0u, 0u};
    }
}

}  // namespace

void det_pack_band_weights(const uint16_t* w, uint16_t* img, int npad, int cin, hipStream_t s) {
    MVP_REQUIRE(npad % 32 == 0 && cin % 32 == 0, "det_pack_band_weights: npad %d, cin %d", npad, cin);
    hipLaunchKernelGGL(det_pack_band_kernel, dim3(512), dim3(256), 0, s, w, img, npad, cin);
    MVP_HIP(hipGetLastError());
}

namespace {
template <int W, int TR, int NWV>
void launch_band(const GParams& p, const uint16_t* wband, hipStream_t s) {
    using C = BandCfg<W, TR>;
    det_dyn_lds<det_conv_band_kernel<W, TR, NWV>>(C::LDS);
    hipLaunchKernelGGL((det_conv_band_kernel<W, TR, NWV>), dim3(det_band_grid()), dim3(64 * NWV), C::LDS, s, p, wband);
}
}  // namespace

void det_launch_band(const GParams& p, int n, const uint16_t* wband, bool waves4, hipStream_t s) {
    GParams pb = p;
    pb.n_nb = det_band_rows(p.npad) / kBandBN;
    // 8 waves (two per SIMD) by default: 22.30 vs 23.33 ms per 128-frame forward with 4
    // (gpurun_out/detband5); MVPOSE_DET_BAND=4 keeps the 4-wave form (tests: bit-identical)
    if (p.W == 80) waves4 ? launch_band<80, 4, 4>(pb, wband, s) : launch_band<80, 4, 8>(pb, wband, s);
    else waves4 ? launch_band<40, 8, 4>(pb, wband, s) : launch_band<40, 8, 8>(pb, wband, s);
    MVP_HIP(hipGetLastError());
}

}  // namespace mvp
