// Person detector, the CSPNeXt blocks' depthwise convs: the 5x5 depthwise kernel and the fused
// depthwise 5x5 + pointwise 1x1 kernel.  Called by detnet.cpp through det.h (launch_det_dw5,
// launch_det_dwpw).
#include "det_common.h"

namespace mvp {
namespace {

// ------------------------------------------------------------------ depthwise 5x5
// Memory-bound (25 MACs per element): one workgroup = an 8 x 16 output tile x G channel
// chunks of 8 (G waves, one chunk per wave).  The 12 x 20 input halo is loaded coalesced
// (G consecutive 16-B chunks of a pixel per lane group) into LDS stored chunk-major, so a
// wave's fragment reads are 64 consecutive pixels of its chunk (conflict-free).  Each lane
// computes two vertically adjacent outputs (6 input rows x 5 taps for 2 outputs); the
// weights are wave-uniform ([C/8][25][8] f32), read through the scalar cache.
constexpr int kDwTH = 8, kDwTW = 16, kDwHH = kDwTH + 4, kDwHW = kDwTW + 4;

struct DwParams {
    const uint16_t* x;
    uint16_t* y;
    const float* w;  // [C/8][25][8]
    const float* b;  // [C]
    int H, W, C, xs, ys, act, tiles_w;
};

template <int G>
__global__ __launch_bounds__(G * 64, 8 / G * 2) void dw5_kernel(DwParams p) {
    __shared__ uint4 sh[G][kDwHH * kDwHW];
    const int n_groups = p.C / (8 * G);
    const int grp = blockIdx.x % n_groups;
    const int t2 = blockIdx.x / n_groups;
    const int tw = t2 % p.tiles_w, th = t2 / p.tiles_w;
    const int n = blockIdx.y;
    const int h0 = th * kDwTH - 2, w0 = tw * kDwTW - 2;
    const int tid = threadIdx.x;
    const uint16_t* xb = p.x + (size_t)n * p.H * p.W * p.xs + grp * 8 * G;
    for (int i = tid; i < kDwHH * kDwHW * G; i += G * 64) {
        const int pix = i / G, q = i - pix * G;
        const int r = pix / kDwHW, c = pix - r * kDwHW;
        const int hi = h0 + r, wi = w0 + c;
        sh[q][pix] = (hi >= 0 && hi < p.H && wi >= 0 && wi < p.W)
                         ? *reinterpret_cast<const uint4*>(xb + ((size_t)hi * p.W + wi) * p.xs + q * 8)
                         : uint4{0u, 0u, 0u, 0u};
    }
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int col = lane & 15, rp = lane >> 4;
    const int chunk = grp * G + wave;
    const float* wc = p.w + (size_t)chunk * 200;
    // channel pairs on packed FMAs (v_pk_fma_f32: two fmaf per instruction, the same roundings):
    // the kernel is VALU-issue-bound (~1,100 VALU instructions per wave with scalar fmaf)
    typedef float f32x2v __attribute__((ext_vector_type(2)));
    f32x2v a0[4], a1[4];
#pragma unroll
    for (int c = 0; c < 4; c++) a0[c] = a1[c] = f32x2v{0.f, 0.f};
    // input rows one at a time (not unrolled): 8 unpacked values live, not 240, so the
    // kernel fits 8 waves per SIMD and the next block's halo load hides under this one
#pragma unroll 1
    for (int ir = 0; ir < 6; ir++) {
#pragma unroll
        for (int kw = 0; kw < 5; kw++) {
            float v[8];
            unpack8(sh[wave][(2 * rp + ir) * kDwHW + col + kw], v);
            if (ir < 5) {
                const float* wk = wc + (ir * 5 + kw) * 8;
#pragma unroll
                for (int c = 0; c < 4; c++)
                    a0[c] = __builtin_elementwise_fma(f32x2v{v[2 * c], v[2 * c + 1]},
                                                      f32x2v{wk[2 * c], wk[2 * c + 1]}, a0[c]);
            }
            if (ir >= 1) {
                const float* wk = wc + ((ir - 1) * 5 + kw) * 8;
#pragma unroll
                for (int c = 0; c < 4; c++)
                    a1[c] = __builtin_elementwise_fma(f32x2v{v[2 * c], v[2 * c + 1]},
                                                      f32x2v{wk[2 * c], wk[2 * c + 1]}, a1[c]);
            }
        }
    }
    const int ho = th * kDwTH + 2 * rp, wo = tw * kDwTW + col;
    if (wo >= p.W) return;
    const float* bc = p.b + chunk * 8;
    float o0[8], o1[8];
#pragma unroll
    for (int c = 0; c < 8; c++) {
        o0[c] = act_f(a0[c >> 1][c & 1] + bc[c], p.act);
        o1[c] = act_f(a1[c >> 1][c & 1] + bc[c], p.act);
    }
    uint16_t* yb = p.y + ((size_t)n * p.H * p.W + (size_t)ho * p.W + wo) * p.ys + chunk * 8;
    if (ho < p.H) *reinterpret_cast<uint4*>(yb) = pack8(o0);
    if (ho + 1 < p.H) *reinterpret_cast<uint4*>(yb + (size_t)p.W * p.ys) = pack8(o1);
}

// ------------------------------------------------------------------ depthwise 5x5 + pointwise 1x1
// One CSPNeXtBlock's conv2 (DepthwiseSeparableConvModule: 5x5 depthwise + BN + SiLU, then 1x1
// pointwise + BN + SiLU, + the block's identity) in one launch: the depthwise output never leaves
// LDS.  Unfused, dw5_kernel wrote it (C channels per pixel) and the 1x1 GEMM read it back: 2 x C x
// 2 B per pixel of HBM traffic and a launch per block, ~37 % of the pair's bytes.
// A workgroup owns a TH x TW pixel tile of one frame and all C channels:
//   dw phase   8-channel chunks, 8 per round (one per wave): the round's (TH+4) x (TW+4) halo
//              is loaded coalesced into LDS (8 consecutive 16-B chunks of a pixel per lane
//              group, dw5_kernel's layout), each wave computes its chunk for the tile (1 or 2
//              outputs per lane: dw5_kernel's fma chains, taps in (kh, kw) order, packed
//              channel pairs) and writes the bf16 result straight into the GEMM's B operand;
//   pw phase   the tile x C couts GEMM on v_mfma_f32_16x16x32_bf16 with the B operand resident
//              for all C/32 K steps and the weight image (det_pack_gemm_weights) streamed per K
//              step through a 2-slot LDS ring (register-staged: step q+2 loads under step q);
//              waves split pixel fragments x cout tiles;
//   epilogue   det_conv_gemm_kernel's: bias, SiLU, + residual, bf16.
// Bit-identical to dw5_kernel + det_conv_gemm_kernel<*, 1, 1>: the same per-output fma chains,
// bf16 rounding of the intermediate, LDS operand layouts (row-major 16-B slots with chunk
// kg at kg ^ swz(row)), MFMA operand roles and K order (tests/test_rtmdet_gpu.py).
struct DwPwParams {
    const uint16_t* x;      // depthwise input view (pixel stride xs)
    const float* dw_w;      // [C/8][25][8]
    const float* dw_b;      // [C]
    const uint16_t* wimg;   // pointwise weight image: [C/32 K steps][C couts][4 swizzled 16-B chunks]
    const float* pw_b;      // [C]
    const uint16_t* res;    // residual view (stride rs) or nullptr
    uint16_t* y;            // output view (stride ys)
    int H, W, N, xs, ys, rs, act_dw, act_pw, tiles_w;
};

template <int C, int TH_, int TW>
struct DwPwCfg {
    static constexpr int TH = TH_, P = TH * TW, OUTS = P / 64;  // dw outputs per lane
    static constexpr int HH = TH + 4, HWD = TW + 4;           // halo rows / columns
    static constexpr int Q = C / 32, NCH = C / 8;             // K steps, 8-channel chunks
    static constexpr int FP = P / 16, NT = C / 16;            // pixel fragments, cout tiles
    static constexpr int PWV = FP < 8 ? FP : 8, CWV = 8 / PWV;
    static constexpr int FPW = FP / PWV, TPW = NT / CWV;      // per wave
    static constexpr int B_BYTES = Q * P * 64, A_BYTES = C * 64, H_BYTES = HH * HWD * 8 * 16;
    static constexpr int LDS = B_BYTES + 2 * A_BYTES + H_BYTES;
    static constexpr int AR = (C * 4 + 511) / 512;            // weight chunks per thread and K step
    static_assert(FP % PWV == 0 && NT % CWV == 0 && (OUTS == 1 || OUTS == 2), "dwpw tiling");
};

template <int C, int TH, int TW>
__global__ __launch_bounds__(512, TH == 4 ? 3 : 2) void dwpw_kernel(DwPwParams p) {
    using G = DwPwCfg<C, TH, TW>;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    uint8_t* Bt = lds;                        // [Q][P rows][4 slots]
    uint8_t* At = lds + G::B_BYTES;           // 2 x [C rows][4 slots]
    uint4* halo = reinterpret_cast<uint4*>(lds + G::B_BYTES + 2 * G::A_BYTES);  // [8 chunks][HH * HWD]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int th = blockIdx.x / p.tiles_w, tw = blockIdx.x - th * p.tiles_w;
    const int n = blockIdx.y;
    const int h0 = th * G::TH, w0 = tw * TW;
    auto swz = [](int r) { return (-(r >> 2)) & 3; };
    // weight ring: step q's C x 64 B slab is contiguous in the image
    uint4 wr[G::AR];
    auto load_w = [&](int q) {
#pragma unroll
        for (int j = 0; j < G::AR; j++) {
            const int i = tid + j * 512;
            if (i < C * 4) wr[j] = *reinterpret_cast<const uint4*>(p.wimg + ((size_t)q * C * 4 + i) * 8);
        }
    };
    auto store_w = [&](int slot) {
#pragma unroll
        for (int j = 0; j < G::AR; j++) {
            const int i = tid + j * 512;
            if (i < C * 4) *reinterpret_cast<uint4*>(At + slot * G::A_BYTES + i * 16) = wr[j];
        }
    };
    load_w(0);
    // the epilogue's residual, loaded now so that it lands under the depthwise phase
    const int wp = wave % G::PWV, wc = wave / G::PWV;
    const int kg = lane >> 4, r16 = lane & 15;
    uint2 rsd[G::FPW][G::TPW];
    if (p.res) {
#pragma unroll
        for (int i = 0; i < G::FPW; i++) {
            const int px = (wp * G::FPW + i) * 16 + r16;
            const int h = h0 + px / TW, w = w0 + px % TW;
#pragma unroll
            for (int j = 0; j < G::TPW; j++) {
                const int co = (wc * G::TPW + j) * 16 + kg * 4;
                rsd[i][j] = (h < p.H && w < p.W && co < p.N)
                                ? *reinterpret_cast<const uint2*>(p.res + (((size_t)n * p.H + h) * p.W + w) * p.rs + co)
                                : uint2{0u, 0u};
            }
        }
    }
    // ---- depthwise phase
    const uint16_t* xb = p.x + (size_t)n * p.H * p.W * p.xs;
    typedef float f32x2v __attribute__((ext_vector_type(2)));
#pragma unroll 1
    for (int c0 = 0; c0 < G::NCH; c0 += 8) {
        const int g = min(8, G::NCH - c0);   // chunks this round
        {   // every load of the round in flight before the first LDS write
            constexpr int HR = (G::HH * G::HWD * 8 + 511) / 512;
            uint4 hv[HR];
#pragma unroll
            for (int j = 0; j < HR; j++) {
                const int i = tid + j * 512;
                hv[j] = uint4{0u, 0u, 0u, 0u};
                if (i < G::HH * G::HWD * g) {
                    const int pix = i / g, q = i - pix * g;
                    const int r = pix / G::HWD, c = pix - r * G::HWD;
                    const int hi = h0 - 2 + r, wi = w0 - 2 + c;
                    if (hi >= 0 && hi < p.H && wi >= 0 && wi < p.W)
                        hv[j] = *reinterpret_cast<const uint4*>(xb + ((size_t)hi * p.W + wi) * p.xs + (c0 + q) * 8);
                }
            }
#pragma unroll
            for (int j = 0; j < HR; j++) {
                const int i = tid + j * 512;
                if (i < G::HH * G::HWD * g) {
                    const int pix = i / g, q = i - pix * g;
                    halo[q * G::HH * G::HWD + pix] = hv[j];
                }
            }
        }
        __syncthreads();
        if (wave < g) {
            const int chunk = c0 + wave;
            const float* wc = p.dw_w + (size_t)chunk * 200;
            const float* bc = p.dw_b + chunk * 8;
            const uint4* hq = halo + wave * G::HH * G::HWD;
            const int q = chunk >> 2, kg = chunk & 3;
            if constexpr (G::OUTS == 2) {   // dw5_kernel's lane layout: 2 vertical outputs per lane
                const int col = lane & 15, rp = lane >> 4;
                f32x2v a0[4], a1[4];
#pragma unroll
                for (int c = 0; c < 4; c++) a0[c] = a1[c] = f32x2v{0.f, 0.f};
#pragma unroll 1
                for (int ir = 0; ir < 6; ir++) {
#pragma unroll
                    for (int kw = 0; kw < 5; kw++) {
                        float v[8];
                        unpack8(hq[(2 * rp + ir) * G::HWD + col + kw], v);
                        if (ir < 5) {
                            const float* wk = wc + (ir * 5 + kw) * 8;
#pragma unroll
                            for (int c = 0; c < 4; c++)
                                a0[c] = __builtin_elementwise_fma(f32x2v{v[2 * c], v[2 * c + 1]},
                                                                  f32x2v{wk[2 * c], wk[2 * c + 1]}, a0[c]);
                        }
                        if (ir >= 1) {
                            const float* wk = wc + ((ir - 1) * 5 + kw) * 8;
#pragma unroll
                            for (int c = 0; c < 4; c++)
                                a1[c] = __builtin_elementwise_fma(f32x2v{v[2 * c], v[2 * c + 1]},
                                                                  f32x2v{wk[2 * c], wk[2 * c + 1]}, a1[c]);
                        }
                    }
                }
                float o0[8], o1[8];
#pragma unroll
                for (int c = 0; c < 8; c++) {
                    o0[c] = act_f(a0[c >> 1][c & 1] + bc[c], p.act_dw);
                    o1[c] = act_f(a1[c >> 1][c & 1] + bc[c], p.act_dw);
                }
                const int pa = (2 * rp) * TW + col, pb = pa + TW;
                *reinterpret_cast<uint4*>(Bt + q * G::P * 64 + pa * 64 + ((kg ^ swz(pa)) * 16)) = pack8(o0);
                *reinterpret_cast<uint4*>(Bt + q * G::P * 64 + pb * 64 + ((kg ^ swz(pb)) * 16)) = pack8(o1);
            } else {                          // one output per lane, the same chain (taps in (kh, kw) order)
                const int col = lane % TW, row = lane / TW;
                f32x2v a0[4];
#pragma unroll
                for (int c = 0; c < 4; c++) a0[c] = f32x2v{0.f, 0.f};
#pragma unroll 1
                for (int kh = 0; kh < 5; kh++) {
#pragma unroll
                    for (int kw = 0; kw < 5; kw++) {
                        float v[8];
                        unpack8(hq[(row + kh) * G::HWD + col + kw], v);
                        const float* wk = wc + (kh * 5 + kw) * 8;
#pragma unroll
                        for (int c = 0; c < 4; c++)
                            a0[c] = __builtin_elementwise_fma(f32x2v{v[2 * c], v[2 * c + 1]},
                                                              f32x2v{wk[2 * c], wk[2 * c + 1]}, a0[c]);
                    }
                }
                float o0[8];
#pragma unroll
                for (int c = 0; c < 8; c++) o0[c] = act_f(a0[c >> 1][c & 1] + bc[c], p.act_dw);
                const int pa = row * TW + col;
                *reinterpret_cast<uint4*>(Bt + q * G::P * 64 + pa * 64 + ((kg ^ swz(pa)) * 16)) = pack8(o0);
            }
        }
        __syncthreads();   // the halo is reloaded by the next round
    }
    store_w(0);
    if (G::Q > 1) load_w(1);
    __syncthreads();
    // ---- pointwise phase
    const int soff = r16 * 64 + ((kg ^ swz(r16)) * 16);
    f32x4 acc[G::FPW][G::TPW];
#pragma unroll
    for (int i = 0; i < G::FPW; i++)
#pragma unroll
        for (int j = 0; j < G::TPW; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int q = 0; q < G::Q; q++) {
        const uint8_t* ab = At + (q & 1) * G::A_BYTES;
        const uint8_t* bb = Bt + q * G::P * 64;
        bf16x8 a[G::TPW], b[G::FPW];
#pragma unroll
        for (int j = 0; j < G::TPW; j++)
            a[j] = *reinterpret_cast<const bf16x8*>(ab + ((wc * G::TPW + j) * 16) * 64 + soff);
#pragma unroll
        for (int i = 0; i < G::FPW; i++)
            b[i] = *reinterpret_cast<const bf16x8*>(bb + ((wp * G::FPW + i) * 16) * 64 + soff);
#pragma unroll
        for (int i = 0; i < G::FPW; i++)
#pragma unroll
            for (int j = 0; j < G::TPW; j++)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[j], b[i], acc[i][j], 0, 0, 0);
        if (q + 1 < G::Q) {
            store_w((q + 1) & 1);   // that slot was last read in step q - 1: every wave is past it
            if (q + 2 < G::Q) load_w(q + 2);
        }
        __syncthreads();
    }
    // ---- epilogue (det_conv_gemm_kernel's)
#pragma unroll
    for (int j = 0; j < G::TPW; j++) {
        const int co = (wc * G::TPW + j) * 16 + kg * 4;
        if (co >= p.N) continue;
        const float4 bb = *reinterpret_cast<const float4*>(p.pw_b + co);
#pragma unroll
        for (int i = 0; i < G::FPW; i++) {
            const int px = (wp * G::FPW + i) * 16 + r16;
            const int h = h0 + px / TW, w = w0 + px % TW;
            if (h >= p.H || w >= p.W) continue;
            const size_t m = ((size_t)n * p.H + h) * p.W + w;
            float v[4] = {acc[i][j][0] + bb.x, acc[i][j][1] + bb.y, acc[i][j][2] + bb.z, acc[i][j][3] + bb.w};
            if (p.act_pw == 2)
#pragma unroll
                for (int e = 0; e < 4; e++) v[e] = act_f(v[e], 2);
            if (p.res) {
                const uint2 r = rsd[i][j];
                v[0] += bf(r.x & 0xffff), v[1] += bf(r.x >> 16), v[2] += bf(r.y & 0xffff), v[3] += bf(r.y >> 16);
            }
            if (p.act_pw == 1)
#pragma unroll
                for (int e = 0; e < 4; e++) v[e] = fmaxf(v[e], 0.f);
            *reinterpret_cast<uint2*>(p.y + m * p.ys + co) =
                uint2{tobf(v[0]) | (tobf(v[1]) << 16), tobf(v[2]) | (tobf(v[3]) << 16)};
        }
    }
}

}  // namespace

void launch_det_dw5(const uint16_t* x, int xs, uint16_t* y, int ys, const float* w, const float* b, int n, int H, int W,
                    int C, int act, hipStream_t s) {
    MVP_REQUIRE(C % 32 == 0 && xs % 8 == 0 && ys % 8 == 0, "dw5: channels must be a multiple of 32");
    DwParams p{x, y, w, b, H, W, C, xs, ys, act, (W + kDwTW - 1) / kDwTW};
    // G chunks of 8 channels per workgroup: 8 (128 B of every pixel, one cache line), else 4.
    // (Measured: the 96-channel planes with all 12 chunks per workgroup read 1.37x the
    // algorithmic bytes instead of 2.07x but ran 555 vs 509 us per 80x80 layer of 512 frames,
    // gpurun_out/detbd3: 768-thread workgroups halve the occupancy.  Those planes now run fused,
    // dwpw_kernel.)
    const int G = C % 64 == 0 ? 8 : 4;
    const long blocks = (long)p.tiles_w * ((H + kDwTH - 1) / kDwTH) * (C / (8 * G));
    if (n == 0 || blocks == 0) return;
    MVP_REQUIRE(blocks < (1L << 31) && n < 65536, "dw5: grid too large");
    if (G == 8)
        hipLaunchKernelGGL(dw5_kernel<8>, dim3((unsigned)blocks, (unsigned)n), dim3(512), 0, s, p);
    else
        hipLaunchKernelGGL(dw5_kernel<4>, dim3((unsigned)blocks, (unsigned)n), dim3(256), 0, s, p);
    MVP_HIP(hipGetLastError());
}

template <int C, int TH, int TW>
void launch_dwpw_t(const DwPwParams& p, int n, hipStream_t s) {
    using G = DwPwCfg<C, TH, TW>;
    det_dyn_lds<dwpw_kernel<C, TH, TW>>(G::LDS);
    const int tiles = ((p.H + G::TH - 1) / G::TH) * p.tiles_w;
    hipLaunchKernelGGL((dwpw_kernel<C, TH, TW>), dim3((unsigned)tiles, (unsigned)n), dim3(512), G::LDS, s, p);
}

void launch_det_dwpw(const uint16_t* x, int xs, const float* dw_w, const float* dw_b, const uint16_t* wimg,
                     const float* pw_b, const uint16_t* res, int rs, uint16_t* y, int ys, int n, int H, int W, int C,
                     int N, int act_dw, int act_pw, hipStream_t s) {
    MVP_REQUIRE(det_dwpw_supported(C) && det_cout_pad(N) == C && xs % 8 == 0 && ys % 4 == 0 && (!res || rs % 4 == 0),
                "dwpw: C=%d cout=%d strides %d/%d", C, N, xs, ys);
    if (n == 0) return;
    MVP_REQUIRE(n < 65536 && (long)H * W < (1L << 26), "dwpw: grid too large");
    constexpr int TW = 16;
    DwPwParams p{x, dw_w, dw_b, wimg, pw_b, res, y, H, W, N, xs, ys, rs, act_dw, act_pw, (W + TW - 1) / TW};
    // 4 x 16 tiles: 36-44 KB of LDS, 3 workgroups per CU (8 x 16 tiles: 2 per CU, 83.5 vs 82.0 ms
    // per 512-frame forward same-box, gpurun_out/r06g)
    if (C == 64) launch_dwpw_t<64, 4, TW>(p, n, s);
    else launch_dwpw_t<96, 4, TW>(p, n, s);
    MVP_HIP(hipGetLastError());
}

// Measured per block, 512 frames (gpurun_out/detbd2, detbd3): 64 channels on 160x160 1.93 ms fused
// (4 x 16 tiles) vs 2.73 for dw5 + GEMM; 96 on 80x80 0.90 vs 1.20 (with the identity); with 8 x 8
// tiles 192 on 40x40 1.00 vs 0.68 and 384 on 20x20 1.12 vs 0.38 — the tile re-reads the whole
// C x C weight matrix and too few tiles hide the serial phases — so only 64 and 96 are fused.

}  // namespace mvp
