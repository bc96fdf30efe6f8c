// Person detector, in front of the network: the letterbox (mmdet's test pipeline) and the stem
// conv that can stage its rows straight from the raw frames.  Called by detnet.cpp through
// det.h, and by the C-ABI's mvp_det_letterbox (below).
#include "det_common.h"

namespace mvp {
namespace {

// ------------------------------------------------------------------ letterbox
// One thread per output pixel.  cv2.resize INTER_LINEAR on uint8 (OpenCV 4.x
// imgproc/resize.cpp): an exact 2x downscale runs INTER_AREA's fast path,
// (a + b + c + d + 2) >> 2; otherwise fixed-point bilinear with 11-bit coefficients,
// exact int32 horizontal pass and the SIMD vertical rounding
// (((S0 >> 4) * b0 >> 16) + ((S1 >> 4) * b1 >> 16) + 2) >> 2.
struct LbParams {
    const uint8_t* f;
    uint32_t* out;  // [n][S][S] pixels of 4 bf16 (8 B = 2 words)
    int H, W, S, nh, nw, area2;
    double scale_x, scale_y;
    float mean[3], stdv[3];
};

__device__ __forceinline__ void lin_coef(int d, double scale, int n_src, int& s0, int& s1, int& c0, int& c1) {
    float fx = (float)((d + 0.5) * scale - 0.5);
    int sx = (int)floorf(fx);
    fx -= (float)sx;
    if (sx < 0) fx = 0.f, sx = 0;
    if (sx >= n_src - 1) fx = 0.f, sx = n_src - 1;
    c1 = (int)rintf(fx * 2048.f);
    c0 = (int)rintf((1.f - fx) * 2048.f);
    s0 = sx;
    s1 = min(sx + 1, n_src - 1);
}

// normalised bf16 channels of a letterboxed u8 pixel (+ a zero 4th)
__device__ __forceinline__ uint2 lb_pack(const LbParams& p, const int* v) {
    float o[3];
#pragma unroll
    for (int c = 0; c < 3; c++) o[c] = ((float)v[c] - p.mean[c]) / p.stdv[c];
    return uint2{tobf(o[0]) | (tobf(o[1]) << 16), tobf(o[2])};
}

// the u8 channels of letterboxed pixel (y, x) of frame n (114 in the padding)
__device__ __forceinline__ void lb_u8(const LbParams& p, int n, int y, int x, int* v) {
    v[0] = v[1] = v[2] = 114;
    const uint8_t* fr = p.f + (size_t)n * p.H * p.W * 3;
    if (y < p.nh && x < p.nw) {
        if (p.area2) {
            const uint8_t* r0 = fr + ((size_t)(2 * y) * p.W + 2 * x) * 3;
            const uint8_t* r1 = r0 + (size_t)p.W * 3;
#pragma unroll
            for (int c = 0; c < 3; c++) v[c] = (r0[c] + r0[3 + c] + r1[c] + r1[3 + c] + 2) >> 2;
        } else {
            int x0, x1, a0, a1, y0, y1, b0, b1;
            lin_coef(x, p.scale_x, p.W, x0, x1, a0, a1);
            lin_coef(y, p.scale_y, p.H, y0, y1, b0, b1);
            const uint8_t* r0 = fr + (size_t)y0 * p.W * 3;
            const uint8_t* r1 = fr + (size_t)y1 * p.W * 3;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const int h0 = r0[x0 * 3 + c] * a0 + r0[x1 * 3 + c] * a1;
                const int h1 = r1[x0 * 3 + c] * a0 + r1[x1 * 3 + c] * a1;
                const int s = (((h0 >> 4) * b0) >> 16) + (((h1 >> 4) * b1) >> 16);
                v[c] = min(max((s + 2) >> 2, 0), 255);
            }
        }
    }
}

// letterboxed pixel (y, x) of frame n: 3 normalised bf16 channels + a zero 4th
__device__ __forceinline__ uint2 lb_pixel(const LbParams& p, int n, int y, int x) {
    int v[3];
    lb_u8(p, n, y, x, v);
    return lb_pack(p, v);
}

// lb_pack through a table of the 3 x 256 normalised values (the stem's staging: the same
// division, done once per value instead of three times per pixel)
__device__ __forceinline__ uint2 lb_pack_lut(const uint16_t* lut, const int* v) {
    return uint2{(uint32_t)lut[v[0]] | ((uint32_t)lut[256 + v[1]] << 16), (uint32_t)lut[512 + v[2]]};
}

// letterboxed pixels (y, x) and (y, x + 1), x even, of frame n on the INTER_AREA fast path (the
// stem's staging, round 6): their 2 x 2 source blocks are 12 contiguous bytes per source row,
// read as 3 dwords instead of 12 bytes each (needs the row start 4-byte aligned: W % 4 == 0);
// the same integer arithmetic as lb_pixel
__device__ __forceinline__ void lb_pair(const LbParams& p, int n, int y, int x, uint2& o0, uint2& o1,
                                        const uint16_t* lut) {
    if (!p.area2 || (p.W & 3) || y >= p.nh || x + 1 >= p.nw) {
        int v0[3], v1[3];
        lb_u8(p, n, y, x, v0);
        lb_u8(p, n, y, x + 1, v1);
        o0 = lb_pack_lut(lut, v0);
        o1 = lb_pack_lut(lut, v1);
        return;
    }
    const uint8_t* r0 = p.f + ((size_t)n * p.H * p.W + (size_t)(2 * y) * p.W + 2 * x) * 3;
    const uint32_t* w0 = reinterpret_cast<const uint32_t*>(r0);
    const uint32_t* w1 = reinterpret_cast<const uint32_t*>(r0 + (size_t)p.W * 3);
    const uint32_t a[3] = {w0[0], w0[1], w0[2]}, b[3] = {w1[0], w1[1], w1[2]};
    auto byte = [](const uint32_t* w, int i) { return (int)((w[i >> 2] >> ((i & 3) * 8)) & 0xff); };
    int v0[3], v1[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        v0[c] = (byte(a, c) + byte(a, 3 + c) + byte(b, c) + byte(b, 3 + c) + 2) >> 2;
        v1[c] = (byte(a, 6 + c) + byte(a, 9 + c) + byte(b, 6 + c) + byte(b, 9 + c) + 2) >> 2;
    }
    o0 = lb_pack_lut(lut, v0);
    o1 = lb_pack_lut(lut, v1);
}

__global__ __launch_bounds__(256) void letterbox_kernel(LbParams p) {
    const int n = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= p.S * p.S) return;
    const int y = i / p.S, x = i - y * p.S;
    *reinterpret_cast<uint2*>(p.out + ((size_t)n * p.S * p.S + i) * 2) = lb_pixel(p, n, y, x);
}

// ------------------------------------------------------------------ stem conv
// 3x3/s2 conv 4 -> 32 channels (24 real + zero-weight padding) on v_mfma_f32_16x16x32_bf16:
// K = 9 taps x 4 channels = 36 padded to 64.  A workgroup computes two output rows; the
// five input rows they read are staged in LDS with a one-pixel zero border.  A row r of
// cout tile c is cout (r >> 2) * 8 + 4c + (r & 3), so lane group g owns the 8 consecutive
// couts 8g..8g+7 of its pixel (one 16-B store).
// LB (round 6): the five input rows are letterboxed from the raw frames as they are staged
// (lb_pixel: letterbox_kernel's arithmetic), so the letterboxed image is never written or read
// back (the letterbox pass folded into the stem; bit-identical).
template <bool LB>
__global__ __launch_bounds__(256) void det_stem_kernel(const uint16_t* __restrict__ x, const float* __restrict__ w,
                                                       const float* __restrict__ bias, uint16_t* __restrict__ y,
                                                       int S, int act, long n_tiles, LbParams lb) {
    extern __shared__ uint2 sx[];  // [5][S + 2]
    __shared__ uint16_t lut[LB ? 3 * 256 : 1];  // LB: the normalised bf16 of every u8 value
    const int Wo = S / 2, LW = S + 2;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4;
    if constexpr (LB)
        for (int i = tid; i < 3 * 256; i += 256) {
            const int c = i >> 8;
            lut[i] = (uint16_t)tobf(((float)(i & 255) - lb.mean[c]) / lb.stdv[c]);
        }
    bf16x8 afr[2][2];
    float4 b4[2];
#pragma unroll
    for (int c = 0; c < 2; c++) {
        const int r = lane & 15, co = (r >> 2) * 8 + 4 * c + (r & 3);
#pragma unroll
        for (int kc = 0; kc < 2; kc++)
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const int k = kc * 32 + g * 8 + j, tap = k >> 2, ch = k & 3;
                afr[c][kc][j] = (__bf16)(tap < 9 ? w[(co * 9 + tap) * 4 + ch] : 0.f);
            }
        b4[c] = *reinterpret_cast<const float4*>(bias + g * 8 + 4 * c);
    }
    const int tiles = Wo / 2;  // output row pairs per image (Ho = Wo)
    const int n_pt = Wo * 2 / 16;  // 16-pixel tiles per row pair
    for (long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const long n = t / tiles;
        const int ho0 = (int)(t - n * tiles) * 2;
        const uint2* xin = reinterpret_cast<const uint2*>(x) + (size_t)n * S * S;
        __syncthreads();
        if constexpr (LB) {
            // pixel pairs (wi, wi + 1), wi even, of the five rows; the zero border columns apart
            const int PR = S / 2;
            for (int i = tid; i < 5 * PR; i += 256) {
                const int r = i / PR, wi = 2 * (i - r * PR);
                const int hi = 2 * ho0 - 1 + r;
                uint2 o0 = {0u, 0u}, o1 = {0u, 0u};
                if (hi >= 0 && hi < S) lb_pair(lb, (int)n, hi, wi, o0, o1, lut);
                sx[r * LW + wi + 1] = o0;
                sx[r * LW + wi + 2] = o1;
            }
            if (tid < 10) sx[(tid >> 1) * LW + (tid & 1) * (LW - 1)] = uint2{0u, 0u};
        } else {
            for (int i = tid; i < 5 * LW; i += 256) {
                const int r = i / LW, c = i - r * LW;
                const int hi = 2 * ho0 - 1 + r, wi = c - 1;
                const bool in = hi >= 0 && hi < S && wi >= 0 && wi < S;
                sx[i] = in ? xin[(size_t)hi * S + wi] : uint2{0u, 0u};
            }
        }
        __syncthreads();
        for (int pt = wave; pt < n_pt; pt += 4) {
            const int pix = pt * 16 + (lane & 15);
            const int orow = pix / Wo, ocol = pix - orow * Wo;
            auto tap_px = [&](int tap) { return sx[(2 * orow + tap / 3) * LW + 2 * ocol + tap % 3]; };
            const uint2 t0 = tap_px(2 * g), t1 = tap_px(2 * g + 1);
            const uint2 t8 = g == 0 ? tap_px(8) : uint2{0u, 0u};
            union {
                uint4 u;
                bf16x8 v;
            } q0, q1;
            q0.u = uint4{t0.x, t0.y, t1.x, t1.y};
            q1.u = uint4{t8.x, t8.y, 0u, 0u};
            uint32_t o[4];
#pragma unroll
            for (int c = 0; c < 2; c++) {
                f32x4 acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afr[c][0], q0.v, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afr[c][1], q1.v, acc, 0, 0, 0);
                o[2 * c] = tobf(act_f(acc[0] + b4[c].x, act)) | (tobf(act_f(acc[1] + b4[c].y, act)) << 16);
                o[2 * c + 1] = tobf(act_f(acc[2] + b4[c].z, act)) | (tobf(act_f(acc[3] + b4[c].w, act)) << 16);
            }
            uint16_t* out = y + (((size_t)n * Wo + ho0 + orow) * Wo + ocol) * 32 + g * 8;
            *reinterpret_cast<uint4*>(out) = uint4{o[0], o[1], o[2], o[3]};
        }
    }
}

}  // namespace

// ---------------------------------------------------------------------------- launchers
namespace {
LbParams lb_params(const uint8_t* frames, int H, int W, int S, const float* mean3, const float* std3, void* out) {
    int nh, nw;
    det_rescale_size(H, W, S, nh, nw);
    MVP_REQUIRE(nh >= 1 && nw >= 1 && nh <= S && nw <= S, "letterbox: bad size");
    LbParams p{};
    p.f = frames;
    p.out = static_cast<uint32_t*>(out);
    p.H = H, p.W = W, p.S = S, p.nh = nh, p.nw = nw;
    p.scale_x = 1.0 / ((double)nw / W);
    p.scale_y = 1.0 / ((double)nh / H);
    p.area2 = p.scale_x == 2.0 && p.scale_y == 2.0 && W == 2 * nw && H == 2 * nh;
    for (int c = 0; c < 3; c++) p.mean[c] = mean3[c], p.stdv[c] = std3[c];
    return p;
}
}  // namespace

void launch_det_letterbox(const uint8_t* frames, int n, int H, int W, int S, const float* mean3, const float* std3,
                          void* out, hipStream_t s) {
    const LbParams p = lb_params(frames, H, W, S, mean3, std3, out);
    if (n == 0) return;
    hipLaunchKernelGGL(letterbox_kernel, dim3((unsigned)((S * S + 255) / 256), (unsigned)n), dim3(256), 0, s, p);
    MVP_HIP(hipGetLastError());
}

void det_rescale_size(int H, int W, int S, int& nh, int& nw) {
    const double sc = std::min((double)S / std::max(H, W), (double)S / std::min(H, W));
    nh = (int)(H * sc + 0.5);
    nw = (int)(W * sc + 0.5);
}

namespace {
void stem_launch(const uint16_t* x, const float* w, const float* b, uint16_t* y, int n, int S, int act, hipStream_t s,
                 const LbParams* lb) {
    MVP_REQUIRE(S % 16 == 0, "det stem: size %d must be a multiple of 16", S);
    const long n_tiles = (long)n * (S / 4);
    if (n_tiles == 0) return;
    const size_t lds = (size_t)5 * (S + 2) * sizeof(uint2);
    const long grid = std::min<long>(n_tiles, (long)cu_count() * 8);
    if (lb)
        hipLaunchKernelGGL(det_stem_kernel<true>, dim3((unsigned)grid), dim3(256), lds, s, x, w, b, y, S, act, n_tiles, *lb);
    else
        hipLaunchKernelGGL(det_stem_kernel<false>, dim3((unsigned)grid), dim3(256), lds, s, x, w, b, y, S, act, n_tiles,
                           LbParams{});
    MVP_HIP(hipGetLastError());
}
}  // namespace

void launch_det_stem(const uint16_t* x, const float* w, const float* b, uint16_t* y, int n, int S, int act,
                     hipStream_t s) {
    stem_launch(x, w, b, y, n, S, act, s, nullptr);
}

void launch_det_letterbox_stem(const uint8_t* frames, int H, int W, const float* mean3, const float* std3,
                               const float* w, const float* b, uint16_t* y, int n, int S, int act, hipStream_t s) {
    const LbParams lb = lb_params(frames, H, W, S, mean3, std3, nullptr);
    stem_launch(nullptr, w, b, y, n, S, act, s, &lb);
}
}  // namespace mvp

extern "C" int mvp_det_letterbox(const uint8_t* frames, int n, int h, int w, int size, const float* mean3,
                                 const float* std3, void* out, void* stream) {
    MVP_ABI_BEGIN
    MVP_REQUIRE(n >= 0 && h > 0 && w > 0 && size > 0 && mean3 && std3, "mvp_det_letterbox: bad arguments");
    MVP_REQUIRE(n == 0 || (frames && out), "mvp_det_letterbox: NULL buffer");
    mvp::launch_det_letterbox(frames, n, h, w, size, mean3, std3, out, reinterpret_cast<hipStream_t>(stream));
    MVP_ABI_END
}
