// Person detector, what is not a conv: channel attention, the SPP max pools, nearest-2x upsample,
// the head's predictions, per-frame selection and NMS.  Called by detnet.cpp through det.h, and
// by the C-ABI's mvp_det_nms (below).
#include "det_common.h"

namespace mvp {
namespace {

// ------------------------------------------------------------------ channel attention
// Channel means: kCaSplit workgroups per image each sum a contiguous pixel range (f32
// per-thread partial sums, then an LDS tree) into part[n][split][C]; then one workgroup per
// image adds the splits in order (deterministic), divides by H*W and applies
// s = hardsigmoid(W.mean + b) with W^T [C][C] read coalesced.
constexpr int kCaSplit = 16;

struct CaParams {
    const uint16_t* x;
    const float* wt;  // W^T [k][c]
    const float* b;
    float* part;  // [n][kCaSplit][C]
    float* s;     // [n][C]
    int HW, C, xs;
};

__global__ __launch_bounds__(256) void ca_pool_kernel(CaParams p) {
    extern __shared__ float red[];  // [rows][C]
    const int n = blockIdx.y, sp = blockIdx.x, tid = threadIdx.x;
    const int Q = p.C / 8;
    const int rows = 256 / Q;  // pixel lanes per chunk
    const int q = tid % Q, r = tid / Q;
    const int per = (p.HW + kCaSplit - 1) / kCaSplit;
    const int px0 = sp * per, px1 = min(p.HW, px0 + per);
    const uint16_t* xb = p.x + (size_t)n * p.HW * p.xs + q * 8;
    if (r < rows) {
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int px = px0 + r; px < px1; px += rows) {
            float v[8];
            unpack8(*reinterpret_cast<const uint4*>(xb + (size_t)px * p.xs), v);
#pragma unroll
            for (int c = 0; c < 8; c++) acc[c] += v[c];
        }
#pragma unroll
        for (int c = 0; c < 8; c++) red[r * p.C + q * 8 + c] = acc[c];
    }
    __syncthreads();
    for (int c = tid; c < p.C; c += 256) {
        float sum = 0.f;
        for (int i = 0; i < rows; i++) sum += red[i * p.C + c];
        p.part[((size_t)n * kCaSplit + sp) * p.C + c] = sum;
    }
}

// One 64-lane workgroup per (image, 64 output channels): the C-long dot products keep their
// k order (one fmaf chain per output), with the weights loaded kCaBatch rows at a time ahead
// of the chain; one workgroup per image with one load per fmaf ran ~95 us per call at 128
// images (a load latency per k, half the CUs idle).
constexpr int kCaBatch = 8;

__global__ __launch_bounds__(64) void ca_fc_kernel(CaParams p) {
    extern __shared__ float mean[];  // [C]
    const int n = blockIdx.y, tid = threadIdx.x;
    for (int c = tid; c < p.C; c += 64) {
        float sum = 0.f;
        for (int i = 0; i < kCaSplit; i++) sum += p.part[((size_t)n * kCaSplit + i) * p.C + c];
        mean[c] = sum / (float)p.HW;
    }
    __syncthreads();
    const int c = blockIdx.x * 64 + tid;
    if (c >= p.C) return;
    float a = p.b[c];
    const float* wc = p.wt + c;
    int k = 0;
    for (; k + kCaBatch <= p.C; k += kCaBatch) {
        float w[kCaBatch];
#pragma unroll
        for (int j = 0; j < kCaBatch; j++) w[j] = wc[(size_t)(k + j) * p.C];
#pragma unroll
        for (int j = 0; j < kCaBatch; j++) a = fmaf(w[j], mean[k + j], a);
    }
    for (; k < p.C; k++) a = fmaf(wc[(size_t)k * p.C], mean[k], a);
    p.s[(size_t)n * p.C + c] = fminf(fmaxf(a + 3.f, 0.f), 6.f) / 6.f;
}

__global__ __launch_bounds__(256) void ca_scale_kernel(uint16_t* x, const float* s, int HW, int C, int xs) {
    const int n = blockIdx.y;
    const int Q = C / 8;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)HW * Q) return;
    const int px = (int)(i / Q), q = (int)(i - (long)px * Q);
    uint4* ptr = reinterpret_cast<uint4*>(x + ((size_t)n * HW + px) * xs + q * 8);
    float v[8];
    unpack8(*ptr, v);
    const float* sc = s + (size_t)n * C + q * 8;
#pragma unroll
    for (int c = 0; c < 8; c++) v[c] *= sc[c];
    *ptr = pack8(v);
}

// ------------------------------------------------------------------ SPP max pools
// maxpool 9 = maxpool 5 twice, 13 = three times (stride 1, -inf padding: exact), so one
// workgroup per (image, G 8-channel groups) keeps the plane in LDS and applies the 5x5 max three
// times, writing each result into its slice.  The 5x5 max is a 5-wide row max, then a 5-tall
// column max of those (max is exact and order-free; every value is bf16, so the packed row
// maxima are exact too); the column max overwrites the plane it started from (the row maxima
// are a plane of their own).  G = 4 (round 6): a thread item is one 16-B chunk of a pixel, so a
// pixel's 64 B load and store coalesce and each phase has 6 items per thread instead of 1.6
// (one 8-channel group per workgroup ran 515 us for the 20x20 x 384 SPP of 512 frames).
template <int G>
__global__ __launch_bounds__(256) void spp_kernel(uint16_t* buf, int H, int W, int C, int xs) {
    extern __shared__ uint4 pl[];  // two planes [H*W][G]: the pooled input, its row maxima
    const int cg = blockIdx.x, n = blockIdx.y, tid = threadIdx.x, HW = H * W, NI = HW * G;
    uint16_t* base = buf + (size_t)n * HW * xs + cg * 8 * G;
    uint4* a = pl;
    uint4* r = pl + NI;
    for (int i = tid; i < NI; i += 256) {
        const int px = i / G, g = i - px * G;
        a[i] = *reinterpret_cast<const uint4*>(base + (size_t)px * xs + g * 8);
    }
    for (int k = 1; k <= 3; k++) {
        __syncthreads();
        for (int i = tid; i < NI; i += 256) {
            const int px = i / G, g = i - px * G, y = px / W, x = px - y * W;
            float m[8];
            for (int c = 0; c < 8; c++) m[c] = -__builtin_inff();
            for (int xx = max(x - 2, 0); xx <= min(x + 2, W - 1); xx++) {
                float v[8];
                unpack8(a[(y * W + xx) * G + g], v);
#pragma unroll
                for (int c = 0; c < 8; c++) m[c] = fmaxf(m[c], v[c]);
            }
            r[i] = pack8(m);
        }
        __syncthreads();
        for (int i = tid; i < NI; i += 256) {
            const int px = i / G, g = i - px * G, y = px / W, x = px - y * W;
            float m[8];
            for (int c = 0; c < 8; c++) m[c] = -__builtin_inff();
            for (int yy = max(y - 2, 0); yy <= min(y + 2, H - 1); yy++) {
                float v[8];
                unpack8(r[(yy * W + x) * G + g], v);
#pragma unroll
                for (int c = 0; c < 8; c++) m[c] = fmaxf(m[c], v[c]);
            }
            const uint4 o = pack8(m);
            a[i] = o;
            *reinterpret_cast<uint4*>(base + (size_t)px * xs + k * C + g * 8) = o;
        }
    }
}

// ------------------------------------------------------------------ nearest 2x
__global__ __launch_bounds__(256) void up2_kernel(const uint16_t* x, int xs, uint16_t* y, int ys, int H, int W, int C) {
    const int n = blockIdx.y, Q = C / 8;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;  // output (pixel, chunk)
    if (i >= (long)4 * H * W * Q) return;
    const int px = (int)(i / Q), q = (int)(i - (long)px * Q);
    const int yo = px / (2 * W), xo = px - yo * (2 * W);
    const uint4 v = *reinterpret_cast<const uint4*>(x + ((size_t)n * H * W + (size_t)(yo >> 1) * W + (xo >> 1)) * xs + q * 8);
    *reinterpret_cast<uint4*>(y + ((size_t)n * 4 * H * W + px) * ys + q * 8) = v;
}

// ------------------------------------------------------------------ head predictions
// One thread per pixel of a level: rtm_cls (1) and rtm_reg (4) 1x1 convs on the [cls |
// reg] features (f32 dot products, weights in LDS), sigmoid score, exp(reg) * stride,
// prior (x, y) * stride, distance2bbox clipped to [0, size].
struct HeadParams {
    const uint16_t* x;  // [n][H][W] pixels of xs elements: cls feat at 0, reg feat at F
    const float* w;     // [5][F]
    const float* b;     // [5]
    float* cand;        // [n][n_priors][6]
    int H, W, F, xs, stride, size, n_priors, prior0;
};

__global__ __launch_bounds__(256) void det_head_kernel(HeadParams p) {
#pragma clang fp contract(off)  // box arithmetic rounded op by op, as mmdet's torch ops
    extern __shared__ float swh[];  // [5][F]
    const int n = blockIdx.y, tid = threadIdx.x;
    for (int i = tid; i < 5 * p.F; i += 256) swh[i] = p.w[i];
    __syncthreads();
    const int px = blockIdx.x * 256 + tid;
    if (px >= p.H * p.W) return;
    const uint16_t* xc = p.x + ((size_t)n * p.H * p.W + px) * p.xs;
    const uint16_t* xr = xc + p.F;
    float a[5] = {p.b[0], p.b[1], p.b[2], p.b[3], p.b[4]};
    for (int k = 0; k < p.F; k += 8) {
        float c[8], r[8];
        unpack8(*reinterpret_cast<const uint4*>(xc + k), c);
        unpack8(*reinterpret_cast<const uint4*>(xr + k), r);
#pragma unroll
        for (int j = 0; j < 8; j++) {
            a[0] = fmaf(swh[k + j], c[j], a[0]);
#pragma unroll
            for (int o = 1; o < 5; o++) a[o] = fmaf(swh[o * p.F + k + j], r[j], a[o]);
        }
    }
    const int yy = px / p.W, xx = px - yy * p.W;
    const float s = (float)p.stride;
    const float pxf = (float)xx * s, pyf = (float)yy * s;
    const float d0 = expf(a[1]) * s, d1 = expf(a[2]) * s, d2 = expf(a[3]) * s, d3 = expf(a[4]) * s;
    const float lim = (float)p.size;
    float* out = p.cand + ((size_t)n * p.n_priors + p.prior0 + px) * 6;
    out[0] = 1.f / (1.f + expf(-a[0]));
    out[1] = fminf(fmaxf(pxf - d0, 0.f), lim);
    out[2] = fminf(fmaxf(pyf - d1, 0.f), lim);
    out[3] = fminf(fmaxf(pxf + d2, 0.f), lim);
    out[4] = fminf(fmaxf(pyf + d3, 0.f), lim);
    out[5] = a[0];
}

// The same head with the features staged through LDS: a pixel's [cls | reg] channels sit
// xs elements apart, so one lane per pixel made every 16-B load instruction touch 64 rows
// (2.3 TB/s).  Here the workgroup's 256 pixels x 32 + 32 channels arrive as 64-B runs per
// pixel (coalesced), then each lane runs the same fmaf chains in the same k order.

__global__ __launch_bounds__(256) void det_head_staged_kernel(HeadParams p) {
#pragma clang fp contract(off)  // box arithmetic rounded op by op, as mmdet's torch ops
    extern __shared__ float swh[];  // [5][F], then the pixel block [256][9] uint4
    uint4* sx = reinterpret_cast<uint4*>(swh + ((5 * p.F + 3) & ~3));
    const int n = blockIdx.y, tid = threadIdx.x;
    for (int i = tid; i < 5 * p.F; i += 256) swh[i] = p.w[i];
    const int HW = p.H * p.W, px0 = blockIdx.x * 256;
    const uint16_t* xb = p.x + (size_t)n * HW * p.xs;
    float a[5] = {p.b[0], p.b[1], p.b[2], p.b[3], p.b[4]};
    for (int kc = 0; kc < p.F; kc += kHeadKC) {
        __syncthreads();  // the previous step's block is consumed (and the weights are in)
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int i = tid + 256 * j, pl = i >> 3, q = i & 7;
            const int pg = min(px0 + pl, HW - 1);
            const int ch = q < 4 ? kc + 8 * q : p.F + kc + 8 * (q - 4);
            sx[pl * 9 + q] = *reinterpret_cast<const uint4*>(xb + (size_t)pg * p.xs + ch);
        }
        __syncthreads();
#pragma unroll
        for (int sq = 0; sq < kHeadKC / 8; sq++) {
            const int k = kc + 8 * sq;
            float c[8], r[8];
            unpack8(sx[tid * 9 + sq], c);
            unpack8(sx[tid * 9 + 4 + sq], r);
#pragma unroll
            for (int j = 0; j < 8; j++) {
                a[0] = fmaf(swh[k + j], c[j], a[0]);
#pragma unroll
                for (int o = 1; o < 5; o++) a[o] = fmaf(swh[o * p.F + k + j], r[j], a[o]);
            }
        }
    }
    const int px = px0 + tid;
    if (px >= HW) return;
    const int yy = px / p.W, xx = px - yy * p.W;
    const float s = (float)p.stride;
    const float pxf = (float)xx * s, pyf = (float)yy * s;
    const float d0 = expf(a[1]) * s, d1 = expf(a[2]) * s, d2 = expf(a[3]) * s, d3 = expf(a[4]) * s;
    const float lim = (float)p.size;
    float* out = p.cand + ((size_t)n * p.n_priors + p.prior0 + px) * 6;
    out[0] = 1.f / (1.f + expf(-a[0]));
    out[1] = fminf(fmaxf(pxf - d0, 0.f), lim);
    out[2] = fminf(fmaxf(pyf - d1, 0.f), lim);
    out[3] = fminf(fmaxf(pxf + d2, 0.f), lim);
    out[4] = fminf(fmaxf(pyf + d3, 0.f), lim);
    out[5] = a[0];
}

// ------------------------------------------------------------------ per-frame argmax
// The reference keeps the first detection after mmdet's NMS = the highest-scoring prior
// that passed score_thr and the min-size filter (NMS never removes the top box).  Ties go
// to the lowest prior index (level-major, row-major: the order of a stable sort).
__global__ __launch_bounds__(256) void det_select_kernel(const float* cand, int n_priors, float score_thr, float fx,
                                                         float fy, float* best) {
#pragma clang fp contract(off)
    __shared__ float ss[256];
    __shared__ int si[256];
    const int n = blockIdx.x, tid = threadIdx.x;
    float bs = -1.f;
    int bi = 0x7fffffff;
    for (int i = tid; i < n_priors; i += 256) {
        const float* c = cand + ((size_t)n * n_priors + i) * 6;
        const float s = c[0];
        const float x1 = c[1] * fx, y1 = c[2] * fy, x2 = c[3] * fx, y2 = c[4] * fy;
        if (s > score_thr && x2 - x1 > 0.f && y2 - y1 > 0.f && s > bs) bs = s, bi = i;  // i increases: first max kept
    }
    ss[tid] = bs;
    si[tid] = bi;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {
            const float s2 = ss[tid + w];
            const int i2 = si[tid + w];
            if (s2 > ss[tid] || (s2 == ss[tid] && i2 < si[tid])) ss[tid] = s2, si[tid] = i2;
        }
        __syncthreads();
    }
    if (tid == 0) {
        float* o = best + (size_t)n * 6;
        if (si[0] == 0x7fffffff) {
            o[0] = o[1] = o[2] = o[3] = 0.f;
            o[4] = -1.f;
            o[5] = -1.f;
        } else {
            const float* c = cand + ((size_t)n * n_priors + si[0]) * 6;
            o[0] = c[1] * fx, o[1] = c[2] * fy, o[2] = c[3] * fx, o[3] = c[4] * fy;
            o[4] = ss[0];
            o[5] = (float)si[0];
        }
    }
}

// ------------------------------------------------------------------ NMS (full list)
// One workgroup per frame.  Per level: the priors above score_thr are ranked by
// (score desc, index asc) with a bitonic sort of (score, index) keys in LDS and the best
// nms_pre kept; the survivors of all levels are rescaled, min-size filtered, sorted again
// and suppressed greedily (IoU > iou_thr, mmcv nms with offset 0).
constexpr int kNmsCap = 8192;  // keys per sort (a level's priors; <= 6400 at size 640)

__device__ void bitonic_desc(unsigned long long* k, int n_pow2) {
    for (int size = 2; size <= n_pow2; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int i = threadIdx.x; i < n_pow2; i += blockDim.x) {
                const int j = i ^ stride;
                if (j > i) {
                    const bool up = (i & size) == 0;  // descending in "up" runs
                    const unsigned long long a = k[i], b = k[j];
                    if (up ? a < b : a > b) k[i] = b, k[j] = a;
                }
            }
        }
    __syncthreads();
}

// key: score bits (positive floats order as unsigned) high, inverted index low, so a
// descending sort puts higher score first and, for equal scores, the lower index first
__device__ __forceinline__ unsigned long long nms_key(float s, int i) {
    return ((unsigned long long)__float_as_uint(s) << 32) | (unsigned)(0x7fffffff - i);
}

__global__ __launch_bounds__(1024) void det_nms_kernel(const float* cand, int n_priors, const int* level_off, int n_levels,
                                                       int nms_pre, float score_thr, float iou_thr, int max_det, float fx,
                                                       float fy, float* dets, int* counts) {
#pragma clang fp contract(off)  // rescale / IoU rounded op by op (mmcv nms, offset 0)
    extern __shared__ unsigned long long keys[];  // [kNmsCap]
    __shared__ int n_sel;
    __shared__ int sel[3072];  // kept prior ids over the levels (nms_pre <= 1024 each, <= 3 levels)
    __shared__ float4 bx[3072];
    __shared__ float sc[3072];
    __shared__ unsigned char dead[3072];
    const int n = blockIdx.x, tid = threadIdx.x;
    const float* cn = cand + (size_t)n * n_priors * 6;
    if (tid == 0) n_sel = 0;
    for (int l = 0; l < n_levels; l++) {
        const int lo = level_off[l], cnt = level_off[l + 1] - lo;
        int np2 = 1;
        while (np2 < cnt) np2 <<= 1;
        for (int i = tid; i < np2; i += blockDim.x) {
            const float s = i < cnt ? cn[(size_t)(lo + i) * 6] : 0.f;
            keys[i] = (i < cnt && s > score_thr) ? nms_key(s, lo + i) : 0ull;
        }
        bitonic_desc(keys, np2);
        const int base = n_sel;
        for (int i = tid; i < nms_pre && i < np2; i += blockDim.x)
            if (keys[i] != 0ull) {
                const int idx = 0x7fffffff - (int)(keys[i] & 0xffffffffu);
                sel[base + i] = idx;
            } else {
                sel[base + i] = -1;
            }
        __syncthreads();
        if (tid == 0) {
            int k = base;
            for (int i = 0; i < nms_pre && i < np2; i++)
                if (sel[base + i] >= 0) sel[k++] = sel[base + i];
            n_sel = k;
        }
        __syncthreads();
    }
    const int m = n_sel;
    // rescale + min-size filter, then one global ranking of the survivors
    int np2 = 1;
    while (np2 < m) np2 <<= 1;
    for (int i = tid; i < np2; i += blockDim.x) {
        unsigned long long key = 0ull;
        if (i < m) {
            const float* c = cn + (size_t)sel[i] * 6;
            const float x1 = c[1] * fx, y1 = c[2] * fy, x2 = c[3] * fx, y2 = c[4] * fy;
            bx[i] = float4{x1, y1, x2, y2};
            sc[i] = c[0];
            if (x2 - x1 > 0.f && y2 - y1 > 0.f) key = nms_key(c[0], i);
        }
        keys[i] = key;
    }
    bitonic_desc(keys, np2);
    for (int i = tid; i < m; i += blockDim.x) dead[i] = 0;
    __syncthreads();
    int kept = 0;
    float* out = dets + (size_t)n * max_det * 5;
    for (int a = 0; a < m && kept < max_det; a++) {
        const unsigned long long ka = keys[a];
        if (ka == 0ull) break;
        const int ia = 0x7fffffff - (int)(ka & 0xffffffffu);
        if (dead[a]) continue;  // uniform: every thread reads the same flag after the barrier
        const float4 A = bx[ia];
        if (tid == 0) {
            float* o = out + (size_t)kept * 5;
            o[0] = A.x, o[1] = A.y, o[2] = A.z, o[3] = A.w, o[4] = sc[ia];
        }
        kept++;
        const float area_a = (A.z - A.x) * (A.w - A.y);
        for (int b = a + 1 + tid; b < m; b += blockDim.x) {
            const unsigned long long kb = keys[b];
            if (kb == 0ull || dead[b]) continue;
            const float4 B = bx[0x7fffffff - (int)(kb & 0xffffffffu)];
            const float w = fmaxf(fminf(A.z, B.z) - fmaxf(A.x, B.x), 0.f);
            const float h = fmaxf(fminf(A.w, B.w) - fmaxf(A.y, B.y), 0.f);
            const float inter = w * h;
            const float iou = inter / (area_a + (B.z - B.x) * (B.w - B.y) - inter);
            if (iou > iou_thr) dead[b] = 1;
        }
        __syncthreads();
    }
    if (tid == 0) counts[n] = kept;
}

}  // namespace

void launch_det_ca(uint16_t* x, int xs, int n, int HW, int C, const float* wt, const float* b, float* scratch,
                   hipStream_t s, bool scale_pass) {
    static_assert(kCaSplit == 16, "det_ca_scales (det.h)");
    MVP_REQUIRE(C % 8 == 0 && C / 8 <= 256 && xs % 8 == 0, "ca: C=%d", C);
    const int rows = 256 / (C / 8);
    const size_t lds = (size_t)rows * C * sizeof(float);
    MVP_REQUIRE(lds <= 64 * 1024, "ca: C=%d needs too much LDS", C);
    if (n == 0) return;
    float* part = scratch;                              // [n][kCaSplit][C]
    float* sc = scratch + (size_t)n * kCaSplit * C;     // [n][C]
    CaParams p{x, wt, b, part, sc, HW, C, xs};
    hipLaunchKernelGGL(ca_pool_kernel, dim3(kCaSplit, (unsigned)n), dim3(256), lds, s, p);
    MVP_HIP(hipGetLastError());
    hipLaunchKernelGGL(ca_fc_kernel, dim3((unsigned)((C + 63) / 64), (unsigned)n), dim3(64), (size_t)C * sizeof(float),
                       s, p);
    MVP_HIP(hipGetLastError());
    if (!scale_pass) return;  // folded into the consumer conv (GParams::ca)
    const long work = (long)HW * (C / 8);
    hipLaunchKernelGGL(ca_scale_kernel, dim3((unsigned)((work + 255) / 256), (unsigned)n), dim3(256), 0, s, x, sc, HW,
                       C, xs);
    MVP_HIP(hipGetLastError());
}

void launch_det_spp(uint16_t* buf, int xs, int n, int H, int W, int C, hipStream_t s) {
    MVP_REQUIRE(C % 8 == 0 && xs >= 4 * C && xs % 8 == 0, "spp: C=%d stride=%d", C, xs);
    // two planes of G 16-B chunks per pixel in LDS: with G = 4, H * W <= 1024 (20 x 20 = 400 at the
    // model's 640; 1,024 = the stride-32 plane of a 1,024 x 1,024 input); larger planes or
    // channel counts not a multiple of 32 take G = 1 (H * W <= 2048)
    const int G = (C % 32 == 0 && H * W <= 1024) ? 4 : 1;
    const size_t lds = (size_t)2 * H * W * G * sizeof(uint4);
    MVP_REQUIRE(lds <= 64 * 1024, "spp: %dx%d plane too large (H * W <= 2048)", H, W);
    if (n == 0) return;
    if (G == 4)
        hipLaunchKernelGGL(spp_kernel<4>, dim3((unsigned)(C / 32), (unsigned)n), dim3(256), lds, s, buf, H, W, C, xs);
    else
        hipLaunchKernelGGL(spp_kernel<1>, dim3((unsigned)(C / 8), (unsigned)n), dim3(256), lds, s, buf, H, W, C, xs);
    MVP_HIP(hipGetLastError());
}

void launch_det_up2(const uint16_t* x, int xs, uint16_t* y, int ys, int n, int H, int W, int C, hipStream_t s) {
    MVP_REQUIRE(C % 8 == 0 && xs % 8 == 0 && ys % 8 == 0, "up2: C=%d", C);
    const long work = (long)4 * H * W * (C / 8);
    if (n == 0 || work == 0) return;
    hipLaunchKernelGGL(up2_kernel, dim3((unsigned)((work + 255) / 256), (unsigned)n), dim3(256), 0, s, x, xs, y, ys, H,
                       W, C);
    MVP_HIP(hipGetLastError());
}

void launch_det_head(const uint16_t* x, int xs, int F, const float* w, const float* b, float* cand, int n, int H, int W,
                     int stride, int size, int n_priors, int prior0, bool direct, hipStream_t s) {
    MVP_REQUIRE(F % 8 == 0 && xs >= 2 * F && prior0 + H * W <= n_priors, "det head: shape");
    HeadParams p{x, w, b, cand, H, W, F, xs, stride, size, n_priors, prior0};
    if (n == 0) return;
    const dim3 grid((unsigned)((H * W + 255) / 256), (unsigned)n);
    // direct: one lane per pixel from HBM
    if (!direct)
        hipLaunchKernelGGL(det_head_staged_kernel, grid, dim3(256),
                           (size_t)((5 * F + 3) & ~3) * sizeof(float) + 256 * 9 * sizeof(uint4), s, p);
    else
        hipLaunchKernelGGL(det_head_kernel, grid, dim3(256), (size_t)5 * F * sizeof(float), s, p);
    MVP_HIP(hipGetLastError());
}

void launch_det_select(const float* cand, int n, int n_priors, float score_thr, float fx, float fy, float* best,
                       hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(det_select_kernel, dim3((unsigned)n), dim3(256), 0, s, cand, n_priors, score_thr, fx, fy, best);
    MVP_HIP(hipGetLastError());
}

}  // namespace mvp

extern "C" int mvp_det_nms(const float* cand, int n, int n_priors, const int* level_off, int n_levels, int nms_pre,
                           float score_thr, float iou_thr, int max_det, float fx, float fy, float* dets, int* counts,
                           void* stream) {
    MVP_ABI_BEGIN
    MVP_REQUIRE(n >= 0 && n_levels >= 1 && n_levels <= 3 && level_off, "mvp_det_nms: bad levels");
    MVP_REQUIRE(nms_pre >= 1 && nms_pre <= 1024 && max_det >= 1, "mvp_det_nms: nms_pre must be in [1, 1024]");
    MVP_REQUIRE(level_off[0] == 0 && level_off[n_levels] == n_priors, "mvp_det_nms: level offsets");
    int offs[4];
    for (int l = 0; l <= n_levels; l++) offs[l] = level_off[l];
    for (int l = 0; l < n_levels; l++)
        MVP_REQUIRE(offs[l + 1] > offs[l] && offs[l + 1] - offs[l] <= mvp::kNmsCap, "mvp_det_nms: level %d has %d priors",
                    l, offs[l + 1] - offs[l]);
    if (n == 0) return MVP_OK;
    MVP_REQUIRE(cand && dets && counts, "mvp_det_nms: NULL buffer");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int* d_off = nullptr;
    MVP_HIP(hipMallocAsync((void**)&d_off, sizeof(offs), s));
    MVP_HIP(hipMemcpyAsync(d_off, offs, sizeof(int) * (n_levels + 1), hipMemcpyHostToDevice, s));
    const size_t lds = (size_t)mvp::kNmsCap * sizeof(unsigned long long);
    mvp::det_dyn_lds<mvp::det_nms_kernel>((int)lds);
    hipLaunchKernelGGL(mvp::det_nms_kernel, dim3((unsigned)n), dim3(1024), lds, s, cand, n_priors, d_off, n_levels,
                       nms_pre, score_thr, iou_thr, max_det, fx, fy, dets, counts);
    MVP_HIP(hipGetLastError());
    MVP_HIP(hipFreeAsync(d_off, s));
    MVP_ABI_END
}
