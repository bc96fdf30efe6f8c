// mvp_heatmap_peaks: up to MVP_MAX_PEAKS local maxima of every heatmap, each decoded as
// decode_kernel (heatmap.hip) decodes its argmax (heatmap_decode.h), so that the multi-view
// geometry can choose among the modes of a bimodal map (mvp_triangulate_peaks).  The contract —
// what a peak is, the order and the filters — is stated in include/mvpose.h.
//
// One wave per map, kWaves maps per workgroup.  A map whose H·W·4 B fits the wave's share of the
// workgroup's LDS budget is staged there (every cell is read up to (2·radius+1)² times); larger
// maps are read from global memory / L2.  Each lane scans the cells lane, lane + 64, ... and keeps
// its best MVP_MAX_PEAKS peaks in registers, ordered; the map's peaks then come out of max_peaks
// rounds of a wave-wide best-of reduction over the lanes' heads, the winning lane popping its own.
#include <cmath>

#include "heatmap_decode.h"

namespace {

constexpr int kWaves = 4;                 // maps per workgroup
constexpr int kPeakBlock = 64 * kWaves;
constexpr int kPeakLds = 64 * 1024;       // dynamic LDS budget of a workgroup: 16 KB = 4096 cells per map
constexpr int kEmpty = 0x7fffffff;        // index of an empty candidate slot

struct PeakParams {
    const float* __restrict__ hm;   // [N][K][H][W]
    const float* __restrict__ cs;   // [N][4] center x, y, scale w, h
    float* __restrict__ peaks;      // [N/V][K][M][3][V]
    int* __restrict__ counts;       // nullable: [N/V][K][V]
    int N, K, H, W, M, radius, V;
    int stride;                     // floats of LDS per wave (0: read the map from global memory)
    int vec;                        // stage with 16-B loads
    float thr, min_rel;
    double in_w, in_h;
};

// cell i = (y, x) with value v is a peak: v > thr, and v beats every other in-bounds cell of
// its window that is no NaN, ties going to the lower flat index
__device__ __forceinline__ bool is_peak(const float* __restrict__ m, int H, int W, int radius, float thr, int i,
                                        int y, int x, float v) {
    if (!(v > thr)) return false;  // NaN included
    const int y0 = max(y - radius, 0), y1 = min(y + radius, H - 1);
    const int x0 = max(x - radius, 0), x1 = min(x + radius, W - 1);
    for (int yy = y0; yy <= y1; yy++)
        for (int xx = x0; xx <= x1; xx++) {
            const int n = yy * W + xx;
            const float u = m[n];
            if (n != i && !(isnan(u) || v > u || (v == u && i < n))) return false;
        }
    return true;
}

__global__ __launch_bounds__(kPeakBlock) void peaks_kernel(PeakParams p) {
    extern __shared__ __attribute__((aligned(16))) float peak_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long map = (long)blockIdx.x * kWaves + wave;
    const bool live = map < (long)p.N * p.K;
    const int HW = p.H * p.W;
    const float* __restrict__ src = p.hm + (live ? map : 0) * HW;
    const float* __restrict__ m = src;
    if (p.stride) {
        float* dst = peak_lds + wave * p.stride;
        if (live) {
            if (p.vec) {
                for (int i = lane * 4; i < HW; i += 256)
                    *reinterpret_cast<float4*>(dst + i) = *reinterpret_cast<const float4*>(src + i);
            } else {
                for (int i = lane; i < HW; i += 64) dst[i] = src[i];
            }
        }
        m = dst;
        __syncthreads();
    }
    if (!live) return;
    // the lane's best peaks, in the `better` order; a lane meets its cells in ascending index,
    // so a new peak goes behind the ones of equal value
    float cv[MVP_MAX_PEAKS];
    int ci[MVP_MAX_PEAKS];
#pragma unroll
    for (int k = 0; k < MVP_MAX_PEAKS; k++) {
        cv[k] = 0.f;
        ci[k] = kEmpty;
    }
    int y = lane / p.W, x = lane - y * p.W;  // (y, x) of i, stepped without divisions
    for (int i = lane; i < HW; i += 64) {
        const float v = m[i];
        if (is_peak(m, p.H, p.W, p.radius, p.thr, i, y, x, v)) {
            float nv = v;
            int ni = i;
            bool ins = false;
#pragma unroll
            for (int k = 0; k < MVP_MAX_PEAKS; k++) {
                ins = ins || ci[k] == kEmpty || nv > cv[k];
                if (ins) {
                    const float tv = cv[k];
                    const int ti = ci[k];
                    cv[k] = nv;
                    ci[k] = ni;
                    nv = tv;
                    ni = ti;
                }
            }
        }
        x += 64;
        while (x >= p.W) {
            x -= p.W;
            y++;
        }
    }
    // round r: the best head of the wave is the map's peak r; lane r keeps it for the write-out
    float mv = 0.f, v0 = 0.f;
    int mi = kEmpty, count = 0;
    for (int r = 0; r < p.M; r++) {
        float bv = cv[0];
        int bi = ci[0];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float ov = __shfl_xor(bv, off);
            const int oi = __shfl_xor(bi, off);
            if (oi != kEmpty && (bi == kEmpty || better(ov, oi, bv, bi))) {
                bv = ov;
                bi = oi;
            }
        }
        if (bi == kEmpty) break;  // wave-uniform
        if (r == 0) v0 = bv;
        else if (!(bv >= __fmul_rn(p.min_rel, v0))) break;  // the later peaks are no larger
        if (ci[0] == bi) {  // the winner pops its head
#pragma unroll
            for (int k = 0; k + 1 < MVP_MAX_PEAKS; k++) {
                cv[k] = cv[k + 1];
                ci[k] = ci[k + 1];
            }
            ci[MVP_MAX_PEAKS - 1] = kEmpty;
        }
        if (lane == r) {
            mv = bv;
            mi = bi;
        }
        count = r + 1;
    }
    const int n = (int)(map / p.K), k = (int)(map - (long)n * p.K);
    const int t = n / p.V, v = n - t * p.V;
    if (lane < p.M) {
        float ox = __builtin_nanf(""), oy = ox, os = 0.f;
        if (lane < count) {
            decode_cell(mi, mv, p.H, p.W, p.in_w, p.in_h, p.cs + 4 * n,
                        [&](int yy, int xx) { return m[yy * p.W + xx]; }, ox, oy);
            os = mv;
        }
        float* o = p.peaks + ((((long)t * p.K + k) * p.M + lane) * 3) * p.V + v;
        o[0] = ox;
        o[p.V] = oy;
        o[2 * p.V] = os;
    }
    if (p.counts && lane == 0) p.counts[((long)t * p.K + k) * p.V + v] = count;
}

}  // namespace

extern "C" int mvp_heatmap_peaks(const float* hm, int N, int K, int H, int W, const float* center_scale, int input_w,
                                 int input_h, int max_peaks, int radius, float thr, float min_rel, int V,
                                 float* peaks, int32_t* counts, void* stream) {
    MVP_ABI_BEGIN
    MVP_REQUIRE(N >= 0 && K > 0 && K <= 32 && H > 0 && W > 0, "mvp_heatmap_peaks: bad sizes (N=%d, K=%d (1..32), H=%d, W=%d)",
                N, K, H, W);
    MVP_REQUIRE((long)H * W <= 65536, "mvp_heatmap_peaks: H*W=%ld > 65536", (long)H * W);
    MVP_REQUIRE(input_w > 0 && input_h > 0, "mvp_heatmap_peaks: bad input size");
    MVP_REQUIRE(max_peaks >= 1 && max_peaks <= MVP_MAX_PEAKS, "mvp_heatmap_peaks: max_peaks=%d (1..%d)", max_peaks,
                MVP_MAX_PEAKS);
    MVP_REQUIRE(radius >= 1 && radius <= 3, "mvp_heatmap_peaks: radius=%d (1..3)", radius);
    MVP_REQUIRE(!std::isnan(thr), "mvp_heatmap_peaks: thr is NaN");
    MVP_REQUIRE(min_rel >= 0.f && min_rel <= 1.f, "mvp_heatmap_peaks: min_rel=%g (0..1)", (double)min_rel);
    MVP_REQUIRE(V >= 1 && N % V == 0, "mvp_heatmap_peaks: N=%d not a multiple of V=%d", N, V);
    if (N == 0) return MVP_OK;
    MVP_REQUIRE(hm && center_scale && peaks, "mvp_heatmap_peaks: NULL device pointer");
    PeakParams p{};
    p.hm = hm;
    p.cs = center_scale;
    p.peaks = peaks;
    p.counts = counts;
    p.N = N;
    p.K = K;
    p.H = H;
    p.W = W;
    p.M = max_peaks;
    p.radius = radius;
    p.V = V;
    p.thr = thr;
    p.min_rel = min_rel;
    p.in_w = input_w;
    p.in_h = input_h;
    const int HW = H * W;
    const int stride = (HW + 3) & ~3;  // whole 16-B rows per wave
    p.stride = (size_t)stride * 4 * kWaves <= (size_t)kPeakLds ? stride : 0;
    p.vec = (HW & 3) == 0 && (reinterpret_cast<uintptr_t>(hm) & 15) == 0;
    const long maps = (long)N * K;
    hipLaunchKernelGGL(peaks_kernel, dim3((unsigned)((maps + kWaves - 1) / kWaves)), dim3(kPeakBlock),
                       (size_t)p.stride * 4 * kWaves, reinterpret_cast<hipStream_t>(stream), p);
    MVP_HIP(hipGetLastError());
    MVP_ABI_END
}
