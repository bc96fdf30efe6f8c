// Device half of the split JPEG decode (jpeg.h): reconstructs frames from the host's per-block
// offsets and quantised coefficients, reproducing libjpeg-turbo's default decode bit for bit —
// dequantisation, jidctint.c's "islow" IDCT, jdsample.c's "fancy" h2v1 / h2v2 upsampling and
// jdcolor.c's fixed-point YCbCr -> RGB, stored BGR — which tests/test_jpeg_gpu.py asserts against
// PIL frame by frame.
//
// Replaces the pixel half of the host decode of Motion-JPEG AVIs and frame<N>.jpg directories
// (the reference's utils.py:851-860); the frames land in HBM, where the 2D stage reads them.
//
// Two kernels.  jpeg_idct_kernel: blocks -> MCU-padded uint8 component planes.  A workgroup of
// 256 threads takes 32 blocks, 8 lanes per block, so a 64-lane wave owns 8 blocks: the lanes
// scatter the block's entries (times the quantiser) into LDS, then each lane runs one column
// and, after the transpose through LDS, one row of the 8x8 IDCT and stores its 8 samples as one
// 8-byte word.  jpeg_bgr_kernel: planes -> BGR; a thread makes 4 pixels of a row (12 bytes),
// interpolating chroma from the planes with the component's REAL size as the edge.  The planes
// are needed between the two because fancy upsampling reads chroma across block and MCU borders.
//
// All arithmetic is 32-bit and wraps (unsigned adds / multiplies, arithmetic shifts), so no
// input has undefined behaviour; it equals libjpeg's whenever the parser's int16 condition holds.
#include <hip/hip_runtime.h>

#include "jpeg.h"
#include "mvp_common.h"

namespace {

using jpeg::Geometry;
using jpeg::Job;

constexpr int CONST_BITS = 13, PASS1_BITS = 2;
constexpr int ROW = 9;          // LDS row pitch of a block, dwords: 8 + 1 pad
constexpr int BLK = 8 * ROW;    // 72 dwords per block: 72 = 8 mod 32

__device__ __forceinline__ int descale(uint32_t x, int n) { return (int)(x + (1u << (n - 1))) >> n; }

// one 8-point pass of jpeg_idct_islow (the even part, then the odd part), results descaled by n
__device__ __forceinline__ void idct8(const int (&d)[8], int (&o)[8], int n) {
    uint32_t z2 = (uint32_t)d[2], z3 = (uint32_t)d[6];
    uint32_t z1 = (z2 + z3) * 4433u;
    uint32_t tmp2 = z1 - z3 * 15137u;
    uint32_t tmp3 = z1 + z2 * 6270u;
    z2 = (uint32_t)d[0];
    z3 = (uint32_t)d[4];
    uint32_t tmp0 = (z2 + z3) << CONST_BITS;
    uint32_t tmp1 = (z2 - z3) << CONST_BITS;
    const uint32_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = (uint32_t)d[7];
    tmp1 = (uint32_t)d[5];
    tmp2 = (uint32_t)d[3];
    tmp3 = (uint32_t)d[1];
    z1 = tmp0 + tmp3;
    z2 = tmp1 + tmp2;
    z3 = tmp0 + tmp2;
    uint32_t z4 = tmp1 + tmp3;
    const uint32_t z5 = (z3 + z4) * 9633u;
    tmp0 *= 2446u;
    tmp1 *= 16819u;
    tmp2 *= 25172u;
    tmp3 *= 12299u;
    z1 = 0u - z1 * 7373u;
    z2 = 0u - z2 * 20995u;
    z3 = 0u - z3 * 16069u + z5;
    z4 = 0u - z4 * 3196u + z5;
    tmp0 += z1 + z3;
    tmp1 += z2 + z4;
    tmp2 += z2 + z3;
    tmp3 += z1 + z4;
    o[0] = descale(tmp10 + tmp3, n);
    o[7] = descale(tmp10 - tmp3, n);
    o[1] = descale(tmp11 + tmp2, n);
    o[6] = descale(tmp11 - tmp2, n);
    o[2] = descale(tmp12 + tmp1, n);
    o[5] = descale(tmp12 - tmp1, n);
    o[3] = descale(tmp13 + tmp0, n);
    o[4] = descale(tmp13 - tmp0, n);
}

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

struct ReconParams {
    const Job* jobs;
    int width, height;
};

__device__ __forceinline__ bool job_ok(const Job& j) {
    return (j.ncomp == 1 && j.hs == 1 && j.vs == 1) ||
           (j.ncomp == 3 && (j.hs == 1 || j.hs == 2) && (j.vs == 1 || (j.vs == 2 && j.hs == 2)));
}

__global__ __launch_bounds__(256) void jpeg_idct_kernel(ReconParams p) {
    const Job job = p.jobs[blockIdx.y];
    if (!job_ok(job)) return;
    const Geometry g = jpeg::geometry(p.width, p.height, job.ncomp, job.hs, job.vs);
    // block lb of the workgroup at ws + 72 lb, its row r at + 9 r: lane (lb, i) touches bank
    // 8 lb + i (+ 9 k) in the column pass and 8 (lb + i) + i (+ k) in the row pass, distinct over
    // a 32-lane half either way
    __shared__ int ws[32 * BLK];
    const int t = threadIdx.x, lb = t >> 3, i = t & 7;
    const int blk = blockIdx.x * 32 + lb;
    const bool live = blk < g.blocks;
    int* w = ws + lb * BLK;
    for (int k = 0; k < 8; k++) w[i * ROW + k] = 0;
    __syncthreads();
    int c = 0, bx = 0, by = 0;
    if (live) {
        const int m = blk / g.per_mcu, j = blk - m * g.per_mcu;
        const int mx = m % g.mcu_w, my = m / g.mcu_w;
        const int nl = g.hs * g.vs;
        c = j < nl ? 0 : j - nl + 1;
        bx = c ? mx : mx * g.hs + j % g.hs;
        by = c ? my : my * g.vs + j / g.hs;
        const uint16_t* q = job.qt + 64 * c;
        const uint32_t lo = job.off[blk];
        const uint32_t hi = min(job.off[blk + 1], lo + 64u);
        for (uint32_t e = lo + (uint32_t)i; e < hi; e += 8) {
            const uint32_t ent = job.coef[e];
            const int pos = (int)(ent >> 16) & 63;
            const int v = (int16_t)(uint16_t)(ent & 0xffff);
            w[(pos >> 3) * ROW + (pos & 7)] = (int)((uint32_t)v * (uint32_t)q[pos]);
        }
    }
    __syncthreads();
    int d[8], o[8];
    if (live) {                                   // pass 1: column i
        for (int k = 0; k < 8; k++) d[k] = w[k * ROW + i];
        idct8(d, o, CONST_BITS - PASS1_BITS);
        for (int k = 0; k < 8; k++) w[k * ROW + i] = o[k];
    }
    __syncthreads();
    if (live) {                                   // pass 2: row i
        for (int k = 0; k < 8; k++) d[k] = w[i * ROW + k];
        idct8(d, o, CONST_BITS + PASS1_BITS + 3);
        uint32_t lo4 = 0, hi4 = 0;
        for (int k = 0; k < 4; k++) {
            lo4 |= (uint32_t)clip8(o[k] + 128) << (8 * k);
            hi4 |= (uint32_t)clip8(o[k + 4] + 128) << (8 * k);
        }
        const int pw = c ? g.pw[1] : g.pw[0];
        const int64_t plane = c == 0 ? 0 : c == 1 ? g.plane[1] : g.plane[2];
        uint8_t* dst = job.planes + plane + (size_t)(8 * by + i) * pw + 8 * bx;
        *reinterpret_cast<uint2*>(dst) = make_uint2(lo4, hi4);
    }
}

// The upsampled chroma sample at luma position (x, y) of plane pl (pitch pw, real size rw x rh).
// jdsample.c: fancy (triangle) filtering only when the component is more than 2 samples wide,
// else replication; the first / last columns and rows have no outside neighbour.
__device__ __forceinline__ int chroma_at(const uint8_t* pl, int pw, int rw, int rh, int hs, int vs, int x, int y) {
    if (hs == 1) return pl[(size_t)y * pw + x];
    const int cx = x >> 1;
    if (rw <= 2) return pl[(size_t)(vs == 2 ? y >> 1 : y) * pw + cx];
    if (vs == 1) {
        const uint8_t* r = pl + (size_t)y * pw;
        const int v = r[cx];
        if (x & 1) return cx == rw - 1 ? v : (3 * v + r[cx + 1] + 2) >> 2;
        return cx == 0 ? v : (3 * v + r[cx - 1] + 1) >> 2;
    }
    const int cy = y >> 1;
    const int ny = (y & 1) ? min(cy + 1, rh - 1) : max(cy - 1, 0);
    const uint8_t* r0 = pl + (size_t)cy * pw;   // nearer row, weight 3
    const uint8_t* r1 = pl + (size_t)ny * pw;
    const int v = 3 * r0[cx] + r1[cx];
    if (x & 1) return cx == rw - 1 ? (4 * v + 7) >> 4 : (3 * v + 3 * r0[cx + 1] + r1[cx + 1] + 7) >> 4;
    return cx == 0 ? (4 * v + 8) >> 4 : (3 * v + 3 * r0[cx - 1] + r1[cx - 1] + 8) >> 4;
}

__global__ __launch_bounds__(256) void jpeg_bgr_kernel(ReconParams p) {
    const Job job = p.jobs[blockIdx.z];
    if (!job_ok(job)) return;
    const Geometry g = jpeg::geometry(p.width, p.height, job.ncomp, job.hs, job.vs);
    const int x0 = 4 * (blockIdx.x * 64 + threadIdx.x), y = blockIdx.y * 4 + threadIdx.y;
    if (x0 >= p.width || y >= p.height) return;
    const uint8_t* py = job.planes + (size_t)y * g.pw[0];
    const int n = min(4, p.width - x0);
    uint8_t px[12];
    for (int k = 0; k < n; k++) {
        const int x = x0 + k;
        const int Y = py[x];
        int r = Y, gg = Y, b = Y;
        if (job.ncomp == 3) {
            const int cb = chroma_at(job.planes + g.plane[1], g.pw[1], g.rw[1], g.rh[1], g.hs, g.vs, x, y) - 128;
            const int cr = chroma_at(job.planes + g.plane[2], g.pw[2], g.rw[2], g.rh[2], g.hs, g.vs, x, y) - 128;
            r = clip8(Y + ((91881 * cr + 32768) >> 16));
            gg = clip8(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
            b = clip8(Y + ((116130 * cb + 32768) >> 16));
        }
        px[3 * k] = (uint8_t)b;
        px[3 * k + 1] = (uint8_t)gg;
        px[3 * k + 2] = (uint8_t)r;
    }
    uint8_t* dst = job.bgr + ((size_t)y * p.width + x0) * 3;
    if (n == 4 && (reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
        uint32_t* d4 = reinterpret_cast<uint32_t*>(dst);
        for (int k = 0; k < 3; k++)
            d4[k] = px[4 * k] | (uint32_t)px[4 * k + 1] << 8 | (uint32_t)px[4 * k + 2] << 16 | (uint32_t)px[4 * k + 3] << 24;
    } else {
        for (int k = 0; k < 3 * n; k++) dst[k] = px[k];
    }
}

}  // namespace

extern "C" int mvp_jpeg_reconstruct(const void* jobs_dev, int n_jobs, int width, int height, void* stream) {
    MVP_ABI_BEGIN
    MVP_REQUIRE(n_jobs >= 0 && n_jobs < 65536, "mvp_jpeg_reconstruct: %d jobs", n_jobs);
    MVP_REQUIRE(width > 0 && height > 0 && width <= 65535 && height <= 65535, "mvp_jpeg_reconstruct: frame %dx%d",
                width, height);
    if (n_jobs == 0) return MVP_OK;
    MVP_REQUIRE(jobs_dev != nullptr, "mvp_jpeg_reconstruct: NULL jobs");
    int blocks = 0;
    int64_t plane_bytes = 0;
    jpeg::worst_case(width, height, &blocks, &plane_bytes);
    const unsigned rows = (unsigned)((height + 3) / 4);
    MVP_REQUIRE(rows < 65536, "mvp_jpeg_reconstruct: frame %dx%d", width, height);
    ReconParams p{static_cast<const Job*>(jobs_dev), width, height};
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((blocks + 31) / 32), (unsigned)n_jobs), dim3(256), 0, s, p);
    MVP_HIP(hipGetLastError());
    hipLaunchKernelGGL(jpeg_bgr_kernel, dim3((unsigned)((width + 255) / 256), rows, (unsigned)n_jobs), dim3(64, 4), 0, s,
                       p);
    MVP_HIP(hipGetLastError());
    MVP_ABI_END
}
