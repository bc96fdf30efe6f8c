// Person detector, conv as GEMM: the im2col GEMM kernel (any 1x1, 3x3/s1 or 3x3/s2 conv), the
// persistent GEMM with its upsample / channel-attention folds, and their weight image.  Launched by
// detnet.cpp through det_launch_fold / _pers / _gemm for the ops whose selected variant
// (det_select.h) is one of theirs; detnet.cpp packs those ops' weights.
#include "det_common.h"

namespace mvp {
namespace {

// ------------------------------------------------------------------ conv = GEMM
// Every detector conv is a GEMM over the flat output-pixel index m = (n, ho, wo):
//   Y[m][cout] = sum_k X~[m][k] W[cout][k],  k = (tap, cin) (weights [cout][kh][kw][cin]),
// X~ the im2col of the NHWC input view, gathered on the fly: K step (tap, 32-channel chunk)
// DMAs, for each of the tile's 128 pixels, the 64 bytes of its tap's input pixel (or zeros
// outside the image) straight into LDS (global_load_lds); a 1x1 conv reads its own pixel.
// Flat pixels need no masking on 20x20 or 40x40 planes, and the same kernel serves the
// stride-2 downsamples.  Workgroup tile: 128 pixels x BN couts, 4 waves as 2 (pixels) x 2
// (couts), operands double-buffered chunk-major in LDS ([k group][row] 16-B slots: every
// 16-lane fragment read is 256 contiguous bytes), the next K step's DMA in flight under
// the current step's MFMAs (v_mfma_f32_16x16x32_bf16).  Epilogue: bias, activation (SiLU
// before the residual, ReLU after it), bf16 stores into the output view.  Workgroups run
// couts-fastest so the blocks sharing an input tile are co-resident (input from HBM once,
// taps from L2).
// PW waves along the pixels (16*FP each) x 2 along the couts: tile 16*FP*PW pixels x BN couts.
// (a 2-slot ring with one chunk per step leaves LDS for three workgroups per CU; FP = 8
// holds a 128 x BN/2 accumulator tile per wave, one wave per SIMD)
template <int BN, int KS, int S, int PW, int NBUF, int CPS, int FP = 4>
__global__ __launch_bounds__(128 * PW, FP == 8 ? 1 : (PW == 2 && NBUF == 2 && CPS == 1) ? 3 : 4 / PW) void
det_conv_gemm_kernel(GParams p) {
    constexpr int NT = 128 * PW;          // threads
    constexpr int NWV = 2 * PW;           // waves
    constexpr int BMP = 16 * FP * PW;     // pixels per tile
    constexpr int A_SLOTS = 4 * BN;       // [kg][cout]
    constexpr int B_SLOTS = 4 * BMP;      // [kg][pix]
    constexpr int SUB = (A_SLOTS + B_SLOTS) * 16;  // one 32-channel K chunk
    constexpr int STAGE = CPS * SUB;      // CPS chunks per ring slot (per barrier)
    constexpr int WCT = BN / 32;          // cout tiles per wave
    constexpr int PAD = KS / 2;
    constexpr int D = NBUF - 1;           // LDS ring: D K steps in flight under the MFMAs
    constexpr int A_R64 = A_SLOTS / 64;   // 64-slot DMA rounds of the weight slice
    static_assert(A_SLOTS % 64 == 0 && B_SLOTS % NT == 0, "slot rounds");
    __shared__ __attribute__((aligned(1024))) uint8_t lds[NBUF * STAGE];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // DMA instructions this wave issues per K step: its weight rounds + the pixel rounds
    const int ops = CPS * ((A_R64 - wave + NWV - 1) / NWV + B_SLOTS / NT);
    const int wp = wave % PW, wc = wave / PW;  // pixel quarter / half, cout half
    // XCD-aware order: the dispatcher deals blockIdx round-robin over the 8 XCDs, so logical
    // blocks (tile, cout block; couts fastest) are renumbered to give every XCD a contiguous
    // range — the cout blocks of a tile then run on one XCD and share its input through that
    // L2 (blockIdx order spread them over n_nb XCDs, each fetching the tile).  A bijection for
    // any grid size: XCD x < r holds q + 1 logical blocks, the others q.
    long lb = blockIdx.x;
    if (p.xcd_order) {
        const long nbk = gridDim.x, q = nbk >> 3, r = nbk & 7, x = blockIdx.x & 7, loc = blockIdx.x >> 3;
        lb = x < r ? x * (q + 1) + loc : r * (q + 1) + (x - r) * q + loc;
    }
    const long tile = lb / p.n_nb;
    const int co0 = (int)(lb - tile * p.n_nb) * BN;
    const long m0 = tile * BMP;
    const int kc = p.cin / 32;            // chunks per tap
    const int nq = KS * KS * kc;          // 32-channel K chunks
    const int K = nq * 32;
    const int nk = (nq + CPS - 1) / CPS;  // ring steps
    // LDS images are row-major with a swizzle: row r (a cout of A, a pixel of B) keeps its
    // four 16-B K chunks (32 channels) in slots 4r .. 4r+3, chunk kg at 4r + (kg ^ swz(r)),
    // swz(r) = -(r >> 2) & 3.  A DMA instruction then reads 16 rows x 64 contiguous bytes
    // (4 lanes per row) instead of 64 rows x 16 B: a quarter of the cache lines per
    // instruction.  The swizzle keeps the 16-lane fragment reads (16 rows, one chunk)
    // conflict-free in every ds_read_b128 lane group.
    auto swz = [](int r) { return (-(r >> 2)) & 3; };
    constexpr int BR = B_SLOTS / NT;  // pixel rounds per thread (FP / 2)
    long bm[BR];
    bool bvalid[BR];
    int bkg[BR], bn_[BR], bho[BR], bwo[BR];
#pragma unroll
    for (int j = 0; j < BR; j++) {
        const int slot = j * NT + tid, row = slot >> 2;
        bkg[j] = (slot & 3) ^ swz(row);
        bm[j] = m0 + row;
        bvalid[j] = bm[j] < p.M;
        bn_[j] = bho[j] = bwo[j] = 0;
        if (KS > 1 && bvalid[j]) {
            const long hw = (long)p.Ho * p.Wo;
            bn_[j] = (int)(bm[j] / hw);
            const int r = (int)(bm[j] - (long)bn_[j] * hw);
            bho[j] = r / p.Wo;
            bwo[j] = r - bho[j] * p.Wo;
        }
    }
    // per-thread DMA sources fixed for the launch: the weight rows of this wave's rounds
    // (advanced by 32 channels per K step), and each pixel's image base (the tap moves it)
    constexpr int ARW = (A_R64 + NWV - 1) / NWV;
    const uint16_t* asrc[ARW];
    const int wstep = p.wimg ? p.npad * 32 : 32;  // elements between K steps of a weight row
#pragma unroll
    for (int j = 0; j < ARW; j++) {
        const int sl = (wave + j * NWV) * 64 + lane;
        const int co = sl >> 2, kg = (sl & 3) ^ swz(co);
        asrc[j] = (co0 + co >= p.npad) ? nullptr
                  : p.wimg             ? p.wimg + ((size_t)co0 * 4 + sl) * 8
                                       : p.w + (size_t)(co0 + co) * K + kg * 8;
    }
    const uint16_t* bimg[BR];
#pragma unroll
    for (int j = 0; j < BR; j++) bimg[j] = p.x + (size_t)bn_[j] * p.H * p.W * p.xs;
    int it_ch = 0, it_kh = 0, it_kw = 0;  // (tap, chunk) of the next issued K step (issued in order)
    // one 32-channel chunk q into sub-slot `base`; chunks past the end DMA zeros (every step
    // issues the same number of operations, which the vmcnt accounting relies on)
    auto issue_chunk = [&](int q, uint8_t* base) {
        const bool live = q < nq;
        const int k0 = q * 32;
#pragma unroll
        for (int j = 0; j < ARW; j++) {
            const int r = wave + j * NWV;
            if (r < A_R64) {  // wave-uniform
                const void* src = (live && asrc[j]) ? (const void*)(asrc[j] + (size_t)q * wstep)
                                                    : (const void*)(p.zero + ((r * 64 + lane) & 1023) * 8);
                glds16_det(src, base + r * 64 * 16);
            }
        }
        int hoff = 0, woff = 0, coff = 0;
        if (KS > 1) {
            hoff = it_kh - PAD, woff = it_kw - PAD, coff = it_ch * 32;
            if (live && ++it_ch == kc) {
                it_ch = 0;
                if (++it_kw == KS) it_kw = 0, it_kh++;
            }
        }
#pragma unroll
        for (int j = 0; j < BR; j++) {
            const uint16_t* px = nullptr;
            if (KS == 1) {
                if (bvalid[j] && live) px = p.x + bm[j] * p.xs + k0;
            } else if (live) {
                const int hi = bho[j] * S + hoff, wi = bwo[j] * S + woff;
                if (bvalid[j] && (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W)
                    px = bimg[j] + ((size_t)hi * p.W + wi) * p.xs + coff;
            }
            const void* src = px ? (const void*)(px + bkg[j] * 8)
                                 : (const void*)(p.zero + ((j * NT + tid) & 1023) * 8);
            glds16_det(src, base + (A_SLOTS + j * NT + wave * 64) * 16);
        }
    };
    auto issue = [&](int k, int buf) {
#pragma unroll
        for (int c = 0; c < CPS; c++) issue_chunk(k * CPS + c, lds + buf * STAGE + c * SUB);
    };
    f32x4 acc[FP][WCT];
#pragma unroll
    for (int i = 0; i < FP; i++)
#pragma unroll
        for (int c = 0; c < WCT; c++) acc[i][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < D && j < nk; j++) issue(j, j);
    wait_vm(ops * (min(D, nk) - 1));  // step 0 landed, the others in flight
    __builtin_amdgcn_s_barrier();
    const int kg = lane >> 4, r16 = lane & 15;
    const int soff = r16 * 64 + ((kg ^ ((-(r16 >> 2)) & 3)) * 16);  // this lane's (row, chunk) in a 16-row block
    int buf = 0;
    for (int k = 0; k < nk; k++) {
        // ring slot (k + D) % NBUF was last read in step k - 1, which every wave has finished
        if (k + D < nk) issue(k + D, buf == 0 ? NBUF - 1 : buf - 1);
#pragma unroll
        for (int cc = 0; cc < CPS; cc++) {
            const uint8_t* base = lds + buf * STAGE + cc * SUB;
            bf16x8 a[WCT], b[FP];
#pragma unroll
            for (int c = 0; c < WCT; c++)
                a[c] = *reinterpret_cast<const bf16x8*>(base + (wc * (BN / 2) + c * 16) * 64 + soff);
#pragma unroll
            for (int i = 0; i < FP; i++)
                b[i] = *reinterpret_cast<const bf16x8*>(base + A_SLOTS * 16 + (wp * 16 * FP + i * 16) * 64 + soff);
#pragma unroll
            for (int i = 0; i < FP; i++)
#pragma unroll
                for (int c = 0; c < WCT; c++)
                    acc[i][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[c], b[i], acc[i][c], 0, 0, 0);
        }
        // step k + 1 must have landed; the steps issued after it may stay in flight.  A plain
        // s_barrier (no release fence: __syncthreads would drain every DMA in flight)
        wait_vm(ops * max(0, min(k + D, nk - 1) - k - 1));
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        buf = buf == NBUF - 1 ? 0 : buf + 1;
    }
    // epilogue: lane holds couts (lane >> 4) * 4 + j of pixel (lane & 15) in each tile
#pragma unroll
    for (int c = 0; c < WCT; c++) {
        const int co = co0 + wc * (BN / 2) + c * 16 + kg * 4;
        if (co >= p.N) continue;
        const float4 bb = *reinterpret_cast<const float4*>(p.bias + co);
#pragma unroll
        for (int i = 0; i < FP; i++) {
            const long m = m0 + wp * 16 * FP + i * 16 + r16;
            if (m >= p.M) continue;
            float v[4] = {acc[i][c][0] + bb.x, acc[i][c][1] + bb.y, acc[i][c][2] + bb.z, acc[i][c][3] + bb.w};
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

// Persistent 1x1 GEMM (round 6).  det_conv_gemm_kernel moves both operands by LDS-DMA; on the
// 1x1 convs (~17 ms of the 512-frame forward) that is ~114 cycles per 1-KiB DMA instruction per
// CU (24.6 GB/s per CU, 6.3 TB/s chip-wide: neck.top_down_blocks.1's main+short conv, 20
// instructions per K step of which 12 are the re-fetched weight slice), the kernels' bound.
// Here the pixel operand (B) still arrives by LDS-DMA into a 3-slot ring, but each wave loads
// its own weight fragments (A) straight into VGPRs with buffer loads (L2-resident, no
// redundancy: PW = 1 puts the 4 waves side by side along the couts, each over all 128 pixels),
// two K steps ahead.  A workgroup per (CU, slot) walks a strided list of (tile, cout block)
// items and the pipeline runs across items.  The epilogue stages each wave's 16-pixel rows in
// LDS and writes whole pixel runs with buffer stores.  Same MFMA operands and sequence (K steps
// 0 .. nq - 1 from zero) and epilogue arithmetic as det_conv_gemm_kernel<BN, 1, 1, ...>:
// bit-identical outputs.
// FM (fold mode): 1 = K channels [0, up_c) read from the nearest-2x upsample's source (the
// neck's DET_UP2 op is not run: the pixel DMA addresses the half-resolution pixel); 2 = the
// channel-attention scale (the DET_CA op's in-place pass is not run): wave 0 DMAs each step's
// table of scales (8 frames x 32 channels, f32) one step ahead, and every thread scales its own
// landed pixel chunks in LDS (f32 product, bf16 round: ca_scale_kernel's arithmetic) before the
// barrier that publishes the step.
template <int BN, int PW, int NBUF, int KS = 1, int STR = 1, int FM = 0>
__global__ __launch_bounds__(256, 2) void det_conv1x1_pers_kernel(GParams p) {
    constexpr int NT = 256, NWV = 4, BMP = 128, D = NBUF - 1;
    constexpr int CWV = NWV / PW;        // waves along the couts
    constexpr int WCO = BN / CWV;        // couts per wave
    constexpr int WCT = WCO / 16;        // 16-cout tiles per wave
    constexpr int FP = BMP / (16 * PW);  // 16-pixel fragments per wave
    constexpr int B_SLOTS = 4 * BMP, SUB = B_SLOTS * 16, BR = B_SLOTS / NT;
    constexpr int ROWB = WCO * 2;        // staged bytes per pixel
    constexpr int OFF_BIAS = NBUF * SUB, OFF_STAGE = OFF_BIAS + kPersMaxN * 4;
    constexpr int OFF_CA = OFF_STAGE + NWV * 16 * ROWB;  // FM & 2: NBUF 1-KiB scale tables
    static_assert(WCO % 16 == 0 && FP * 16 * PW == BMP && B_SLOTS % NT == 0, "tiling");
    static_assert(KS == 1 || FM == 0, "folds: 1x1 only");
    static_assert(!(FM & 2) || BR == 2, "lds_read_ca6: two chunks per thread");
    // one LDS object: with a second __shared__ array the compiler's LDS-DMA alias check put
    // vmcnt(0) in front of every fragment read
    __shared__ __attribute__((aligned(1024))) uint8_t lds[OFF_CA + ((FM & 2) ? NBUF * 1024 : 0)];
    float* bias_s = reinterpret_cast<float*>(lds + OFF_BIAS);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wp = wave % PW, wc = wave / PW;
    const int kc = p.cin / 32;        // 32-channel chunks per tap
    const int nq = KS * KS * kc;      // K steps per item: (tap, chunk), chunks fastest
    // items: logical blocks (tile, cout block; couts fastest) split into 8 contiguous XCD ranges
    // (the dispatcher deals blockIdx round-robin over the XCDs); XCD x's gx workgroups take its
    // range round-robin, so the cout blocks of a tile run side by side on one XCD
    const long nblk = (p.M + BMP - 1) / BMP * p.n_nb;
    const int G = gridDim.x, xcd = blockIdx.x & 7, loc = blockIdx.x >> 3;
    const int gx = G / 8 + (xcd < (G & 7) ? 1 : 0);
    const long qx = nblk >> 3, rx = nblk & 7;
    const long x0 = xcd < rx ? xcd * (qx + 1) : rx * (qx + 1) + (xcd - rx) * qx;
    const long x1 = x0 + qx + (xcd < rx ? 1 : 0);
    const long n_items = x1 - x0 > loc ? (x1 - x0 - loc + gx - 1) / gx : 0;
    const long S = n_items * nq;  // K steps of this workgroup
    if (S == 0) return;           // workgroup-uniform
    for (int i = tid; i < p.N; i += NT) bias_s[i] = p.bias[i];
    auto swz = [](int r) { return (-(r >> 2)) & 3; };
    const int kg = lane >> 4, r16 = lane & 15;
    int b_row[BR], b_kg[BR];
#pragma unroll
    for (int j = 0; j < BR; j++) {
        const int slot = j * NT + tid;
        b_row[j] = slot >> 2;
        b_kg[j] = (slot & 3) ^ swz(b_row[j]);
    }
    // A: lane (kg, r16) of tile c holds chunk kg of cout co0 + wc * WCO + 16c + r16 (the packed
    // image's slot (q * npad + co) * 4 + (kg ^ swz(co)))
    const i32x4 wr = make_rsrc(p.wimg, (int)std::min<long>((long)p.npad * nq * 64, 0x7fffffffL));
    const int a_step = p.npad * 64;  // bytes between K steps of the image
    int a_lane[WCT];                 // this lane's byte offset per tile for co0 = 0 (step 0)
#pragma unroll
    for (int c = 0; c < WCT; c++) {
        const int co = wc * WCO + c * 16 + r16;
        a_lane[c] = co * 64 + ((kg ^ swz(co)) * 16);
    }
    bf16x8 areg[NBUF][WCT];
    // issue K step g (item g / nq, step g % nq): its pixel image into ring slot ST, its weight
    // fragments into areg[ST]
    // the issue stream (steps are issued in order): its item, step in the item and, for 3x3, the
    // tap and chunk of that step and the output pixels (frame, row, column) of this thread's B
    // rows -- advanced per step, so no division in the per-step path
    long i_it = 0, i_tile = 0;
    int i_k = 0, i_co0 = 0, i_ch = 0, i_kw = 0, i_kh = 0;
    int b_n[BR], b_ho[BR], b_wo[BR];
    long b_up[BR];  // FM & 1: the half-resolution source pixel of each B row
    const long hw = (long)p.Ho * p.Wo;
    // FM & 2: first frame of the scale table of the next issued step; its DMA (wave 0): lane l
    // holds the scales of channels 4 (l & 7) .. + 3 of the step's 32, frame n0 + (l >> 3)
    long ca_n0 = 0;
    auto ca_table = [&](int slot, long n0, int kk) {
        const long nfr = p.M / hw;
        const long fr = std::min<long>(n0 + (lane >> 3), nfr - 1);
        glds16_det(p.ca + fr * p.cin + kk * 32 + (lane & 7) * 4, lds + OFF_CA + slot * 1024);
    };
    auto issue = [&](auto Ss) {
        constexpr int ST = decltype(Ss)::value;
        if (i_k == 0) {  // a new item
            const long lb = x0 + loc + i_it * gx;
            i_tile = lb / p.n_nb;
            i_co0 = (int)(lb - i_tile * p.n_nb) * BN;
            if constexpr (KS > 1) {
                const long hw = (long)p.Ho * p.Wo;
#pragma unroll
                for (int j = 0; j < BR; j++) {
                    const long m = i_tile * BMP + b_row[j];
                    b_n[j] = m < p.M ? (int)(m / hw) : -1;
                    const int r = m < p.M ? (int)(m - (long)b_n[j] * hw) : 0;
                    b_ho[j] = r / p.Wo;
                    b_wo[j] = r - b_ho[j] * p.Wo;
                }
            }
            if constexpr ((FM & 1) != 0) {
#pragma unroll
                for (int j = 0; j < BR; j++) {
                    const long m = i_tile * BMP + b_row[j];
                    b_up[j] = 0;
                    if (m < p.M) {
                        const long n = m / hw;
                        const int r = (int)(m - n * hw), h = r / p.W, w = r - h * p.W;
                        b_up[j] = (n * (p.H >> 1) + (h >> 1)) * (p.W >> 1) + (w >> 1);
                    }
                }
            }
        }
        const int k = i_k;
        uint8_t* base = lds + ST * SUB;
        if constexpr (KS == 1) {
#pragma unroll
            for (int j = 0; j < BR; j++) {
                const long m = i_tile * BMP + b_row[j];
                const uint16_t* px = p.x + m * p.xs;
                if constexpr ((FM & 1) != 0)
                    if (k * 32 < p.up_c) px = p.up + b_up[j] * p.up_s;
                const void* src = m < p.M ? (const void*)(px + k * 32 + b_kg[j] * 8)
                                          : (const void*)(p.zero + ((j * NT + tid) & 1023) * 8);
                glds16_det(src, base + (j * NT + wave * 64) * 16);
            }
        } else {
            // the GEMM kernel's K order: chunk fastest, then the tap column, then the tap row
#pragma unroll
            for (int j = 0; j < BR; j++) {
                const int hi = b_ho[j] * STR + i_kh - KS / 2, wi = b_wo[j] * STR + i_kw - KS / 2;
                const bool in = b_n[j] >= 0 && (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W;
                const void* src = in ? (const void*)(p.x + (((long)b_n[j] * p.H + hi) * p.W + wi) * p.xs + i_ch * 32 + b_kg[j] * 8)
                                     : (const void*)(p.zero + ((j * NT + tid) & 1023) * 8);
                glds16_det(src, base + (j * NT + wave * 64) * 16);
            }
            if (++i_ch == kc) {
                i_ch = 0;
                if (++i_kw == KS) i_kw = 0, i_kh++;
            }
        }
#pragma unroll
        for (int c = 0; c < WCT; c++) {
            // couts past npad: an out-of-range offset (the load returns zeros)
            const int off = i_co0 + wc * WCO + c * 16 < p.npad ? k * a_step + i_co0 * 64 + a_lane[c] : 0x7ff00000;
            areg[ST][c] = buffer_load_frag(wr, off);
        }
        if (++i_k == nq) i_k = 0, i_it++, i_kh = 0;
        if constexpr ((FM & 2) != 0) {  // the next step's scale table (wave 0; clamped past the end)
            if (i_k == 0) ca_n0 = (x0 + loc + i_it * gx) / p.n_nb * BMP / hw;
            if (wave == 0) ca_table((ST + 1) % NBUF, ca_n0, i_k);
        }
    };
    // vector memory instructions per issued step (this wave)
    const int OPS = BR + WCT + ((FM & 2) != 0 && wave == 0 ? 1 : 0);
    // FM & 2: scale this thread's two landed chunks of the step in ring slot `slot` (its own
    // DMAs; the step's table landed one barrier earlier), in the consumption order of the steps
    int sc_k = 0, sc_fs[BR];
    long sc_it = 0;
    auto ca_scale = [&](int slot) {
        if (sc_k == 0) {
            const long tile = (x0 + loc + sc_it * gx) / p.n_nb;
            const long n0 = tile * BMP / hw;
#pragma unroll
            for (int j = 0; j < BR; j++) {
                const long m = tile * BMP + b_row[j];
                sc_fs[j] = m < p.M ? (int)(m / hw - n0) : 0;
            }
        }
        uint8_t* d0 = lds + slot * SUB + tid * 16;
        uint8_t* d1 = d0 + NT * 16;
        const uint8_t* tb = lds + OFF_CA + slot * 1024;
        u32x4 v[2];
        f32x4 sc[2][2];
        lds_read_ca6(d0, d1, tb + sc_fs[0] * 128 + b_kg[0] * 32, tb + sc_fs[1] * 128 + b_kg[1] * 32, v[0], v[1],
                     sc[0][0], sc[0][1], sc[1][0], sc[1][1]);
#pragma unroll
        for (int j = 0; j < 2; j++) {
            float f[8];
            unpack8(uint4{v[j][0], v[j][1], v[j][2], v[j][3]}, f);
#pragma unroll
            for (int e = 0; e < 4; e++) f[e] *= sc[j][0][e], f[4 + e] *= sc[j][1][e];
            const uint4 o = pack8(f);
            lds_write_u4(j ? d1 : d0, u32x4{o.x, o.y, o.z, o.w});
        }
        if (++sc_k == nq) sc_k = 0, sc_it++;
    };
    f32x4 acc[FP][WCT];
#pragma unroll
    for (int i = 0; i < FP; i++)
#pragma unroll
        for (int c = 0; c < WCT; c++) acc[i][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr ((FM & 2) != 0) {  // step 0's scale table, published before the first issue
        ca_n0 = (x0 + loc) / p.n_nb * BMP / hw;
        if (wave == 0) ca_table(0, ca_n0, 0);
        wait_vm(0);
        __builtin_amdgcn_s_barrier();
    }
    static_for<0, D>([&](auto J) {
        if (J < S) issue(J);
    });
    wait_vm(OPS * (int)(std::min<long>(D, S) - 1));
    if constexpr ((FM & 2) != 0) {
        ca_scale(0);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    const int soff = r16 * 64 + ((kg ^ ((-(r16 >> 2)) & 3)) * 16);
    uint8_t* stage = lds + OFF_STAGE + wave * 16 * ROWB;  // this wave's epilogue rows
    int k = 0;
    long it = 0;
    unsigned ends = 0;  // bit t: iteration g - 1 - t ran an epilogue
    constexpr int kStores = FP * ((2 * WCO + 63) / 64);  // store instructions per epilogue (this wave)
    auto step = [&](long g, auto Ss) {
        constexpr int ST = decltype(Ss)::value;
        if (g + D < S) issue(std::integral_constant<int, (ST + D) % NBUF>{});
        {
            // this step's weight fragments landed at the previous step's wait (the asm loads are
            // invisible to the compiler): tell it so here, before their first use
#pragma unroll
            for (int c = 0; c < WCT; c++) asm volatile("" : "+v"(areg[ST][c]));
            const uint8_t* base = lds + ST * SUB;
            bf16x8 b[FP];
#pragma unroll
            for (int i = 0; i < FP; i++) b[i] = *reinterpret_cast<const bf16x8*>(base + (wp * 16 * FP + i * 16) * 64 + soff);
#pragma unroll
            for (int i = 0; i < FP; i++)
#pragma unroll
                for (int c = 0; c < WCT; c++)
                    acc[i][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(areg[ST][c], b[i], acc[i][c], 0, 0, 0);
        }
        // step g + 1 landed (pixels and weights): younger are the later steps' operations and
        // the stores of the epilogues run since its issue (iterations g + 1 - D .. g - 1).  Loads,
        // stores and LDS-DMA retire in issue order, so counting the stores keeps their slow write
        // acknowledgements off this wait.
        wait_vm(OPS * (int)(std::min<long>(g + D, S - 1) - g - 1) + kStores * __builtin_popcount(ends & ((1u << (D - 1)) - 1)));
        ends <<= 1;
        if constexpr ((FM & 2) != 0)
            if (g + 1 < S) ca_scale((ST + 1) % NBUF);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (++k < nq) return;
        // ---- the item's epilogue (det_conv_gemm_kernel's arithmetic), a fresh accumulator
        const long lb = x0 + loc + it * gx;
        const long tile = lb / p.n_nb;
        const int co0 = (int)(lb - tile * p.n_nb) * BN;
        const long m0 = tile * BMP;
        float4 bb[WCT];
#pragma unroll
        for (int c = 0; c < WCT; c++) {
            const int co = co0 + wc * WCO + c * 16 + kg * 4;
            bb[c] = lds_read_f4_sync(bias_s + (co < p.N ? co : 0));
        }
        // buffer stores: lanes past the couts / pixels get an out-of-range offset and are dropped
        const long mv = p.M - m0;
        const i32x4 yr = make_rsrc(p.y + m0 * p.ys, (int)((mv < BMP ? mv : BMP) * p.ys * 2));
#pragma unroll
        for (int i = 0; i < FP; i++) {
            const long mi = m0 + wp * 16 * FP + i * 16;
#pragma unroll
            for (int c = 0; c < WCT; c++) {
                const int co = co0 + wc * WCO + c * 16 + kg * 4;
                const long m = mi + r16;
                float v[4] = {acc[i][c][0] + bb[c].x, acc[i][c][1] + bb[c].y, acc[i][c][2] + bb[c].z,
                              acc[i][c][3] + bb[c].w};
                acc[i][c] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (p.act == 2)
#pragma unroll
                    for (int e = 0; e < 4; e++) v[e] = act_f(v[e], 2);
                if (p.res && co < p.N && m < p.M) {
                    const uint2 r = *reinterpret_cast<const uint2*>(p.res + m * p.rs + co);
                    v[0] += bf(r.x & 0xffff), v[1] += bf(r.x >> 16), v[2] += bf(r.y & 0xffff), v[3] += bf(r.y >> 16);
                }
                if (p.act == 1)
#pragma unroll
                    for (int e = 0; e < 4; e++) v[e] = fmaxf(v[e], 0.f);
                lds_write_u2(stage + r16 * ROWB + (c * 16 + kg * 4) * 2,
                             uint2{tobf(v[0]) | (tobf(v[1]) << 16), tobf(v[2]) | (tobf(v[3]) << 16)});
            }
            // the wave's 16 pixels x WCO couts back as 16-B row chunks: a store instruction writes
            // whole ROWB-byte pixel runs instead of 16 runs of 32 B
            constexpr int NCH = 16 * ROWB / 16;
#pragma unroll
            for (int q0 = 0; q0 < NCH; q0 += 64) {
                const int q = min(q0 + lane, NCH - 1);
                const int px = q / (ROWB / 16), ch = q - px * (ROWB / 16);
                const u32x4 o = lds_read_u4_sync(stage + q * 16);
                const int co = co0 + wc * WCO + ch * 8;
                const bool ok = q0 + lane < NCH && co < p.N;
                const int off = ok ? ((wp * 16 * FP + i * 16 + px) * p.ys + co) * 2 : 0x7ff00000;
                buffer_store_u4(o, yr, off);
            }
        }
        ends |= 1;
        k = 0;
        it++;
    };
    for (long g = 0; g < S; g += NBUF)
        static_for<0, NBUF>([&](auto J) {
            if (g + J < S) step(g + J, J);
        });
}

}  // namespace

__global__ __launch_bounds__(256) void det_pack_gemm_kernel(const uint16_t* __restrict__ w, uint16_t* __restrict__ img,
                                                          int npad, int K) {
    const long n = (long)npad * K / 8;  // 16-B slots
    for (long d = blockIdx.x * 256L + threadIdx.x; d < n; d += (long)gridDim.x * 256) {
        const long qc = d >> 2;  // (K step, cout)
        const int c = (int)(d & 3), co = (int)(qc % npad), q = (int)(qc / npad);
        const int kg = c ^ ((-(co >> 2)) & 3);  // the GEMM kernel's swz(co): co0 is a multiple of 16
        *reinterpret_cast<uint4*>(img + d * 8) =
            *reinterpret_cast<const uint4*>(w + (size_t)co * K + (size_t)q * 32 + kg * 8);
    }
}

void det_pack_gemm_weights(const uint16_t* w, uint16_t* img, int npad, int K, hipStream_t s) {
    MVP_REQUIRE(npad % 32 == 0 && K % 32 == 0, "det_pack_gemm_weights: npad %d, K %d", npad, K);
    hipLaunchKernelGGL(det_pack_gemm_kernel, dim3(512), dim3(256), 0, s, w, img, npad, K);
    MVP_HIP(hipGetLastError());
}

namespace {
// the cout tile det_conv_bn chose, as a constant: f(det_int<BN>)
template <typename F>
void by_bn(int bn, F&& f) {
    if (bn == 192) f(det_int<192>{});
    else if (bn == 128) f(det_int<128>{});
    else if (bn == 96) f(det_int<96>{});
    else if (bn == 64) f(det_int<64>{});
    else f(det_int<32>{});
}

// the conv's taps and stride (1x1, 3x3/s1 or 3x3/s2), as constants: f(det_int<KS>, det_int<STRIDE>)
template <typename F>
void by_ks_stride(int ks, int stride, F&& f) {
    if (ks == 1) f(det_int<1>{}, det_int<1>{});
    else if (stride == 1) f(det_int<3>{}, det_int<1>{});
    else f(det_int<3>{}, det_int<2>{});
}

// the persistent kernel's waves along the pixels for a cout tile (96 and 32: 2 x 2 waves)
template <int BN>
constexpr int kPersPW = (BN == 96 || BN == 32) ? 2 : 1;

// the persistent GEMM's grid over the conv's (tile, cout block) items, occ workgroups per CU
dim3 pers_grid(const GParams& p, int occ) { return dim3((unsigned)det_pers_grid(det_gemm_blocks(p.M, p.npad), occ)); }
}  // namespace

void det_launch_fold(const GParams& p, DetKernel variant, int occ, hipStream_t s) {
    const dim3 grid = pers_grid(p, occ);
    by_bn(det_conv_bn(p.npad), [&](auto bn) {
        constexpr int BN = decltype(bn)::value, PW = kPersPW<BN>;
        if constexpr (BN == 192 || BN == 96) {  // the instantiated fold kernels (det_fold_shape_ok)
            if (variant == DK_FOLD_UP) hipLaunchKernelGGL((det_conv1x1_pers_kernel<BN, PW, 3, 1, 1, 1>), grid, dim3(256), 0, s, p);
            else hipLaunchKernelGGL((det_conv1x1_pers_kernel<BN, PW, 3, 1, 1, 2>), grid, dim3(256), 0, s, p);
        }
    });
    MVP_HIP(hipGetLastError());
}

void det_launch_pers(const GParams& p, int ks, int stride, int occ, hipStream_t s) {
    const dim3 grid = pers_grid(p, occ);
    by_ks_stride(ks, stride, [&](auto k, auto st) {
        by_bn(det_conv_bn(p.npad), [&](auto bn) {
            constexpr int BN = decltype(bn)::value, KS = decltype(k)::value, STR = decltype(st)::value;
            hipLaunchKernelGGL((det_conv1x1_pers_kernel<BN, kPersPW<BN>, 3, KS, STR>), grid, dim3(256), 0, s, p);
        });
    });
    MVP_HIP(hipGetLastError());
}

void det_launch_gemm(const GParams& p, int ks, int stride, hipStream_t s) {
    const long blocks = det_gemm_blocks(p.M, p.npad);
    by_ks_stride(ks, stride, [&](auto k, auto st) {
        by_bn(det_conv_bn(p.npad), [&](auto bn) {
            constexpr int BN = decltype(bn)::value, KS = decltype(k)::value, STR = decltype(st)::value;
            hipLaunchKernelGGL((det_conv_gemm_kernel<BN, KS, STR, 2, 3, 1>), dim3((unsigned)blocks), dim3(256), 0, s, p);
        });
    });
    MVP_HIP(hipGetLastError());
}

}  // namespace mvp
