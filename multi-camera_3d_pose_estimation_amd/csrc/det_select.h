// The person detector's switches and the kernel each of its launches ends in.  detnet.cpp reads
// the switches once per mvp_det_create and selects every op's kernel there; nothing is re-decided
// per launch, and a switch changed under a live handle changes nothing.  Host-only and free of the
// HIP runtime (tools/kernel_select_check.cpp runs it without a device).
#pragma once
#include <algorithm>

#include "../../include/mvpose.h"  // MVP_DET_*; by its place in the tree, so that -Icsrc alone builds the host check

#ifndef DET_HALO_TR
#define DET_HALO_TR 4  // output rows per halo tile (2, 4 or 8)
#endif

namespace mvp {

// The detector's MVPOSE_DET_* environment switches (A/B runs and tests).  read_det_switches() in
// detnet.cpp is their only reader.  (MVPOSE_DET_DWPW shapes the op list in mvpose/rtmdet.py before
// the library sees it.)
struct DetSwitches {
    bool xcd = true;           // MVPOSE_DET_XCD=0: the GEMM kernel takes its blocks in blockIdx order, not XCD-contiguous
    int band = 1;              // MVPOSE_DET_BAND: 0 = the band convs on the im2col GEMM path, 4 = the band kernel's 4-wave form
    int pers = 1;              // MVPOSE_DET_PERS: 0 = one tile per workgroup everywhere (and no conv folds), 3 = the 3x3 GEMM convs persistent too
    int pers_occ = 2;          // MVPOSE_DET_PERS_OCC=n (atoi, >= 1): the persistent GEMM's workgroups per CU
    bool fold = true;          // MVPOSE_DET_FOLD=0: every producer pass (letterbox, upsample, attention scale) keeps its launch
    bool halo_pers = true;     // MVPOSE_DET_HALO_PERS=0: det_conv_halo_kernel instead of the persistent halo kernel
    bool halo_rows2 = false;   // MVPOSE_DET_HALO_ROWS=2: the halo kernel's 2-row tiles
    bool live = true;          // MVPOSE_DET_LIVE=0: the halo kernel's full 64-cout form for the 48-live-cout convs
    bool head_direct = false;  // MVPOSE_DET_HEAD_DIRECT=1: the head with one lane per pixel reading HBM
};

// The variant a launch runs (mvp_det_kernels' ids).  Cout tile, input chunks, taps, stride and
// plane width are functions of the shape: each family's launcher turns them into template arguments.
enum DetKernel {
    DK_NONE = 0,  // no kernel serves the op: mvp_det_create fails
    // MVP_DET_CONV, in order of preference
    DK_BAND_8W,  // det_conv_band_kernel, 8 waves
    DK_BAND_4W,
    DK_HALO_2ROW,  // det_conv_halo_kernel<.., 2>
    DK_HALO,       // det_conv_halo_kernel<.., DET_HALO_TR>
    DK_HALO_LIVE3,
    DK_HALO_PERS_LT2,  // det_conv_halo_pers_kernel, 2 / 3 / 4 live 16-cout tiles
    DK_HALO_PERS_LT3,
    DK_HALO_PERS_LT4,
    DK_FOLD_UP,  // det_conv1x1_pers_kernel FM 1: the upsample in the pixel DMA
    DK_FOLD_CA,  // ... FM 2: the attention scales applied in LDS
    DK_PERS_GEMM,
    DK_GEMM,
    // MVP_DET_HEAD
    DK_HEAD_STAGED,
    DK_HEAD_DIRECT,
    // MVP_DET_STEM
    DK_LETTERBOX_STEM,  // the letterbox inside the stem
    DK_STEM,
    // one kernel each
    DK_LETTERBOX,
    DK_DW5,
    DK_DWPW,
    DK_CA_POOL,  // MVP_DET_CA's record; the op launches pool, fc and, unless folded, scale
    DK_CA_FC,
    DK_CA_SCALE,
    DK_SPP,
    DK_UP2,
    DK_SELECT,
    DK_COUNT
};

inline const char* det_kernel_name(int k) {
    static const char* const names[DK_COUNT] = {
        "",           "band_8w",       "band_4w",       "halo_2row",     "halo",      "halo_live3",
        "halo_pers_lt2", "halo_pers_lt3", "halo_pers_lt4", "fold_up",    "fold_ca",   "pers_gemm",
        "gemm",       "head_staged",   "head_direct",   "letterbox_stem", "stem",     "letterbox",
        "dw5",        "dwpw",          "ca_pool",       "ca_fc",         "ca_scale",  "spp",
        "up2",        "select"};
    return k > 0 && k < DK_COUNT ? names[k] : "";
}

// What an op's kernel depends on: h x w is the input plane, cin / cout the views' stored channels,
// live the couts with non-zero weights or bias (mvp_det_op.aux of a conv; 0 = all), res whether a
// residual is added.
struct DetOpShape {
    int kind = 0, h = 0, w = 0, cin = 0, cout = 0, ks = 0, stride = 1, live = 0, res = 0;
};
// the producer pass folded into the op (plan_folds): the letterbox into the stem, an upsample or
// an attention's scale pass into a 1x1 conv
enum DetFold { DF_NONE = 0, DF_UP = 1, DF_CA = 2, DF_LETTERBOX = 3 };

constexpr int kPersMaxN = 1024;  // couts whose biases the persistent 1x1 kernel stages in LDS
constexpr int kBandBN = 64;      // couts per work item of the band-halo kernel
constexpr int kGemmPx = 128;     // pixels per GEMM tile: 2 pixel waves x 4 fragments of 16
constexpr int kHeadKC = 32;      // channels of cls and of reg per staging step of the staged head

// Detector conv weights are padded to whole 32-cout rows ([det_cout_pad(cout)][kh][kw][cin]).
inline int det_cout_pad(int cout) { return (cout + 31) / 32 * 32; }
inline bool det_dwpw_supported(int C) { return C == 64 || C == 96; }

// cout tile of the GEMM kernels: the widest of 192 / 128 / 96 / 64 dividing the padded couts, else
// 32.  Measured alternatives, all slower on RTMDet-m (profiles/r03detcfg.txt, 128 frames, same box):
// 128-cout tiles 27.2-27.5 vs 25.9 ms, 256-pixel tiles of 8 waves 27.7, of 4 waves 32.6, a 4-slot
// ring level; removed with their environment switches in round 3.  Round 6 re-measured 256-pixel
// tiles on the <= 40x40 planes' 192-cout convs only (their 128-pixel tiles re-read each weight
// slice 1.7-6.6x): 84.5 vs 81.2 ms per 512 frames, removed again (profiles/r06_det_wide_live_ab.txt).
inline int det_conv_bn(int npad) {
    return npad % 192 == 0 ? 192 : npad % 128 == 0 ? 128 : npad % 96 == 0 ? 96 : npad % 64 == 0 ? 64 : 32;
}
// 128-pixel tiles x cout blocks of a GEMM-path conv over M output pixels
inline long det_gemm_blocks(long M, int npad) {
    const int bn = det_conv_bn(npad);
    return (M + kGemmPx - 1) / kGemmPx * ((npad + bn - 1) / bn);
}

// Whether a conv of this shape runs on the persistent 1x1 GEMM with a fold (`ca`: the scale fold,
// whose tables hold 8 frames per 128-pixel tile): the one predicate of plan_folds and the selection.
inline bool det_fold_shape_ok(int H, int W, int cin, int N, int ks, bool ca) {
    if (ks != 1 || N > kPersMaxN || cin % 32 != 0) return false;
    const int bn = det_conv_bn(det_cout_pad(N));
    if (bn != 192 && bn != 96) return false;  // the instantiated fold kernels
    // a 128-pixel tile's rows span at most 8 frames (the scale table)
    const long hw = (long)H * W;
    return hw > 0 && (!ca || (127 + hw - 1) / hw + 1 <= 8);
}

// The band-halo kernel: 3x3/s1, >= 96 input channels, 80x80 / 40x40 planes, couts in blocks of 64
inline bool det_band_eligible(int H, int W, int cin, int npad, int ks, int stride) {
    return ks == 3 && stride == 1 && H == W && (W == 80 || W == 40) && cin % 32 == 0 && cin / 32 >= 3 &&
           npad % 32 == 0 && npad <= 32 * kBandBN;
}
inline int det_band_rows(int npad) { return (npad + kBandBN - 1) / kBandBN * kBandBN; }  // cout rows of the band image
// the band and persistent kernels' grid unit: one workgroup per CU, a multiple of 8 (the XCD round
// robin of blockIdx)
inline int det_cu_grid(int cus) { return std::max(8, cus / 8 * 8); }

inline DetKernel select_det_conv(const DetOpShape& c, DetFold fold, const DetSwitches& sw, int cus) {
    const int npad = det_cout_pad(c.cout);
    const int live = c.live <= 0 || c.live > c.cout ? c.cout : c.live;
    if ((c.ks != 1 || c.stride != 1) && (c.ks != 3 || (c.stride != 1 && c.stride != 2))) return DK_NONE;
    if (c.cin % 32 != 0 || c.cout % 4 != 0) return DK_NONE;
    if (fold != DF_NONE && (fold == DF_LETTERBOX || !det_fold_shape_ok(c.h, c.w, c.cin, c.cout, c.ks, fold == DF_CA)))
        return DK_NONE;
    // The band kernel splits each XCD's grid/8 workgroups into groups of n_nb (one per cout
    // block): a part with fewer than 8 * n_nb CUs would get no group at all, so it takes the
    // GEMM path.
    if (det_band_eligible(c.h, c.w, c.cin, npad, c.ks, c.stride) &&
        det_band_rows(npad) / kBandBN <= det_cu_grid(cus) / 8 && sw.band != 0)
        return sw.band == 4 ? DK_BAND_4W : DK_BAND_8W;
    // halo-tile kernels for the 32- and 64-channel 3x3/s1 convs (<= 64 couts): 14.03 -> 13.77
    // and 13.90 -> 13.86 ms per 64 frames against the im2col GEMM (same-box tools/det_ab.sh)
    if (c.ks == 3 && c.stride == 1 && (c.cin == 32 || c.cin == 64) && npad <= 64) {
        if (sw.halo_rows2) return DK_HALO_2ROW;
        const bool pers = !c.res && sw.halo_pers;
        if (npad == 64) {
            if (live == 48 && pers) return DK_HALO_PERS_LT3;
            if (live == 64 && pers) return DK_HALO_PERS_LT4;
            // 48 real couts in 64 (RTMDet-m stem.2, stage-1 conv1): 3 live tiles
            if (live <= 48 && live > 32 && !c.res && DET_HALO_TR % 4 == 0 && sw.live) return DK_HALO_LIVE3;
            return DK_HALO;
        }
        // RTMDet-m stem.1 (24 -> 24 couts stored as 32): both 16-cout tiles live
        return c.cin == 32 && live > 16 && pers ? DK_HALO_PERS_LT2 : DK_HALO;
    }
    if (fold == DF_UP) return DK_FOLD_UP;
    if (fold == DF_CA) return DK_FOLD_CA;
    if (c.cout <= kPersMaxN && sw.pers != 0 && (c.ks == 1 || sw.pers == 3)) return DK_PERS_GEMM;
    return DK_GEMM;
}

// The kernel of an op: (shape, fold, switches, CU count) -> variant, in the launchers' order of
// preference.  A folded upsample launches nothing; say so with `fold` on its consumer, not here.
inline DetKernel select_det_kernel(const DetOpShape& c, DetFold fold, const DetSwitches& sw, int cus) {
    switch (c.kind) {
    case MVP_DET_STEM: return fold == DF_LETTERBOX ? DK_LETTERBOX_STEM : DK_STEM;
    case MVP_DET_CONV: return select_det_conv(c, fold, sw, cus);
    case MVP_DET_DW: return c.cin % 32 == 0 ? DK_DW5 : DK_NONE;
    case MVP_DET_DWPW: return det_dwpw_supported(c.cin) && det_cout_pad(c.cout) == c.cin ? DK_DWPW : DK_NONE;
    case MVP_DET_CA: return DK_CA_POOL;
    case MVP_DET_SPP: return DK_SPP;
    case MVP_DET_UP2: return DK_UP2;
    case MVP_DET_HEAD: return (c.cin / 2) % kHeadKC == 0 && !sw.head_direct ? DK_HEAD_STAGED : DK_HEAD_DIRECT;
    }
    return DK_NONE;
}

// Elements of the weight image the op's kernel reads (det_pack_gemm_weights; for the band variants
// det_pack_band_weights); 0: it reads the weight blob itself.
inline long det_image_elems(DetKernel k, const DetOpShape& c) {
    const long K = c.kind == MVP_DET_DWPW ? c.cin : (long)c.ks * c.ks * c.cin;  // dwpw: its pointwise conv
    const int npad = det_cout_pad(c.cout);
    switch (k) {
    case DK_BAND_8W:
    case DK_BAND_4W: return det_band_rows(npad) * K;
    case DK_FOLD_UP:
    case DK_FOLD_CA:
    case DK_PERS_GEMM:
    case DK_GEMM:
    case DK_DWPW: return npad * K;
    default: return 0;
    }
}

}  // namespace mvp
