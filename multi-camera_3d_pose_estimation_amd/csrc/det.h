// Internal (not part of the C-ABI): the person detector's (RTMDet-m) kernels for gfx950, as the
// detector graph runtime (detnet.cpp) launches them: the network, the test pipeline in front of it
// and the prediction / selection behind it.  Which kernel an op runs is decided once, at
// mvp_det_create (det_select.h).
//
// Reference: PoseEstimator.predict -> mmdet inference_detector (mmpose_pose_estimation.py
// :98-99, :234-241) and the hand-off rule (:242-250); algorithm restated in
// oracle/rtmdet_ref.py (mmdet / mmcv / cv2 are absent here: parity unpinned).
//
// Layout: bf16 NHWC activations; a "view" is a channel slice [coff, coff + c) of a
// tensor whose pixels are `stride` elements apart, so concatenation is free (producers
// write into their slice of the shared buffer).
//
// One kernel family per file, the helpers they share in det_common.h:
//   det_pre.hip   letterbox, stem                 det_halo.hip  halo tile, persistent halo
//   det_dw.hip    depthwise 5x5, fused dw + pw    det_band.hip  band halo
//   det_gemm.hip  im2col GEMM, persistent GEMM    det_post.hip  attention, SPP, up2, head, NMS
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "det_select.h"

namespace mvp {

// mmcv rescale_size for scale (S, S), keep_ratio: the resized extent of an H x W frame.
void det_rescale_size(int H, int W, int S, int& nh, int& nw);
void launch_det_letterbox(const uint8_t* frames, int n, int H, int W, int S, const float* mean3, const float* std3,
                          void* out, hipStream_t s);
// 3x3/s2 conv 4 -> 32 channels on the letterboxed [n][S][S][4] input, w f32 [32][9][4].
void launch_det_stem(const uint16_t* x, const float* w, const float* b, uint16_t* y, int n, int S, int act,
                     hipStream_t s);
// the letterbox folded into the stem: the stem stages its input rows letterboxed from the raw
// [n][H][W][3] uint8 frames (bit-identical to launch_det_letterbox + launch_det_stem)
void launch_det_letterbox_stem(const uint8_t* frames, int H, int W, const float* mean3, const float* std3,
                               const float* w, const float* b, uint16_t* y, int n, int S, int act, hipStream_t s);
void launch_det_dw5(const uint16_t* x, int xs, uint16_t* y, int ys, const float* w, const float* b, int n, int H, int W,
                    int C, int act, hipStream_t s);
// A conv (1x1, or 3x3 stride 1 / 2, pad ks/2; act as ConvLaunch.relu: 2 = SiLU before the residual,
// 1 = ReLU after it) as every conv kernel family takes it.  detnet.cpp builds it from the op
// (conv_params) and calls the launcher of the family mvp_det_create selected (det_select.h).
struct GParams {
    const uint16_t* x;
    const uint16_t* w;  // [npad][KS*KS*cin]
    const float* bias;  // [npad]
    const uint16_t* res;
    uint16_t* y;
    const uint16_t* zero;  // >= 16 KiB of zeros
    long M;                // n * Ho * Wo
    int cin, N, npad, xs, ys, rs, act, n_nb;
    int xcd_order;         // GEMM kernel: XCD-contiguous logical block order
    int H, W, Ho, Wo;
    // GEMM kernel: w re-laid by det_pack_gemm_weights (per 32-channel K step, every cout's
    // four swizzled 16-B chunks in LDS slot order: a weight DMA instruction reads 1 KB
    // contiguous instead of 16 rows x 64 B); nullptr: gather from w
    const uint16_t* wimg = nullptr;
    // Producer passes folded into a 1x1 conv's pixel DMA on the persistent GEMM (round 6), the
    // producer's own launch skipped, bit-identical to running it: input channels [0, up_c) are the
    // nearest-2x upsample of `up`, an H/2 x W/2 plane with pixel stride up_s (the neck's DET_UP2);
    // `ca`: [n][cin] f32 scales applied to every input channel as it lands (DET_CA's in-place pass)
    const uint16_t* up = nullptr;
    const float* ca = nullptr;
    int up_s = 0, up_c = 0;
};

// Functions shared between the detector's translation units stay out of libmvpose.so's dynamic
// symbols.
#define DET_LOCAL __attribute__((visibility("hidden")))

// The conv families' launchers: each picks its kernel instance from the shape and launches it.
// n: frames (> 0); variant: what mvp_det_create selected; occ: workgroups per CU.
DET_LOCAL void det_launch_band(const GParams& p, int n, const uint16_t* wband, bool waves4, hipStream_t s);  // det_band.hip
DET_LOCAL void det_launch_halo(const GParams& p, int n, DetKernel variant, hipStream_t s);                   // det_halo.hip
DET_LOCAL void det_launch_fold(const GParams& p, DetKernel variant, int occ, hipStream_t s);                 // det_gemm.hip
DET_LOCAL void det_launch_pers(const GParams& p, int ks, int stride, int occ, hipStream_t s);
DET_LOCAL void det_launch_gemm(const GParams& p, int ks, int stride, hipStream_t s);
// A CSPNeXtBlock's depthwise 5x5 (dw_w [C/8][25][8] f32, dw_b [C]) and pointwise 1x1 (wimg: the
// GEMM weight image of the [det_cout_pad(N) == C][C] weights, pw_b [C]) in one launch, the
// intermediate kept in LDS; bit-identical to launch_det_dw5 + the 1x1 GEMM.
void launch_det_dwpw(const uint16_t* x, int xs, const float* dw_w, const float* dw_b, const uint16_t* wimg,
                     const float* pw_b, const uint16_t* res, int rs, uint16_t* y, int ys, int n, int H, int W, int C,
                     int N, int act_dw, int act_pw, hipStream_t s);
// The GEMM kernel's weight image (same element count as w: npad x K, K = ks * ks * cin)
void det_pack_gemm_weights(const uint16_t* w, uint16_t* img, int npad, int K, hipStream_t s);
// The band-halo kernel's weight image (det_band_rows(npad) x K elements)
void det_pack_band_weights(const uint16_t* w, uint16_t* img, int npad, int cin, hipStream_t s);
// channel attention in place; scratch: [n][17][C] f32 (per-split partial sums + scales)
void launch_det_ca(uint16_t* x, int xs, int n, int HW, int C, const float* wt, const float* b, float* scratch,
                   hipStream_t s, bool scale_pass = true);
// the [n][C] scales launch_det_ca leaves in its scratch
inline const float* det_ca_scales(const float* scratch, int n, int C) { return scratch + (size_t)n * 16 * C; }
void launch_det_spp(uint16_t* buf, int xs, int n, int H, int W, int C, hipStream_t s);
void launch_det_up2(const uint16_t* x, int xs, uint16_t* y, int ys, int n, int H, int W, int C, hipStream_t s);
void launch_det_head(const uint16_t* x, int xs, int F, const float* w, const float* b, float* cand, int n, int H, int W,
                     int stride, int size, int n_priors, int prior0, bool direct, hipStream_t s);
void launch_det_select(const float* cand, int n, int n_priors, float score_thr, float fx, float fy, float* best,
                       hipStream_t s);

}  // namespace mvp
