// Person detector (RTMDet-m) kernels for gfx950: the parts of the network that are not
// dense convolutions (those run on conv_mfma_kernel through launch_conv_generic), plus
// the test pipeline in front of it and the prediction / selection behind it.
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
// This file: launch_det_conv_gemm, which routes a conv to its family (called by detnet.cpp).
#include "det_common.h"

namespace mvp {

void launch_det_conv_gemm(const uint16_t* x, int xs, const uint16_t* w, const float* bias, const uint16_t* res, int rs,
                          uint16_t* y, int ys, int n, int H, int W, int cin, int N, int ks, int stride, int act,
                          hipStream_t s, const uint16_t* wimg, const uint16_t* wband, int live, const DetConvFold* fold) {
    if (live <= 0 || live > N) live = N;
    const int fm = fold ? (fold->up ? 1 : 0) | (fold->ca ? 2 : 0) : 0;
    if (fm) {
        MVP_REQUIRE(wimg && det_fold_shape_ok(H, W, cin, N, ks, fm & 2),
                    "det conv: fold on a conv the fold kernels do not take");
        MVP_REQUIRE(fm != 3, "det conv: one fold per conv");
        MVP_REQUIRE(!(fm & 1) || (H % 2 == 0 && W % 2 == 0 && fold->up_c % 32 == 0 && fold->up_c <= cin &&
                                  fold->up_s % 8 == 0),
                    "det conv: upsample fold shape");
    }
    MVP_REQUIRE(cin % 32 == 0 && N % 4 == 0 && xs % 8 == 0 && ys % 4 == 0 && (!res || rs % 4 == 0),
                "det conv: cin=%d cout=%d strides %d/%d", cin, N, xs, ys);
    MVP_REQUIRE((ks == 1 && stride == 1) || (ks == 3 && (stride == 1 || stride == 2)), "det conv: ks %d stride %d", ks,
                stride);
    const int pad = ks / 2;
    const int Ho = (H + 2 * pad - ks) / stride + 1, Wo = (W + 2 * pad - ks) / stride + 1;
    const int npad = det_cout_pad(N);
    // cout tile: the widest of 192 / 128 / 96 / 64 dividing the padded couts.  Measured
    // alternatives, all slower on RTMDet-m (profiles/r03detcfg.txt, 128 frames, same box):
    // 128-cout tiles 27.2-27.5 vs 25.9 ms, 256-pixel tiles of 8 waves 27.7, of 4 waves 32.6,
    // a 4-slot ring level; removed with their environment switches in round 3.  Round 6
    // re-measured 256-pixel tiles on the <= 40x40 planes' 192-cout convs only (their 128-pixel
    // tiles re-read each weight slice 1.7-6.6x): 84.5 vs 81.2 ms per 512 frames, removed again
    // (profiles/r06_det_wide_live_ab.txt).
    const int bn = det_conv_bn(npad);
    GParams p{x, w, bias, res, y, conv_zero_region(), (long)n * Ho * Wo, cin, N, npad, xs, ys, rs, act,
              (npad + bn - 1) / bn, 0, H, W, Ho, Wo, wimg};
    if (fm) p.up = fold->up, p.up_s = fold->up_s, p.up_c = fold->up_c, p.ca = fold->ca;
    p.xcd_order = det_env("MVPOSE_DET_XCD") != '0';  // A/B: 0 = blockIdx order

    // band-halo kernel for the 3x3/s1 convs with >= 96 input channels on the 80x80 / 40x40
    // planes (det_conv_band_kernel)
    // The kernel splits each XCD's grid/8 workgroups into groups of n_nb (one per cout block):
    // a part with fewer than 8 * n_nb CUs would get no group at all, so it takes the GEMM path.
    // MVPOSE_DET_BAND (tests): 0 = the im2col GEMM kernel, 4 = the band kernel's 4-wave form
    const char band = det_env("MVPOSE_DET_BAND");
    if (wband && det_band_eligible(H, W, cin, npad, ks, stride) &&
        det_band_rows(npad) / kBandBN <= det_band_grid() / 8 && band != '0') {
        det_launch_band(p, n, wband, band == '4', s);
        return;
    }
    // halo-tile kernels for the 32- and 64-channel 3x3/s1 convs (<= 64 couts): 14.03 -> 13.77
    // and 13.90 -> 13.86 ms per 64 frames against the im2col GEMM (same-box tools/det_ab.sh)
    if (ks == 3 && stride == 1 && (cin == 32 || cin == 64) && npad <= 64) {
        det_launch_halo(p, n, live, s);
        return;
    }
    constexpr int kPx = 128;  // pixels per tile: 2 pixel waves x 4 fragments of 16
    const long blocks = (p.M + kPx - 1) / kPx * p.n_nb;
    if (blocks == 0) return;
    MVP_REQUIRE(blocks < (1L << 31), "det conv: grid too large");
    // folds: the persistent 1x1 GEMM, whatever MVPOSE_DET_PERS now says (decided at create)
    if (fm) {
        det_launch_fold(p, fm, blocks, s);
        return;
    }
    // persistent GEMM.  MVPOSE_DET_PERS (A/B and tests): 0 = one tile per workgroup everywhere;
    // 3 = the 3x3 GEMM convs too
    const char pers = det_env("MVPOSE_DET_PERS");
    if (wimg && N <= kPersMaxN && pers != '0' && (ks == 1 || pers == '3')) {
        det_launch_pers(p, ks, stride, blocks, s);
        return;
    }
    det_launch_gemm(p, ks, stride, blocks, s);
}

}  // namespace mvp
