// MSRAHeatmap decode arithmetic shared by decode_kernel (heatmap.hip) and peaks_kernel
// (heatmap_peaks.hip): the order in which two cells of a map compare, and the way a chosen cell
// becomes an image-pixel keypoint.  One copy, so a peak decodes to the bits the argmax would.
#pragma once
#include "mvp_common.h"

namespace {

__device__ __forceinline__ bool better(float v, int i, float bv, int bi) {
    // np.argmax: first occurrence of the max; NaN counts as the max (first NaN wins)
    const bool vn = isnan(v), bn = isnan(bv);
    if (bn) return vn && i < bi;
    if (vn) return true;
    return v > bv || (v == bv && i < bi);
}

// Cell bi (flat index y*W + x) with value bv of an H x W map -> image pixels: val <= 0 -> -1,
// the +-0.25 sign refinement inside 1 < px < W-1, 1 < py < H-1, * scale_factor
// (input_size / heatmap_size, f32), then the restore keypoints / input_size * input_scale +
// input_center - 0.5 * input_scale in f64, stored f32.  at(y, x) reads the map; cs: the crop's
// center x, y, scale w, h.
template <class At>
__device__ __forceinline__ void decode_cell(int bi, float bv, int H, int W, double in_w, double in_h,
                                            const float* __restrict__ cs, At at, float& ox, float& oy) {
    const int py = bi / W, px = bi - (bi / W) * W;
    float kx = (float)px, ky = (float)py;
    if (!(bv > 0.f)) {  // locs[vals <= 0.] = -1 (NaN > 0 is false but NaN <= 0 is false too)
        if (!isnan(bv)) {
            kx = -1.f;
            ky = -1.f;
        }
    }
    const int ipx = (int)kx, ipy = (int)ky;
    if (1 < ipx && ipx < W - 1 && 1 < ipy && ipy < H - 1) {
        const float dx = __fsub_rn(at(ipy, ipx + 1), at(ipy, ipx - 1));
        const float dy = __fsub_rn(at(ipy + 1, ipx), at(ipy - 1, ipx));
        const float sgx = dx > 0.f ? 1.f : (dx < 0.f ? -1.f : (isnan(dx) ? dx : 0.f));
        const float sgy = dy > 0.f ? 1.f : (dy < 0.f ? -1.f : (isnan(dy) ? dy : 0.f));
        kx = __fadd_rn(kx, __fmul_rn(sgx, 0.25f));
        ky = __fadd_rn(ky, __fmul_rn(sgy, 0.25f));
    }
    // * scale_factor (input_size / heatmap_size, f32)
    kx = __fmul_rn(kx, (float)(in_w / W));
    ky = __fmul_rn(ky, (float)(in_h / H));
    // keypoints / input_size * input_scale + input_center - 0.5 * input_scale (f64, stored f32)
    ox = (float)((double)kx / in_w * (double)cs[2] + (double)cs[0] - 0.5 * (double)cs[2]);
    oy = (float)((double)ky / in_h * (double)cs[3] + (double)cs[1] - 0.5 * (double)cs[3]);
}

}  // namespace
