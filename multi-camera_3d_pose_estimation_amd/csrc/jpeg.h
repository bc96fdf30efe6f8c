// Baseline JPEG split decode: the host entropy-decodes a frame into one offset per 8x8 block
// plus a list of its non-zero quantised coefficients (jpeg.cpp); the device dequantises and
// reconstructs the pixels — libjpeg's "islow" IDCT, "fancy" chroma upsampling and fixed-point
// YCbCr -> RGB — bit-identical to libjpeg-turbo's decode (jpeg_recon.hip).  Layouts shared by
// both sides and documented in include/mvpose.h.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define JPEG_HD __host__ __device__
#else
#define JPEG_HD
#endif

namespace jpeg {

// Component planes are MCU-padded: with luma sampling hs x vs and mcu_w x mcu_h MCUs, luma is
// 8 hs mcu_w x 8 vs mcu_h samples and each chroma plane 8 mcu_w x 8 mcu_h.  Blocks are numbered
// in scan order: MCU by MCU in raster order; inside an MCU the hs x vs luma blocks in raster
// order, then Cb, then Cr.
struct Geometry {
    int ncomp, hs, vs;
    int mcu_w, mcu_h;
    int per_mcu;           // blocks of one MCU: hs * vs + (ncomp - 1)
    int blocks;            // per_mcu * mcu_w * mcu_h
    int pw[3], ph[3];      // padded plane size of each component, samples
    int rw[3], rh[3];      // real size of each component: ceil(width h / hmax) x ceil(height v / vmax)
    int64_t plane[4];      // byte offset of each component's plane (the chroma ones as if present)
    int64_t bytes;         // all planes of the frame's ncomp components
};

JPEG_HD inline Geometry geometry(int width, int height, int ncomp, int hs, int vs) {
    Geometry g{};
    g.ncomp = ncomp;
    g.hs = hs;
    g.vs = vs;
    g.mcu_w = (width + 8 * hs - 1) / (8 * hs);
    g.mcu_h = (height + 8 * vs - 1) / (8 * vs);
    g.per_mcu = hs * vs + (ncomp - 1);
    g.blocks = g.per_mcu * g.mcu_w * g.mcu_h;
    // written out per component (no loop, no runtime index) so the struct stays in registers
    const int cw = 8 * g.mcu_w, ch = 8 * g.mcu_h;
    g.pw[0] = cw * hs;
    g.ph[0] = ch * vs;
    g.pw[1] = g.pw[2] = cw;
    g.ph[1] = g.ph[2] = ch;
    g.rw[0] = width;
    g.rh[0] = height;
    g.rw[1] = g.rw[2] = (width + hs - 1) / hs;
    g.rh[1] = g.rh[2] = (height + vs - 1) / vs;
    g.plane[0] = 0;
    g.plane[1] = (int64_t)g.pw[0] * g.ph[0];
    g.plane[2] = g.plane[1] + (int64_t)cw * ch;
    g.plane[3] = g.plane[2] + (int64_t)cw * ch;
    g.bytes = ncomp == 1 ? g.plane[1] : g.plane[3];
    return g;
}

// Blocks and plane bytes of the sampling with the most of them among the supported ones
// (what a launch over frames of mixed sampling must provide for).
JPEG_HD inline void worst_case(int width, int height, int* blocks, int64_t* plane_bytes) {
    int b = 0;
    int64_t p = 0;
    for (int m = 0; m < 3; m++) {
        const Geometry g = geometry(width, height, 3, m ? 2 : 1, m == 2 ? 2 : 1);
        if (g.blocks > b) b = g.blocks;
        if (g.bytes > p) p = g.bytes;
    }
    *blocks = b;
    *plane_bytes = p;
}

// coefficient entry: natural-order position (0..63) << 16 | (uint16) quantised value
inline uint32_t coef_entry(int pos, int value) { return (uint32_t)pos << 16 | (uint16_t)(int16_t)value; }

struct Job {               // 48 B: one frame
    const uint32_t* off;   // blocks + 1 offsets into coef: block b owns entries [off[b], off[b + 1])
    const uint32_t* coef;  // the frame's entries
    const uint16_t* qt;    // [3][64] quantisation tables of the components, natural order
    uint8_t* planes;       // scratch: the padded component planes, Geometry::bytes
    uint8_t* bgr;          // [height][width][3] output
    uint8_t ncomp, hs, vs, pad0;
    uint32_t pad1;
};
static_assert(sizeof(Job) == 48, "Job is 48 bytes");

}  // namespace jpeg
