// The HRNet graph's switches and the kernel each of its launches ends in.  graph.cpp reads the
// switches once per mvp_graph_create and selects every launch's kernel while it compiles the
// graph; nothing is re-decided per launch.  Host-only and free of the HIP runtime
// (tools/kernel_select_check.cpp runs it without a device).
#pragma once

namespace mvp {

// The backbone's MVPOSE_* environment switches (diagnostics, A/B runs and tests; all off by
// default).  read_switches() in graph.cpp is their only reader.
struct Switches {
    // fusion passes
    bool no_fuse = false;       // MVPOSE_NO_FUSE=1: every op launches on its own
    bool no_catfuse = false;    // MVPOSE_NO_CATFUSE=1: the Bottleneck downsample stays its own conv
    bool no_pairfuse = false;   // MVPOSE_NO_PAIRFUSE=1: no Bottleneck join (conv1x1_pair)
    bool no_bneck = false;      // MVPOSE_NO_BNECK=1: no whole-Bottleneck launch (bneck.hip)
    bool no_stemfuse = false;   // MVPOSE_NO_STEMFUSE=1: the two stem convs apart (no stem2.hip)
    bool no_transfuse = false;  // MVPOSE_NO_TRANSFUSE=1: transition1's two convs apart (no trans1.hip)
    bool no_sibfuse = false;    // MVPOSE_NO_SIBFUSE=1: one launch per 3x3/s2 sibling
    bool no_headfuse = false;   // MVPOSE_NO_HEADFUSE=1: fuse_sum, then the head
    bool no_tblock64 = false;   // MVPOSE_NO_TBLOCK64=1: a 64-ch BasicBlock runs as two convs
    // kernels
    bool no_head1x1 = false;    // MVPOSE_NO_HEAD1X1=1: the head on conv_mfma_kernel (and no head fusion)
    bool no_tconv = false;      // MVPOSE_NO_TCONV=1: no tconv.hip / tconv16.hip
    bool no_tconv16 = false;    // MVPOSE_TCONV16=0: tconv.hip's 64-cout tiles on the 128/256-ch planes
    bool no_s2conv = false;     // MVPOSE_NO_S2CONV=1: 3x3/s2 convs on conv_mfma_kernel
    bool no_tblock = false;     // MVPOSE_NO_TBLOCK=1: 32-ch BasicBlocks on basic_block_c32_kernel
    bool no_tblock32s = false;  // MVPOSE_NO_TBLOCK32S=1: ... on the tile kernel (tblock.hip) at every batch
    bool stem2_tile = false;    // MVPOSE_STEM2_TILE=1: stem2's tile kernel at every batch
    bool crop_stream = false;   // MVPOSE_CROP_STREAM=1: the crop-streaming kernels at every batch
    int s2_tile = 0;            // MVPOSE_S2_TILE=n (atoi): conv_mfma_kernel's 3x3/s2 tile shape, tuning only
};

// The numbers are mvp_graph_plan's documented route values.
enum Route {
    R_BLOCK = 1,      // fused BasicBlock (op - 1, op)
    R_TWIN = 2,       // transition1: 3x3/s1 conv + its 3x3/s2 twin
    R_SIBLINGS = 3,   // 3x3/s2 siblings on one input
    R_HEAD_FUSE = 4,  // heatmap head + the last fuse sum
    R_BNECK = 5,      // whole Bottleneck
    R_STEM2 = 6,      // stem conv + conv2
    R_STEM = 7,
    R_CONV = 8,       // one conv (possibly cat-fused)
    R_PAIR = 9,       // Bottleneck join: 1x1 conv (possibly cat-fused) + the next block's conv1
    R_FUSE_SUM = 10,
};

// The kernel family a launch runs (mvp_graph_kernels' ids); tile shapes and template arguments
// inside a family are its launcher's business.
enum Kernel {
    K_NONE = 0,  // no kernel serves the launch: mvp_graph_create fails
    // R_CONV, in order of preference
    K_HEAD1X1,
    K_CONV1X1_WIDE,
    K_CONV1X1,
    K_TCONV,
    K_TCONV16,
    K_S2CONV,
    K_CONV_MFMA,
    // R_BLOCK
    K_TBLOCK32S,
    K_TBLOCK32,
    K_BASIC_BLOCK_C32,
    K_TBLOCK64,        // contiguous crop range per workgroup
    K_TBLOCK64_TILES,  // tiles strided over the grid
    // R_STEM2
    K_STEM2,
    K_STEM2_TILE,
    // R_STEM
    K_STEM_MFMA,
    K_STEM,
    // routes with one kernel
    K_TRANS1,
    K_S2CONV_MULTI,
    K_HEAD_FUSE,
    K_BNECK,
    K_CONV1X1_PAIR,
    K_FUSE_SUM,
    K_COUNT
};

// The kernel function's base name, as a kernel trace shows it.
inline const char* kernel_name(int k) {
    static const char* const names[K_COUNT] = {
        "",
        "head1x1_kernel", "conv1x1_pair_kernel", "conv1x1_kernel", "tconv_kernel", "tconv16_kernel", "s2conv_kernel",
        "conv_mfma_kernel",
        "tblock32s_kernel", "tblock32_kernel", "basic_block_c32_kernel", "tblock64_kernel", "tblock64_kernel",
        "stem2_kernel", "stem2_tile_kernel",
        "stem_mfma_kernel", "stem_kernel",
        "trans1_kernel", "s2conv_kernel", "head_fuse_kernel", "bneck_kernel", "conv1x1_pair_kernel", "fuse_sum_n_kernel"};
    return k > 0 && k < K_COUNT ? names[k] : "";
}

// What a launch's kernel depends on.  R_CONV: the conv (cin counts a cat-fused source's channels
// too, h x w is the input plane, cat the first input's channels when cat-fused, else 0).
// R_BLOCK: cin and the plane.  R_STEM: the input plane.  Other routes: nothing.
struct LaunchShape {
    int cin = 0, cout = 0, h = 0, w = 0, ks = 0, stride = 0, relu = 0, res = 0, f32_out = 0, cat = 0;
};

// A launch's kernel below one crop per CU (tiles spread over every CU) and from there on (the
// crop-streaming kernels: a contiguous crop range per workgroup; measured in
// profiles/r04_crop_ranges_ab.txt).  Most launches have one kernel for both.
struct KernelChoice {
    Kernel small = K_NONE, stream = K_NONE;
};

inline bool crop_ranges_balanced(int n, int cus, const Switches& sw) { return sw.crop_stream || n >= cus; }

inline Kernel pick_kernel(const KernelChoice& c, int n, int cus, const Switches& sw) {
    return crop_ranges_balanced(n, cus, sw) ? c.stream : c.small;
}

// Conv weight padding rule shared with the host packer: Cout rounded up to the tile.
inline int conv_cout_pad(int cout) { return cout <= 32 ? 32 : (cout + 63) / 64 * 64; }

// s2conv.hip's planes whose weights are streamed from the 128-cout weight image.
inline bool s2conv_streams_image(const LaunchShape& c) {
    return (c.h == 32 && c.w == 24 && c.cout == 128 && c.cin == 64) ||
           (c.h == 16 && c.w == 12 && c.cout % 128 == 0 && (c.cin == 32 || c.cin == 64 || c.cin == 128));
}

inline Kernel select_conv(const LaunchShape& c, const Switches& sw, bool has_image) {
    const bool plane = c.ks == 3 && !c.f32_out && !c.cat;
    if (c.ks == 1 && c.stride == 1 && c.f32_out && !c.cat)
        return c.cin == 32 && c.cout == 17 && !c.res && !c.relu && !sw.no_head1x1 ? K_HEAD1X1 : K_CONV_MFMA;
    if (c.ks == 1 && c.stride == 1 && !c.f32_out) {
        // one wave owns all 256 couts: 64 -> 256 + residual, or the cat-fused 64 + 64 -> 256
        if (c.cout == 256 && c.relu && ((c.cin == 64 && c.res) || (c.cin == 128 && c.cat == 64))) return K_CONV1X1_WIDE;
        const int cp = conv_cout_pad(c.cout), kch = c.cin / 32;
        const int bm = cp % 128 == 0 && c.cin <= 64 ? 128 : cp % 64 == 0 ? 64 : 32;
        if (c.cout % (bm / 4) == 0 && (kch == 1 || kch == 2 || kch == 4 || kch == 8)) return K_CONV1X1;
        return c.cat ? K_NONE : K_CONV_MFMA;  // only the 1x1 kernels read two inputs
    }
    if (c.cat) return K_NONE;
    if (plane && c.stride == 1 && c.relu && c.cout % 32 == 0 && !sw.no_tconv) {
        if (c.cin == 256 && c.cout == 32 && c.h == 64 && c.w == 48) return K_TCONV;  // transition1.0
        if (c.cout % 64 == 0) {
            if (c.cin == 64 && c.cout == 64 && ((c.h == 32 && c.w == 24) || (c.h == 64 && c.w == 48))) return K_TCONV;
            const bool p128 = c.cin == 128 && c.h == 16 && c.w == 12, p256 = c.cin == 256 && c.h == 8 && c.w == 6;
            if (has_image && !sw.no_tconv16 && ((p128 && c.cout == 128) || (p256 && c.cout % 128 == 0))) return K_TCONV16;
            if (p128 || p256) return K_TCONV;
        }
    }
    if (plane && c.stride == 2 && !c.res && !sw.no_s2conv) {
        if (c.h == 64 && c.w == 48 && c.cout == 64 && c.cin == 32) return K_S2CONV;                  // fuse 1<-0
        if (c.h == 32 && c.w == 24 && c.cout == 128 && (c.cin == 32 || c.cin == 64)) return K_S2CONV;  // transition2, fuse 2<-{0,1}
        if (s2conv_streams_image(c)) return K_S2CONV;  // -> 256 @ 8x6: transition3, fuse 3<-{0,1,2}
    }
    return K_CONV_MFMA;
}

// The kernel(s) of a launch: (op shape, route, switches, whether the caller can give the kernel
// a weight image) -> kernel, in the launchers' order of preference.
inline KernelChoice select_kernel(Route route, const LaunchShape& c, const Switches& sw, bool has_image) {
    auto one = [](Kernel k) { return KernelChoice{k, k}; };
    switch (route) {
    case R_CONV: return one(select_conv(c, sw, has_image));
    case R_BLOCK: {
        if (c.cin == 64) return {K_TBLOCK64_TILES, K_TBLOCK64};
        const Kernel tile = c.w == 48 && c.h % 16 == 0 && !sw.no_tblock ? K_TBLOCK32 : K_BASIC_BLOCK_C32;
        const bool s32 = c.h == 64 && c.w == 48 && !sw.no_tblock32s && !sw.no_tblock;
        return {tile, s32 ? K_TBLOCK32S : tile};
    }
    case R_STEM2: return {K_STEM2_TILE, sw.stem2_tile ? K_STEM2_TILE : K_STEM2};
    case R_STEM: {  // the 256x192 crop: MFMA path
        const int ho = (c.h - 1) / 2 + 1, wo = (c.w - 1) / 2 + 1;
        return one(wo == 96 && c.h % 2 == 0 && ho % 2 == 0 ? K_STEM_MFMA : K_STEM);
    }
    case R_TWIN: return one(K_TRANS1);
    case R_SIBLINGS: return one(K_S2CONV_MULTI);
    case R_HEAD_FUSE: return one(K_HEAD_FUSE);
    case R_BNECK: return one(K_BNECK);
    case R_PAIR: return one(K_CONV1X1_PAIR);
    case R_FUSE_SUM: return one(K_FUSE_SUM);
    }
    return {};
}

// Elements of the weight image (tconv16_pack_weights) the kernel reads; 0: it reads none.
inline long conv_image_elems(Kernel k, const LaunchShape& c) {
    return k == K_TCONV16 || (k == K_S2CONV && s2conv_streams_image(c)) ? (long)c.cout * 9 * c.cin : 0;
}

}  // namespace mvp
