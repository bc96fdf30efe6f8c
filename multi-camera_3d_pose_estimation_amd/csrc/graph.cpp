// Backbone graph runtime: validation, fusion passes that compile the ops into one launch
// list, each launch's kernel selected once (kernel_select.h), liveness-based arena planning
// from that list, launch.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "conv.h"
#include "mvp_common.h"

namespace mvp {
namespace {

// One kernel launch of the forward.  The fusion passes emit these and select_kernels gives each
// its kernel; arena planning, forward, mvp_graph_plan / mvp_graph_kernels and the derived-weight
// fill only read them.
struct Launch {
    Route route;                // what the launch computes (the passes) ...
    int op;                     // launching op: the launch's place in op order (plan records, lifetimes)
    std::vector<int> covers;    // every op it computes, launcher first (R_SIBLINGS: in output order)
    std::vector<int> reads;     // tensors it reads from memory ...
    std::vector<int> writes;    // ... and writes to it; LDS / register intermediates are in neither
    KernelChoice kernel;        // ... and the kernel that computes it (select_kernels)
    int64_t macs = 0;           // per crop, over covers
    // route parameters (op indices, -1: none)
    int cat_src = -1;           // R_CONV / R_PAIR / lead R_BNECK: absorbed 1x1 whose input and weights are concatenated
    int tail = -1;              // R_PAIR: the 256 -> 64 successor
    int conv1 = -1, conv2 = -1; // R_BNECK
    int perm = 0;               // R_BNECK: conv1 sums K in the Bottleneck join's order (bneck.hip)
    int lead = 0;               // R_BNECK: layer1's first block, 64-ch input, conv3 cat-fused with the downsample
    int stem = -1;              // R_STEM2
    int twin = -1;              // R_TWIN
    int fuse = -1;              // R_HEAD_FUSE
    int planar = 0;             // R_BNECK output / R_TWIN input in chunk-planar layout
    // derived weights (owned; alloc_weights / fill_weights / free_weights)
    uint16_t* w = nullptr;      // cat_src: [cout_pad][cin + cin_src]; R_SIBLINGS: [128][3][3][cin]
    float* b = nullptr;         // cat_src: summed biases [cout_pad]; R_SIBLINGS: [128]
    uint16_t* w_img = nullptr;  // R_CONV: the image its kernel reads (conv_image_elems); R_TWIN: trans1 image
};

struct Segment {
    int first_op = 0, last_op = -1;  // inclusive op range
    int first_launch = 0, end_launch = 0;
    int micro_batch = 0;             // 0 = whole batch
};

struct Graph {
    std::vector<mvp_tensor_desc> tensors;
    std::vector<mvp_op_desc> ops;
    std::vector<Segment> segs;
    std::vector<int> local_seg;  // segment a tensor is local to (micro-batch sized), -1 = full batch
    int input = -1, output = -1;
    const uint16_t* wb = nullptr;
    const float* fb = nullptr;
    int max_batch = 0;
    Switches sw;                   // the environment's, as mvp_graph_create found it
    int cus = 0;                   // cu_count(): crop-streaming kernels from one crop per CU
    std::vector<Launch> launches;  // in op order once finish_launches has run
    std::vector<int> owner;        // per op: index of the launch that covers it, -1 = none yet
    std::vector<int64_t> offset;   // per-crop-batch arena offsets (bytes), -1 = external
    int64_t arena_bytes = 0;
    char* arena = nullptr;
};

int64_t elem_size(int dtype) { return dtype == MVP_DT_F32_NCHW ? 4 : 2; }

int64_t tensor_bytes(const mvp_tensor_desc& t, int batch) {
    return (int64_t)batch * t.h * t.w * t.c * elem_size(t.dtype);
}

// The only reader of the backbone's switches: once per mvp_graph_create.
Switches read_switches() {
    auto first_is = [](const char* name, char c) {
        const char* e = getenv(name);
        return e && e[0] == c;
    };
    Switches sw;
    sw.no_fuse = first_is("MVPOSE_NO_FUSE", '1');
    sw.no_catfuse = first_is("MVPOSE_NO_CATFUSE", '1');
    sw.no_pairfuse = first_is("MVPOSE_NO_PAIRFUSE", '1');
    sw.no_bneck = first_is("MVPOSE_NO_BNECK", '1');
    sw.no_stemfuse = first_is("MVPOSE_NO_STEMFUSE", '1');
    sw.no_transfuse = first_is("MVPOSE_NO_TRANSFUSE", '1');
    sw.no_sibfuse = first_is("MVPOSE_NO_SIBFUSE", '1');
    sw.no_headfuse = first_is("MVPOSE_NO_HEADFUSE", '1');
    sw.no_tblock64 = first_is("MVPOSE_NO_TBLOCK64", '1');
    sw.no_head1x1 = first_is("MVPOSE_NO_HEAD1X1", '1');
    sw.no_tconv = first_is("MVPOSE_NO_TCONV", '1');
    sw.no_tconv16 = first_is("MVPOSE_TCONV16", '0');
    sw.no_s2conv = first_is("MVPOSE_NO_S2CONV", '1');
    sw.no_tblock = first_is("MVPOSE_NO_TBLOCK", '1');
    sw.no_tblock32s = first_is("MVPOSE_NO_TBLOCK32S", '1');
    sw.stem2_tile = first_is("MVPOSE_STEM2_TILE", '1');
    sw.crop_stream = first_is("MVPOSE_CROP_STREAM", '1');
    const char* e = getenv("MVPOSE_S2_TILE");
    sw.s2_tile = e ? atoi(e) : 0;
    return sw;
}

void validate(Graph& g, int64_t w_elems, int64_t f_elems) {
    const int nt = (int)g.tensors.size();
    auto T = [&](int id) -> const mvp_tensor_desc& {
        MVP_REQUIRE(id >= 0 && id < nt, "graph: tensor id %d out of range", id);
        return g.tensors[id];
    };
    std::vector<int> defined(nt, 0);
    defined[g.input] = 1;
    for (size_t k = 0; k < g.ops.size(); k++) {
        const mvp_op_desc& op = g.ops[k];
        const mvp_tensor_desc& o = T(op.out);
        MVP_REQUIRE(op.n_in >= 1 && op.n_in <= 4, "graph op %zu: n_in=%d", k, op.n_in);
        for (int i = 0; i < op.n_in; i++) {
            if (op.kind == MVP_OP_CONV && i == 1 && op.in[1] < 0) continue;
            T(op.in[i]);
            MVP_REQUIRE(defined[op.in[i]], "graph op %zu reads tensor %d before it is produced", k, op.in[i]);
        }
        MVP_REQUIRE(!defined[op.out], "graph op %zu: tensor %d produced twice", k, op.out);
        if (op.kind == MVP_OP_STEM) {
            const mvp_tensor_desc& x = T(op.in[0]);
            MVP_REQUIRE(x.c == 4 && x.dtype == MVP_DT_BF16_NHWC, "stem: input must be bf16 NHWC with 4 channels");
            MVP_REQUIRE(o.c == 64 && o.h == (x.h - 1) / 2 + 1 && o.w == (x.w - 1) / 2 + 1, "stem: output shape");
            MVP_REQUIRE(op.w_off >= 0 && op.w_off + 64 * 36 <= f_elems && op.b_off >= 0 && op.b_off + 64 <= f_elems,
                        "stem: weights out of the f32 blob");
        } else if (op.kind == MVP_OP_CONV) {
            const mvp_tensor_desc& x = T(op.in[0]);
            const int pad = op.ks / 2;
            MVP_REQUIRE(op.ks == 1 || op.ks == 3, "conv op %zu: ks", k);
            MVP_REQUIRE(op.stride == 1 || (op.stride == 2 && op.ks == 3), "conv op %zu: stride", k);
            MVP_REQUIRE(x.c == op.cin && x.dtype == MVP_DT_BF16_NHWC && op.cin % 32 == 0,
                        "conv op %zu: input channels %d vs cin %d", k, x.c, op.cin);
            MVP_REQUIRE(o.c == op.cout && o.h == (x.h + 2 * pad - op.ks) / op.stride + 1 &&
                            o.w == (x.w + 2 * pad - op.ks) / op.stride + 1,
                        "conv op %zu: output shape", k);
            MVP_REQUIRE(o.dtype == MVP_DT_F32_NCHW || op.cout % 4 == 0, "conv op %zu: cout %% 4", k);
            if (op.n_in > 1 && op.in[1] >= 0) {
                const mvp_tensor_desc& r = T(op.in[1]);
                MVP_REQUIRE(r.h == o.h && r.w == o.w && r.c == o.c && r.dtype == MVP_DT_BF16_NHWC &&
                                o.dtype == MVP_DT_BF16_NHWC,
                            "conv op %zu: residual shape", k);
            }
            const int64_t cp = conv_cout_pad(op.cout);
            MVP_REQUIRE(op.w_off >= 0 && op.w_off % 8 == 0 && op.w_off + cp * op.ks * op.ks * op.cin <= w_elems,
                        "conv op %zu: weights out of the bf16 blob", k);
            MVP_REQUIRE(op.b_off >= 0 && op.b_off % 4 == 0 && op.b_off + cp <= f_elems,
                        "conv op %zu: bias out of the f32 blob", k);
        } else if (op.kind == MVP_OP_FUSE) {
            MVP_REQUIRE(o.dtype == MVP_DT_BF16_NHWC && o.c % 8 == 0, "fuse op %zu: output", k);
            for (int i = 0; i < op.n_in; i++) {
                const mvp_tensor_desc& x = T(op.in[i]);
                const int u = op.up[i];
                MVP_REQUIRE(u >= 1 && x.c == o.c && x.h * u == o.h && x.w * u == o.w, "fuse op %zu: input %d shape",
                            k, i);
            }
        } else {
            fail(MVP_ERR_ARG, "graph op %zu: unknown kind %d", k, op.kind);
        }
        defined[op.out] = 1;
    }
    MVP_REQUIRE(defined[g.output], "graph: output tensor never produced");
    // segments: contiguous op ranges in increasing order
    const int ns = (int)g.segs.size();
    int prev = -1;
    for (int k = 0; k < (int)g.ops.size(); k++) {
        const int sg = g.ops[k].segment;
        MVP_REQUIRE(sg >= 0 && sg < ns, "graph op %d: segment %d out of range", k, sg);
        MVP_REQUIRE(sg >= prev, "graph op %d: segments must be contiguous and ordered", k);
        if (sg != prev) g.segs[sg].first_op = k;
        g.segs[sg].last_op = k;
        prev = sg;
    }
}

// ---- what the fusion passes share ----------------------------------------------------------

bool is_free(const Graph& g, int k) { return k >= 0 && g.owner[k] < 0; }

// The launch op k launches itself (nullptr: k is free, or absorbed into another op's launch).
Launch* launch_of(Graph& g, int k) {
    if (k < 0 || g.owner[k] < 0) return nullptr;
    Launch& L = g.launches[g.owner[k]];
    return L.op == k ? &L : nullptr;
}

void cover(Graph& g, Launch& L, int k) {
    L.covers.push_back(k);
    g.owner[k] = (int)(&L - g.launches.data());
}

Launch& emit(Graph& g, Route route, int op, std::vector<int> reads, std::vector<int> writes) {
    g.launches.push_back(Launch{route, op, {}, std::move(reads), std::move(writes)});
    cover(g, g.launches.back(), op);
    return g.launches.back();
}

bool has_res(const mvp_op_desc& op) { return op.n_in > 1 && op.in[1] >= 0; }

// A conv of this kernel size, stride and activation (relu < 0: either) with a bf16 NHWC output ...
bool is_conv(const Graph& g, int k, int ks, int stride, int relu) {
    if (k < 0) return false;
    const mvp_op_desc& op = g.ops[k];
    return op.kind == MVP_OP_CONV && op.ks == ks && op.stride == stride && (relu < 0 || !op.relu == !relu) &&
           g.tensors[op.out].dtype == MVP_DT_BF16_NHWC;
}
// ... and no residual.
bool plain_conv(const Graph& g, int k, int ks, int stride, int relu) {
    return is_conv(g, k, ks, stride, relu) && !has_res(g.ops[k]);
}

// The launch of a conv on its own: reads its input and residual, writes its output.
Launch& emit_conv(Graph& g, int k) {
    const mvp_op_desc& op = g.ops[k];
    std::vector<int> reads{op.in[0]};
    if (has_res(op)) reads.push_back(op.in[1]);
    return emit(g, R_CONV, k, reads, {op.out});
}

// Readers per tensor and producing op per tensor.  skip_block_mid: a fused BasicBlock's
// intermediate (its head's in[0]) is not counted as read.
struct UseDef {
    std::vector<int> uses, producer;
};
UseDef use_def(Graph& g, bool skip_block_mid) {
    const int nt = (int)g.tensors.size();
    UseDef ud{std::vector<int>(nt, 0), std::vector<int>(nt, -1)};
    for (int k = 0; k < (int)g.ops.size(); k++) {
        const mvp_op_desc& op = g.ops[k];
        ud.producer[op.out] = k;
        const Launch* L = skip_block_mid ? launch_of(g, k) : nullptr;
        for (int i = 0; i < op.n_in; i++)
            if (op.in[i] >= 0 && !(i == 0 && L && L->route == R_BLOCK)) ud.uses[op.in[i]]++;
    }
    return ud;
}

// Input channels of a 1x1 launch: its op's, plus the cat-fused source's.
int cat_cin(Graph& g, int k) {
    const Launch* L = launch_of(g, k);
    return g.ops[k].cin + (L && L->cat_src >= 0 ? g.ops[L->cat_src].cin : 0);
}

// ---- fusion passes, in the order mvp_graph_create runs them ---------------------------------

// A 3x3 conv pair conv1 (relu) -> conv2 (+ conv1's input as residual, relu) on 32 channels
// (64x48 plane) or 64 channels (32x24 plane, tblock64.hip) whose intermediate feeds nothing
// else becomes one fused BasicBlock launch; the intermediate tensor is then never allocated.
void fuse(Graph& g) {
    const int no = (int)g.ops.size();
    const UseDef ud = use_def(g, false);
    auto is_block_conv3 = [&](int k) {
        const mvp_op_desc& op = g.ops[k];
        return is_conv(g, k, 3, 1, 1) && (op.cin == 32 || op.cin == 64) && op.cout == op.cin;
    };
    for (int k = 0; k + 1 < no; k++) {
        const mvp_op_desc& a = g.ops[k];
        const mvp_op_desc& b = g.ops[k + 1];
        if (!is_free(g, k) || !is_block_conv3(k) || !is_block_conv3(k + 1) || a.cin != b.cin) continue;
        const bool b_res = b.n_in > 1 && b.in[1] == a.in[0];
        const mvp_tensor_desc& t = g.tensors[a.out];
        if (has_res(a) || !b_res || b.in[0] != a.out || ud.uses[a.out] != 1 || a.out == g.output) continue;
        const bool ok =
            a.cin == 32 ? basic_block_c32_supported(t.h, t.w) : !g.sw.no_tblock64 && tblock64_supported(t.h, t.w);
        if (a.segment != b.segment || !ok) continue;
        cover(g, emit(g, R_BLOCK, k + 1, {a.in[0]}, {b.out}), k);
        k++;
    }
}

// Cat-fusion: y = act(conv1x1_B(h) + bias_B + t) whose residual t = conv1x1_A(x) + bias_A
// (no activation, consumed only here: the Bottleneck downsample) becomes ONE 1x1 conv over
// the channel concatenation [h, x] with weights [W_B | W_A] and bias bias_B + bias_A.  The
// t tensor (256 channels at 64x48 in HRNet-W32: 1.6 GB per 1024 crops, written then read
// back as the residual) disappears, and t is no longer rounded to bf16 before the add.
void cat_fuse(Graph& g) {
    if (g.sw.no_catfuse) return;
    const UseDef ud = use_def(g, true);
    for (int b = 0; b < (int)g.ops.size(); b++) {
        const mvp_op_desc& B = g.ops[b];
        if (!is_free(g, b) || !is_conv(g, b, 1, 1, -1) || !has_res(B)) continue;
        const int t = B.in[1], a = ud.producer[t];
        if (a >= b || !is_free(g, a) || !plain_conv(g, a, 1, 1, 0)) continue;
        const mvp_op_desc& A = g.ops[a];
        if (A.cout != B.cout || ud.uses[t] != 1 || t == g.output || A.segment != B.segment) continue;
        const int kch = (A.cin + B.cin) / 32;  // conv1x1_kernel instantiations: K = 32, 64, 128, 256
        if (kch != 2 && kch != 4 && kch != 8) continue;
        Launch& L = emit(g, R_CONV, b, {B.in[0], A.in[0]}, {B.out});
        L.cat_src = a;
        cover(g, L, a);
    }
}

// The Bottleneck chain ending in conv3 c (1x1 64 -> 256): conv1 a (1x1 cin1 -> 64) -> conv2 b
// (3x3 64 -> 64) -> c, all ReLU, a and b free with no residual and outputs nothing else reads,
// one segment, on the plane bneck.hip serves.
bool bneck_chain(Graph& g, const UseDef& ud, int c, int cin1, int& a, int& b) {
    auto mid = [&](int k, int ks, int cin) {
        return is_free(g, k) && plain_conv(g, k, ks, 1, 1) && g.ops[k].cin == cin && g.ops[k].cout == 64 &&
               ud.uses[g.ops[k].out] == 1 && g.ops[k].out != g.output && g.ops[k].segment == g.ops[c].segment;
    };
    if (!is_conv(g, c, 1, 1, 1) || g.ops[c].cin != 64 || g.ops[c].cout != 256) return false;
    b = ud.producer[g.ops[c].in[0]];
    if (!mid(b, 3, 64)) return false;
    a = ud.producer[g.ops[b].in[0]];
    if (!mid(a, 1, cin1)) return false;
    const mvp_tensor_desc& x = g.tensors[g.ops[a].in[0]];
    return !g.sw.no_bneck && bneck_supported(x.h, x.w, x.c, g.ops[a].cout);
}

// Bottleneck fusion (bneck.hip): layer1's Bottleneck on the 256-ch 64x48 plane — conv1 (1x1
// 256 -> 64, ReLU), conv2 (3x3 64 -> 64, ReLU), conv3 (1x1 64 -> 256, + the block's input,
// ReLU), intermediates read by nothing else — runs as one streaming launch; the two 64-ch
// intermediates are never allocated.  Runs before pair_fuse (which would otherwise join conv1
// to the previous block's conv3); conv1 keeps the K order the join would have given it (perm)
// so the result stays bit-identical to the unfused graph.
void bneck_fuse(Graph& g) {
    const bool pair_enabled = !g.sw.no_pairfuse;
    const int no = (int)g.ops.size();
    const UseDef ud = use_def(g, true);
    int a = -1, b = -1;
    for (int c = 0; c < no; c++) {
        const mvp_op_desc& C = g.ops[c];
        if (!is_free(g, c) || !has_res(C) || !bneck_chain(g, ud, c, 256, a, b) || g.ops[a].in[0] != C.in[1]) continue;
        // would pair_fuse have joined conv1 to its producer (a 1x1 256-cout ReLU conv)?
        const int f = ud.producer[C.in[1]];
        const bool perm = pair_enabled && f >= 0 && (is_free(g, f) || launch_of(g, f)) && is_conv(g, f, 1, 1, 1) &&
                          g.ops[f].cout == 256 && g.ops[f].segment == C.segment &&
                          conv1x1_pair_supported(cat_cin(g, f), 256, 64);
        Launch& L = emit(g, R_BNECK, c, {C.in[1]}, {C.out});
        L.conv1 = a, L.conv2 = b, L.perm = perm;
        cover(g, L, a);
        cover(g, L, b);
    }
    // layer1's first block: conv1 (1x1 64 -> 64) and the downsample (1x1 64 -> 256, cat-fused
    // into conv3) read the same 64-ch tensor; conv3's K is [conv2's output | that tensor]
    for (int c = 0; c < no; c++) {
        Launch* L = launch_of(g, c);
        if (!L || L->route != R_CONV || L->cat_src < 0) continue;
        const mvp_op_desc& D = g.ops[L->cat_src];
        if (D.cin != 64 || !bneck_chain(g, ud, c, 64, a, b) || g.ops[a].in[0] != D.in[0]) continue;
        L->route = R_BNECK;
        L->reads = {D.in[0]};
        L->conv1 = a, L->conv2 = b, L->lead = 1;
        cover(g, *L, a);
        cover(g, *L, b);
    }
}

// Pair fusion (Bottleneck join): a 1x1 conv A producing 256 channels with ReLU (the
// Bottleneck's conv3, single input + residual or cat-fused with the downsample) whose
// output T is read by a 1x1 conv B (256 -> 64, ReLU, no residual: the next Bottleneck's
// conv1) runs as one conv1x1_pair launch that writes T (still needed as the next
// residual) and B's output; T is no longer re-read for B.
void pair_fuse(Graph& g) {
    if (g.sw.no_pairfuse) return;
    const UseDef ud = use_def(g, false);
    for (int b = 0; b < (int)g.ops.size(); b++) {
        const mvp_op_desc& B = g.ops[b];
        if (!is_free(g, b) || !plain_conv(g, b, 1, 1, 1) || B.cin != 256 || B.cout != 64) continue;
        const int a = ud.producer[B.in[0]];
        Launch* L = launch_of(g, a);
        if (a < 0 || a >= b || !(is_free(g, a) || (L && L->route == R_CONV)) || !is_conv(g, a, 1, 1, 1)) continue;
        const mvp_op_desc& A = g.ops[a];
        if (A.cout != 256 || A.segment != B.segment) continue;
        if (!conv1x1_pair_supported(cat_cin(g, a), A.cout, B.cout)) continue;
        if (!L) L = &emit_conv(g, a);
        L->route = R_PAIR;
        L->tail = b;
        L->writes.push_back(B.out);
        cover(g, *L, b);
    }
}

// Stem fusion: the stem conv (OP_STEM, 4 -> 64, s2) whose output feeds only a 3x3/s2 64 -> 64
// conv (HRNet's conv2) runs inside that conv's launch (stem2.hip); the 128x96x64 intermediate
// (1.6 GB per 1024 crops) is never allocated.
void stem_fuse(Graph& g) {
    if (g.sw.no_stemfuse) return;
    const int no = (int)g.ops.size();
    const UseDef ud = use_def(g, false);
    for (int a = 0; a < no; a++) {
        const mvp_op_desc& A = g.ops[a];
        if (A.kind != MVP_OP_STEM || !is_free(g, a) || ud.uses[A.out] != 1 || A.out == g.output) continue;
        for (int b = a + 1; b < no; b++) {
            const mvp_op_desc& B = g.ops[b];
            if (B.in[0] != A.out) continue;
            const mvp_tensor_desc& x = g.tensors[A.in[0]];
            if (is_free(g, b) && plain_conv(g, b, 3, 2, 1) && B.segment == A.segment &&
                stem2_supported(x.h, x.w, B.cin, B.cout)) {
                Launch& L = emit(g, R_STEM2, b, {A.in[0]}, {B.out});
                L.stem = a;
                cover(g, L, a);
            }
            break;
        }
    }
}

// Transition fusion: HRNet's transition1 reads the layer1 output (256 ch @ 64x48) with two
// 3x3 convs (s1 -> 32 ch, s2 -> 64 ch); trans1.hip runs both from one pass over it.
void twin_fuse(Graph& g) {
    if (g.sw.no_transfuse) return;
    const int no = (int)g.ops.size();
    for (int a = 0; a < no; a++) {
        if (!is_free(g, a) || !plain_conv(g, a, 3, 1, 1)) continue;
        const mvp_op_desc& A = g.ops[a];
        const mvp_tensor_desc& x = g.tensors[A.in[0]];
        for (int b = a + 1; b < no; b++) {
            const mvp_op_desc& B = g.ops[b];
            if (B.in[0] != A.in[0] || !is_free(g, b) || !plain_conv(g, b, 3, 2, 1) || B.segment != A.segment) continue;
            if (!trans1_supported(x.h, x.w, x.c, A.cout, B.cout)) continue;
            Launch& L = emit(g, R_TWIN, a, {A.in[0]}, {A.out, B.out});
            L.twin = b;
            cover(g, L, b);
            break;
        }
    }
}

// Planar layout: a fused Bottleneck whose output feeds only a fused transition1 (its two convs
// and nothing else) writes it chunk-planar ([N][16][H][W][16]) and trans1 reads it so: each
// 16-channel item of trans1 is then contiguous in HBM instead of a quarter of every 128-B line
// (PMC: trans1 read its 1.6 GB input 1.67 times).  Numerically a no-op.
void planar_fuse(Graph& g) {
    const UseDef ud = use_def(g, false);
    for (Launch& T : g.launches) {
        if (T.route != R_TWIN) continue;
        const int t = T.reads[0];
        Launch* B = launch_of(g, ud.producer[t]);
        if (B && B->route == R_BNECK && !B->lead && ud.uses[t] == 2 && t != g.output) B->planar = T.planar = 1;
    }
}

// Sibling fusion: in an HRModule fuse layer the branch-0 tensor (32 ch @ 64x48) is the input
// of up to three 3x3/s2 convs (-> 64 ch for branch 1; -> 32 ch + ReLU starting the chains to
// branches 2 and 3).  They run as ONE launch over cout-concatenated weights (s2conv_multi):
// the 201 MB input is read once instead of once per conv.
void sib_fuse(Graph& g) {
    if (g.sw.no_sibfuse) return;
    const int no = (int)g.ops.size();
    auto plain_s2 = [&](int k) { return is_free(g, k) && plain_conv(g, k, 3, 2, -1) && g.ops[k].cout % 32 == 0; };
    for (int a = 0; a < no; a++) {
        if (!plain_s2(a)) continue;
        const mvp_op_desc& A = g.ops[a];
        const mvp_tensor_desc& x = g.tensors[A.in[0]];
        int tot = A.cout;
        std::vector<int> list;
        for (int b = a + 1; b < no && list.size() < 2; b++) {
            const mvp_op_desc& B = g.ops[b];
            if (B.in[0] != A.in[0] || !plain_s2(b) || B.segment != A.segment) continue;
            if (!s2conv_multi_supported(x.h, x.w, x.c, tot + B.cout)) continue;
            list.push_back(b);
            tot += B.cout;
        }
        if (list.empty()) continue;
        Launch& L = emit(g, R_SIBLINGS, a, {A.in[0]}, {A.out});
        for (int b : list) {
            L.writes.push_back(g.ops[b].out);
            cover(g, L, b);
        }
    }
}

// Head fusion: the last fuse layer's out0 (32 ch @ 64x48) feeds only the heatmap head (1x1
// 32 -> 17, f32 NCHW); the head kernel forms out0 per pixel itself, so the 201 MB tensor is
// never written or re-read (bit-identical: same sums, same bf16 rounding).
void head_fuse(Graph& g) {
    if (g.sw.no_headfuse || g.sw.no_head1x1) return;
    const UseDef ud = use_def(g, false);
    for (int k = 0; k < (int)g.ops.size(); k++) {
        const mvp_op_desc& H = g.ops[k];
        if (H.kind != MVP_OP_CONV || !is_free(g, k) || g.tensors[H.out].dtype != MVP_DT_F32_NCHW || H.ks != 1 ||
            H.relu || has_res(H))
            continue;
        const int f = ud.producer[H.in[0]];
        if (!is_free(g, f) || g.ops[f].kind != MVP_OP_FUSE || ud.uses[H.in[0]] != 1 || H.in[0] == g.output ||
            g.ops[f].segment != H.segment)
            continue;
        const mvp_op_desc& F = g.ops[f];
        if (!head_fuse_supported(H.cin, H.cout, F.n_in)) continue;
        Launch& L = emit(g, R_HEAD_FUSE, k, std::vector<int>(F.in, F.in + F.n_in), {H.out});
        L.fuse = f;
        cover(g, L, f);
    }
}

int64_t op_macs(const Graph& g, int k) {
    const mvp_op_desc& op = g.ops[k];
    if (op.kind != MVP_OP_CONV && op.kind != MVP_OP_STEM) return 0;
    const mvp_tensor_desc& o = g.tensors[op.out];
    const int cin = op.kind == MVP_OP_STEM ? 3 : op.cin;
    return (int64_t)o.h * o.w * op.cout * cin * op.ks * op.ks;
}

// Every op no pass claimed launches on its own; then the list goes into op order (= launch
// order) and each segment gets its range of it.
void finish_launches(Graph& g) {
    const int no = (int)g.ops.size();
    for (int k = 0; k < no; k++) {
        const mvp_op_desc& op = g.ops[k];
        if (!is_free(g, k)) continue;
        if (op.kind == MVP_OP_CONV) emit_conv(g, k);
        else if (op.kind == MVP_OP_STEM) emit(g, R_STEM, k, {op.in[0]}, {op.out});
        else emit(g, R_FUSE_SUM, k, std::vector<int>(op.in, op.in + op.n_in), {op.out});
    }
    std::sort(g.launches.begin(), g.launches.end(), [](const Launch& a, const Launch& b) { return a.op < b.op; });
    std::vector<int> covered(no, 0);
    for (Segment& sg : g.segs) sg.first_launch = sg.end_launch = 0;
    for (int l = 0; l < (int)g.launches.size(); l++) {
        Launch& L = g.launches[l];
        for (int k : L.covers) {
            g.owner[k] = l;
            covered[k]++;
            L.macs += op_macs(g, k);
        }
        Segment& sg = g.segs[g.ops[L.op].segment];
        if (sg.end_launch == 0) sg.first_launch = l;
        sg.end_launch = l + 1;
    }
    for (int k = 0; k < no; k++) MVP_REQUIRE(covered[k] == 1, "graph: op %d covered by %d launches", k, covered[k]);
}

// ---- kernel selection -------------------------------------------------------------------------

// What select_kernel looks at (kernel_select.h LaunchShape).
LaunchShape launch_shape(const Graph& g, const Launch& L) {
    const mvp_op_desc& op = g.ops[L.op];
    const mvp_tensor_desc& x = g.tensors[op.in[0]];
    const bool cat = L.cat_src >= 0;
    LaunchShape c;
    c.cin = op.cin + (cat ? g.ops[L.cat_src].cin : 0), c.cout = op.cout, c.h = x.h, c.w = x.w;
    c.ks = op.ks, c.stride = op.stride, c.relu = op.relu;
    c.res = !cat && has_res(op);  // a cat-fused launch has its residual in the second input
    c.f32_out = g.tensors[op.out].dtype == MVP_DT_F32_NCHW;
    c.cat = cat ? op.cin : 0;
    return c;
}

// Every launch's kernel, from its route, its shape and the switches: chosen here once, so the
// weight images, mvp_graph_kernels and every forward agree on it.  The graph makes the weight
// image for whichever kernel reads one, hence has_image = true.
void select_kernels(Graph& g) {
    for (Launch& L : g.launches) {
        L.kernel = select_kernel(L.route, launch_shape(g, L), g.sw, true);
        MVP_REQUIRE(L.kernel.small != K_NONE && L.kernel.stream != K_NONE, "graph op %d: no kernel serves it", L.op);
    }
}

// ---- derived weights ---------------------------------------------------------------------
// Device-side weights a launch owns: allocated at graph create time, filled from the blobs by
// fill_weights (create and mvp_graph_refresh_weights).

void alloc_weights(Graph& g) {
    for (Launch& L : g.launches) {
        const mvp_op_desc& op = g.ops[L.op];
        if (L.cat_src >= 0) {
            const int cp = conv_cout_pad(op.cout), cin = op.cin + g.ops[L.cat_src].cin;
            MVP_HIP(hipMalloc(&L.w, (size_t)cp * cin * sizeof(uint16_t)));
            MVP_HIP(hipMalloc(&L.b, (size_t)cp * sizeof(float)));
        } else if (L.route == R_SIBLINGS) {
            MVP_HIP(hipMalloc(&L.w, (size_t)128 * 9 * op.cin * sizeof(uint16_t)));
            MVP_HIP(hipMalloc(&L.b, (size_t)128 * sizeof(float)));
        } else if (L.route == R_TWIN) {
            MVP_HIP(hipMalloc(&L.w_img, (size_t)kTrans1ImageElems * sizeof(uint16_t)));
        } else if (const long n = L.route == R_CONV ? conv_image_elems(L.kernel.small, launch_shape(g, L)) : 0) {
            MVP_HIP(hipMalloc(&L.w_img, (size_t)n * sizeof(uint16_t)));
        }
    }
}

void fill_weights(Graph& g) {
    for (Launch& L : g.launches) {
        const mvp_op_desc& op = g.ops[L.op];
        if (L.cat_src >= 0) {  // [W | W_src], bias + bias_src
            const mvp_op_desc& A = g.ops[L.cat_src];
            const int cp = conv_cout_pad(op.cout), cin = op.cin + A.cin;
            MVP_HIP(hipMemcpy2D(L.w, (size_t)cin * 2, g.wb + op.w_off, (size_t)op.cin * 2, (size_t)op.cin * 2, cp,
                                hipMemcpyDeviceToDevice));
            MVP_HIP(hipMemcpy2D(L.w + op.cin, (size_t)cin * 2, g.wb + A.w_off, (size_t)A.cin * 2, (size_t)A.cin * 2,
                                cp, hipMemcpyDeviceToDevice));
            std::vector<float> hb(cp), ha(cp);
            MVP_HIP(hipMemcpy(hb.data(), g.fb + op.b_off, cp * sizeof(float), hipMemcpyDeviceToHost));
            MVP_HIP(hipMemcpy(ha.data(), g.fb + A.b_off, cp * sizeof(float), hipMemcpyDeviceToHost));
            for (int i = 0; i < cp; i++) hb[i] += ha[i];
            MVP_HIP(hipMemcpy(L.b, hb.data(), cp * sizeof(float), hipMemcpyHostToDevice));
        } else if (L.route == R_SIBLINGS) {  // the members' rows one after another, zero rows after them
            const int kk = 9 * op.cin;
            MVP_HIP(hipMemset(L.w, 0, (size_t)128 * kk * sizeof(uint16_t)));
            MVP_HIP(hipMemset(L.b, 0, (size_t)128 * sizeof(float)));
            int row = 0;
            for (int m : L.covers) {
                const mvp_op_desc& o = g.ops[m];
                MVP_HIP(hipMemcpy(L.w + (size_t)row * kk, g.wb + o.w_off, (size_t)o.cout * kk * sizeof(uint16_t),
                                  hipMemcpyDeviceToDevice));
                MVP_HIP(hipMemcpy(L.b + row, g.fb + o.b_off, (size_t)o.cout * sizeof(float), hipMemcpyDeviceToDevice));
                row += o.cout;
            }
        } else if (L.route == R_TWIN) {
            trans1_pack_weights(g.wb, op.w_off, g.ops[L.twin].w_off, L.w_img, nullptr);
        } else if (L.w_img) {
            tconv16_pack_weights(g.wb + op.w_off, L.w_img, op.cin, op.cout, nullptr);
        }
    }
    MVP_HIP(hipDeviceSynchronize());
}

void free_weights(Graph& g) {
    for (Launch& L : g.launches) {
        if (L.w) (void)hipFree(L.w);
        if (L.b) (void)hipFree(L.b);
        if (L.w_img) (void)hipFree(L.w_img);
        L.w = L.w_img = nullptr;
        L.b = nullptr;
    }
}

// ---- arena ----------------------------------------------------------------------------------
// Greedy first-fit placement of tensors in one arena by lifetime [def, last use], both taken
// from the launches' read / write lists at their launching op's index.
// A tensor produced and consumed only inside one micro-batched segment is
// "local": it is sized for one micro-batch and re-used by every micro-batch.
// Every other tensor a micro-batched segment touches is sliced per micro-batch,
// so its lifetime is widened to the whole segment (later micro-batches replay
// the segment's ops).
void plan(Graph& g) {
    const int nt = (int)g.tensors.size();
    std::vector<int> first(nt, -1), last(nt, -1);
    std::vector<int> seg_of_def(nt, -1);
    std::vector<int> multi_seg(nt, 0);  // used by more than one segment
    std::vector<int> use_seg(nt, -1);
    for (const Launch& L : g.launches) {
        const int k = L.op, seg = g.ops[k].segment;
        auto touch = [&](int t) {
            last[t] = std::max(last[t], k);
            if (use_seg[t] < 0) use_seg[t] = seg;
            else if (use_seg[t] != seg) multi_seg[t] = 1;
        };
        for (int t : L.writes) {
            first[t] = k;
            seg_of_def[t] = seg;
            touch(t);
        }
        for (int t : L.reads) touch(t);
    }
    g.local_seg.assign(nt, -1);
    for (int t = 0; t < nt; t++) {
        if (t == g.input || t == g.output || first[t] < 0) continue;
        const int sg = seg_of_def[t];
        if (!multi_seg[t] && g.segs[sg].micro_batch > 0 && g.segs[sg].micro_batch < g.max_batch) g.local_seg[t] = sg;
    }
    for (const Launch& L : g.launches) {
        const Segment& sg = g.segs[g.ops[L.op].segment];
        if (sg.micro_batch <= 0 || sg.micro_batch >= g.max_batch) continue;
        auto widen = [&](int t) {
            if (g.local_seg[t] >= 0) return;
            first[t] = std::min(first[t] < 0 ? sg.first_op : first[t], sg.first_op);
            last[t] = std::max(last[t], sg.last_op);
        };
        for (int t : L.writes) widen(t);
        for (int t : L.reads) widen(t);
    }
    std::vector<int> order;
    for (int t = 0; t < nt; t++)
        if (t != g.input && t != g.output && first[t] >= 0) order.push_back(t);
    auto alloc_bytes = [&](int t) {
        const int b = g.local_seg[t] >= 0 ? g.segs[g.local_seg[t]].micro_batch : g.max_batch;
        return (tensor_bytes(g.tensors[t], b) + 255) / 256 * 256;
    };
    std::sort(order.begin(), order.end(), [&](int a, int b) { return alloc_bytes(a) > alloc_bytes(b); });
    g.offset.assign(nt, -1);
    struct Placed {
        int64_t off, size;
        int first, last;
    };
    std::vector<Placed> placed;
    int64_t top = 0;
    for (int t : order) {
        const int64_t size = alloc_bytes(t);
        std::vector<Placed> live;
        for (const Placed& p : placed)
            if (!(p.last < first[t] || last[t] < p.first)) live.push_back(p);
        std::sort(live.begin(), live.end(), [](const Placed& a, const Placed& b) { return a.off < b.off; });
        int64_t off = 0;
        for (const Placed& p : live) {
            if (off + size <= p.off) break;
            off = std::max(off, p.off + p.size);
        }
        placed.push_back({off, size, first[t], last[t]});
        g.offset[t] = off;
        top = std::max(top, off + size);
    }
    g.arena_bytes = top;
}

// Micro-batches of one forward of `batch` crops, segment by segment: fn(segment, first crop, crops).
template <class F>
void for_each_micro_batch(const Graph& g, int batch, F fn) {
    for (const Segment& sg : g.segs) {
        const int mb = (sg.micro_batch > 0 && sg.micro_batch < batch) ? sg.micro_batch : batch;
        for (int64_t b0 = 0; b0 < batch && sg.first_launch < sg.end_launch; b0 += mb)
            fn(sg, b0, (int)std::min<int64_t>(mb, batch - b0));
    }
}

}  // namespace
}  // namespace mvp

using mvp::Graph;
using mvp::Launch;

extern "C" int mvp_graph_create(const mvp_tensor_desc* tensors, int n_tensors, const mvp_op_desc* ops, int n_ops,
                                const int* seg_micro_batch, int n_segments, int input_tensor, int output_tensor,
                                const uint16_t* w_dev, int64_t w_elems, const float* f_dev, int64_t f_elems,
                                int max_batch, void** handle_out) {
    MVP_ABI_BEGIN
    MVP_REQUIRE(handle_out != nullptr, "mvp_graph_create: handle_out is NULL");
    *handle_out = nullptr;
    MVP_REQUIRE(tensors && n_tensors > 0 && ops && n_ops > 0, "mvp_graph_create: empty graph");
    MVP_REQUIRE(input_tensor >= 0 && input_tensor < n_tensors && output_tensor >= 0 && output_tensor < n_tensors &&
                    input_tensor != output_tensor,
                "mvp_graph_create: bad input/output tensor ids");
    MVP_REQUIRE(max_batch > 0, "mvp_graph_create: max_batch must be > 0");
    MVP_REQUIRE(seg_micro_batch && n_segments > 0, "mvp_graph_create: segments missing");
    Graph* g = new Graph();
    try {
        g->tensors.assign(tensors, tensors + n_tensors);
        g->ops.assign(ops, ops + n_ops);
        g->input = input_tensor;
        g->output = output_tensor;
        g->wb = w_dev;
        g->fb = f_dev;
        g->max_batch = max_batch;
        g->segs.resize(n_segments);
        for (int i = 0; i < n_segments; i++) {
            MVP_REQUIRE(seg_micro_batch[i] >= 0, "mvp_graph_create: negative micro-batch");
            g->segs[i].micro_batch = seg_micro_batch[i];
        }
        mvp::validate(*g, w_elems, f_elems);
        g->owner.assign(n_ops, -1);
        g->launches.reserve(n_ops);  // the passes hold Launch references across emit()
        g->sw = mvp::read_switches();
        g->cus = mvp::cu_count();
        if (!g->sw.no_fuse) {  // each pass looks at its own switch
            mvp::fuse(*g);
            mvp::cat_fuse(*g);
            mvp::bneck_fuse(*g);
            mvp::pair_fuse(*g);
            mvp::stem_fuse(*g);
            mvp::twin_fuse(*g);
            mvp::planar_fuse(*g);
            mvp::sib_fuse(*g);
            mvp::head_fuse(*g);
        }
        mvp::finish_launches(*g);
        mvp::select_kernels(*g);
        mvp::alloc_weights(*g);
        mvp::fill_weights(*g);
        mvp::plan(*g);
        if (g->arena_bytes > 0) {
            hipError_t e = hipMalloc(&g->arena, g->arena_bytes);
            if (e != hipSuccess)
                mvp::fail(MVP_ERR_NOMEM, "mvp_graph_create: arena of %lld bytes: %s", (long long)g->arena_bytes,
                          hipGetErrorString(e));
        }
    } catch (...) {
        mvp::free_weights(*g);
        delete g;
        throw;
    }
    *handle_out = g;
    MVP_ABI_END
}

extern "C" int mvp_graph_forward(void* handle, const void* input_dev, int batch, void* output_dev, void* stream) {
    MVP_ABI_BEGIN
    Graph* g = static_cast<Graph*>(handle);
    MVP_REQUIRE(g != nullptr, "mvp_graph_forward: NULL handle");
    MVP_REQUIRE(batch >= 0 && batch <= g->max_batch, "mvp_graph_forward: batch %d exceeds max_batch %d", batch,
                g->max_batch);
    MVP_REQUIRE(input_dev && output_dev, "mvp_graph_forward: NULL input/output");
    if (batch == 0) return MVP_OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int64_t slice = 0;  // first crop of the current micro-batch
    auto ptr = [&](int t) -> void* {
        const mvp_tensor_desc& d = g->tensors[t];
        if (g->local_seg[t] >= 0) return g->arena + g->offset[t];
        char* base = t == g->input ? (char*)const_cast<void*>(input_dev)
                     : t == g->output ? (char*)output_dev
                                      : g->arena + g->offset[t];
        return base + slice * mvp::tensor_bytes(d, 1);
    };
    auto bf16 = [&](int t) { return (uint16_t*)ptr(t); };
    auto run = [&](const Launch& L, int nb) {
        const mvp_op_desc& op = g->ops[L.op];
        const mvp_tensor_desc& o = g->tensors[op.out];
        const mvp_tensor_desc& x = g->tensors[L.reads[0]];
        const mvp::Kernel kernel = mvp::pick_kernel(L.kernel, nb, g->cus, g->sw);
        switch (L.route) {
        case mvp::R_BLOCK: {
            const mvp_op_desc& c1 = g->ops[L.op - 1];
            const uint16_t *xb = bf16(op.in[1]), *w1 = g->wb + c1.w_off, *w2 = g->wb + op.w_off;
            const float *b1 = g->fb + c1.b_off, *b2 = g->fb + op.b_off;
            uint16_t* y = bf16(op.out);
            switch (kernel) {
            case mvp::K_TBLOCK32S: mvp::launch_tblock32s(xb, w1, b1, w2, b2, y, nb, o.h, o.w, s); break;
            case mvp::K_TBLOCK32: mvp::launch_tblock32(xb, w1, b1, w2, b2, y, nb, o.h, o.w, s); break;
            case mvp::K_BASIC_BLOCK_C32: mvp::launch_basic_block_c32(xb, w1, b1, w2, b2, y, nb, o.h, o.w, s); break;
            default: mvp::launch_tblock64(xb, w1, b1, w2, b2, y, nb, o.h, o.w, kernel == mvp::K_TBLOCK64, s);
            }
            break;
        }
        case mvp::R_TWIN: {  // transition1: this 3x3/s1 conv and its 3x3/s2 sibling, one pass
            const mvp_op_desc& b = g->ops[L.twin];
            mvp::launch_trans1(bf16(op.in[0]), L.w_img, g->fb + op.b_off, g->fb + b.b_off, bf16(op.out),
                               bf16(b.out), nb, L.planar, s);
            break;
        }
        case mvp::R_SIBLINGS: {  // this 3x3/s2 conv and its siblings on the same input
            mvp::S2Multi m;
            m.x = bf16(op.in[0]), m.w = L.w, m.bias = L.b;
            m.N = nb, m.H = x.h, m.W = x.w, m.Cin = op.cin;
            m.n_out = (int)L.covers.size();
            for (int i = 0; i < m.n_out; i++) {
                const mvp_op_desc& o2 = g->ops[L.covers[i]];
                m.y[i] = bf16(o2.out), m.cout[i] = o2.cout, m.relu[i] = o2.relu;
            }
            mvp::launch_s2conv_multi(m, s);
            break;
        }
        case mvp::R_HEAD_FUSE: {  // the last fuse layer's out0, formed per pixel by the head
            const mvp_op_desc& f = g->ops[L.fuse];
            const mvp_tensor_desc& fo = g->tensors[f.out];
            const uint16_t* ins[4];
            for (int i = 0; i < f.n_in; i++) ins[i] = bf16(f.in[i]);
            mvp::launch_head_fuse(ins, f.up, f.n_in, f.relu, g->wb + op.w_off, g->fb + op.b_off, (float*)ptr(op.out),
                                  nb, fo.h, fo.w, s);
            break;
        }
        case mvp::R_BNECK: {  // the whole Bottleneck: conv1 + conv2 + this conv3
            const mvp_op_desc& a = g->ops[L.conv1];
            const mvp_op_desc& c2 = g->ops[L.conv2];
            mvp::BneckLaunch bl;
            bl.x = bf16(a.in[0]);
            bl.w1 = g->wb + a.w_off, bl.b1 = g->fb + a.b_off;
            bl.w2 = g->wb + c2.w_off, bl.b2 = g->fb + c2.b_off;
            bl.w3 = L.lead ? L.w : g->wb + op.w_off, bl.b3 = L.lead ? L.b : g->fb + op.b_off;
            bl.y = bf16(op.out);
            bl.N = nb, bl.H = x.h, bl.W = x.w;
            bl.perm = L.perm, bl.lead = L.lead, bl.planar = L.planar;
            mvp::launch_bneck(bl, s);
            break;
        }
        case mvp::R_STEM2: {  // stem conv1 + this conv2 in one launch
            const mvp_op_desc& st = g->ops[L.stem];
            mvp::launch_stem2(bf16(st.in[0]), g->fb + st.w_off, g->fb + st.b_off, g->wb + op.w_off, g->fb + op.b_off,
                              bf16(op.out), nb, x.h, x.w, kernel == mvp::K_STEM2, s);
            break;
        }
        case mvp::R_STEM:
            mvp::launch_stem(bf16(op.in[0]), g->fb + op.w_off, g->fb + op.b_off, bf16(op.out), nb, x.h, x.w, s);
            break;
        case mvp::R_CONV:
        case mvp::R_PAIR: {
            mvp::ConvLaunch c{};
            c.x = bf16(op.in[0]);
            c.w = g->wb + op.w_off, c.bias = g->fb + op.b_off;
            c.res = mvp::has_res(op) ? bf16(op.in[1]) : nullptr;
            c.out_f32_nchw = o.dtype == MVP_DT_F32_NCHW;
            c.y = c.out_f32_nchw ? nullptr : bf16(op.out);
            c.yf = c.out_f32_nchw ? (float*)ptr(op.out) : nullptr;
            c.N = nb, c.H = x.h, c.W = x.w;
            c.Cin = op.cin, c.Cout = op.cout, c.ks = op.ks, c.stride = op.stride, c.relu = op.relu;
            c.w_img = L.w_img, c.s2_tile = g->sw.s2_tile;
            if (L.cat_src >= 0) {  // cat-fused: [in[0], absorbed op's input] x [W | W_absorbed]
                const mvp_op_desc& a = g->ops[L.cat_src];
                c.x2 = bf16(a.in[0]), c.c1 = op.cin, c.Cin = op.cin + a.cin;
                c.w = L.w, c.bias = L.b, c.res = nullptr;
            }
            if (L.route == mvp::R_CONV) {
                switch (kernel) {
                case mvp::K_HEAD1X1: mvp::launch_head1x1(c, s); break;
                case mvp::K_CONV1X1_WIDE: mvp::launch_conv1x1_wide(c, s); break;
                case mvp::K_CONV1X1: mvp::launch_conv1x1_direct(c, s); break;
                case mvp::K_TCONV: mvp::launch_tconv(c, s); break;
                case mvp::K_TCONV16: mvp::launch_tconv16(c, s); break;
                case mvp::K_S2CONV: mvp::launch_s2conv(c, s); break;
                default: mvp::launch_conv_generic(c, s);
                }
                break;
            }
            const mvp_op_desc& b = g->ops[L.tail];  // Bottleneck join: this conv + the next block's conv1
            mvp::PairLaunch pl;
            pl.x = c.x, pl.x2 = c.x2;
            pl.c1 = c.x2 ? c.c1 : c.Cin, pl.c2 = c.x2 ? c.Cin - c.c1 : 0;
            pl.w1 = c.w, pl.b1 = c.bias, pl.res = c.res, pl.y = c.y;
            pl.w2 = g->wb + b.w_off, pl.b2 = g->fb + b.b_off, pl.y2 = bf16(b.out);
            pl.n_pix = (long)nb * x.h * x.w;
            mvp::launch_conv1x1_pair(pl, s);
            break;
        }
        case mvp::R_FUSE_SUM: {
            const uint16_t* ins[4];
            for (int i = 0; i < op.n_in; i++) ins[i] = bf16(op.in[i]);
            mvp::launch_fuse_sum(ins, op.up, op.n_in, bf16(op.out), nb, o.h, o.w, o.c, op.relu, s);
            break;
        }
        }
    };
    mvp::for_each_micro_batch(*g, batch, [&](const mvp::Segment& sg, int64_t b0, int nb) {
        slice = b0;
        for (int l = sg.first_launch; l < sg.end_launch; l++) run(g->launches[l], nb);
    });
    MVP_ABI_END
}

// Launch plan of one forward (diagnostics for tools/fwd_breakdown.py: pairs the kernel trace with
// the graph's MACs so each kernel family gets its FLOP and MFMA fraction).  One record per kernel
// launch, in launch order: {launching op, route, crops in the launch, MACs of every op it covers}.
extern "C" int mvp_graph_plan(void* handle, int batch, int64_t* rec_out, int max_records, int* n_records,
                              int64_t* covered_macs_out) {
    MVP_ABI_BEGIN
    Graph* g = static_cast<Graph*>(handle);
    MVP_REQUIRE(g && rec_out && n_records, "mvp_graph_plan: NULL pointer");
    MVP_REQUIRE(batch > 0 && batch <= g->max_batch, "mvp_graph_plan: batch %d", batch);
    int n = 0;
    int64_t total = 0;
    mvp::for_each_micro_batch(*g, batch, [&](const mvp::Segment& sg, int64_t, int nb) {
        for (int l = sg.first_launch; l < sg.end_launch; l++, n++) {
            const Launch& L = g->launches[l];
            total += L.macs * nb;
            if (n >= max_records) continue;
            const int64_t rec[4] = {L.op, L.route, nb, L.macs * nb};
            std::copy(rec, rec + 4, rec_out + 4 * n);
        }
    });
    *n_records = n;
    if (covered_macs_out) *covered_macs_out = total;
    MVP_ABI_END
}

// The kernel of each launch of one forward of `batch` crops: one id (kernel_select.h Kernel;
// its name from mvp_graph_kernel_name) per record of mvp_graph_plan, in the same order.  A
// smaller last micro-batch may run another kernel than the full ones.
extern "C" int mvp_graph_kernels(void* handle, int batch, int* kernels_out, int max_records, int* n_records) {
    MVP_ABI_BEGIN
    Graph* g = static_cast<Graph*>(handle);
    MVP_REQUIRE(g && kernels_out && n_records, "mvp_graph_kernels: NULL pointer");
    MVP_REQUIRE(batch > 0 && batch <= g->max_batch, "mvp_graph_kernels: batch %d", batch);
    int n = 0;
    mvp::for_each_micro_batch(*g, batch, [&](const mvp::Segment& sg, int64_t, int nb) {
        for (int l = sg.first_launch; l < sg.end_launch; l++, n++)
            if (n < max_records) kernels_out[n] = mvp::pick_kernel(g->launches[l].kernel, nb, g->cus, g->sw);
    });
    *n_records = n;
    MVP_ABI_END
}

extern "C" const char* mvp_graph_kernel_name(int kernel) { return mvp::kernel_name(kernel); }

// The blobs were rewritten in place (e.g. a weight broadcast from rank 0 after the graph was
// built): re-derive every weight the graph copied out of them at create time.  Blocking.
extern "C" int mvp_graph_refresh_weights(void* handle) {
    MVP_ABI_BEGIN
    Graph* g = static_cast<Graph*>(handle);
    MVP_REQUIRE(g != nullptr, "mvp_graph_refresh_weights: NULL handle");
    MVP_HIP(hipDeviceSynchronize());
    mvp::fill_weights(*g);
    MVP_ABI_END
}

extern "C" int mvp_graph_arena_bytes(void* handle, int64_t* bytes_out) {
    MVP_ABI_BEGIN
    MVP_REQUIRE(handle && bytes_out, "mvp_graph_arena_bytes: NULL argument");
    *bytes_out = static_cast<Graph*>(handle)->arena_bytes;
    MVP_ABI_END
}

extern "C" int mvp_graph_destroy(void* handle) {
    MVP_ABI_BEGIN
    Graph* g = static_cast<Graph*>(handle);
    if (g) {
        if (g->arena) (void)hipFree(g->arena);
        mvp::free_weights(*g);
        delete g;
    }
    MVP_ABI_END
}
