"""The graph's kernel selection (csrc/kernel_select.h) without a device: tools/kernel_select_check.cpp
is built with the host compiler and asked, for every conv of HRNet-W32 and the BasicBlock planes of
test_conv_planes_gpu.py, which kernel it selects under the default switches, under each kernel
switch, and with MVPOSE_CROP_STREAM on and off at a batch below and at the CU count.  The expected
answers are written out by hand from the launcher chains this selection replaced (launch_conv ->
head1x1 | conv1x1_direct (-> wide) | tconv (-> tconv16) | s2conv | generic; launch_basic_block_c32 ->
tblock32s | tblock32 | basic_block_c32_kernel; tblock64 and stem2 by crop_ranges_balanced).  The
weight image a selected kernel implies must be the one the old tconv16_image_elems formula,
restated below, allocated under the default switches."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-camera_3d_pose_estimation_amd", "csrc")
R_BLOCK, R_STEM2, R_STEM, R_CONV = 1, 6, 7, 8
CUS = 256
SWITCHES = ["no_tconv", "no_tconv16", "no_s2conv", "no_head1x1", "no_tblock", "no_tblock32s"]

GEN, C11, WIDE, HEAD = "conv_mfma_kernel", "conv1x1_kernel", "conv1x1_pair_kernel", "head1x1_kernel"
TC, T16, S2 = "tconv_kernel", "tconv16_kernel", "s2conv_kernel"
T_OFF = {"no_tconv": GEN}
T16_OFF = {"no_tconv": GEN, "no_tconv16": TC}
S2_OFF = {"no_s2conv": GEN}

# (cin, cout, h, w, ks, stride, relu, res, f32 out, cat): kernel under the default switches, then
# the kernel under each switch that changes it.  h x w is the input plane; cat is the first
# input's channels of a cat-fused 1x1 (cin then counts both inputs).
CONVS = {
    # heatmap head
    (32, 17, 64, 48, 1, 1, 0, 0, 1, 0): (HEAD, {"no_head1x1": GEN}),
    # layer1's 1x1 convs: conv1, the downsample, conv3 (+ residual: one wave per 256 couts),
    # conv3 cat-fused with the downsample
    (64, 64, 64, 48, 1, 1, 1, 0, 0, 0): (C11, {}),
    (64, 256, 64, 48, 1, 1, 0, 0, 0, 0): (C11, {}),
    (64, 256, 64, 48, 1, 1, 1, 1, 0, 0): (WIDE, {}),
    (256, 64, 64, 48, 1, 1, 1, 0, 0, 0): (C11, {}),
    (128, 256, 64, 48, 1, 1, 1, 0, 0, 64): (WIDE, {}),
    # fuse-layer 1x1 projections
    (64, 32, 32, 24, 1, 1, 0, 0, 0, 0): (C11, {}),
    (128, 32, 16, 12, 1, 1, 0, 0, 0, 0): (C11, {}),
    (128, 64, 16, 12, 1, 1, 0, 0, 0, 0): (C11, {}),
    (256, 32, 8, 6, 1, 1, 0, 0, 0, 0): (C11, {}),
    (256, 64, 8, 6, 1, 1, 0, 0, 0, 0): (C11, {}),
    (256, 128, 8, 6, 1, 1, 0, 0, 0, 0): (C11, {}),
    # 3x3/s1: BasicBlock convs per branch (conv1, conv2 + residual), layer1's conv2, transition1.0
    (32, 32, 64, 48, 3, 1, 1, 0, 0, 0): (GEN, {}),
    (32, 32, 64, 48, 3, 1, 1, 1, 0, 0): (GEN, {}),
    (64, 64, 64, 48, 3, 1, 1, 0, 0, 0): (TC, T_OFF),
    (64, 64, 64, 48, 3, 1, 1, 1, 0, 0): (TC, T_OFF),  # test_conv_planes_gpu's (64, 64, 48) plane
    (256, 32, 64, 48, 3, 1, 1, 0, 0, 0): (TC, T_OFF),
    (64, 64, 32, 24, 3, 1, 1, 0, 0, 0): (TC, T_OFF),
    (64, 64, 32, 24, 3, 1, 1, 1, 0, 0): (TC, T_OFF),
    (128, 128, 16, 12, 3, 1, 1, 0, 0, 0): (T16, T16_OFF),
    (128, 128, 16, 12, 3, 1, 1, 1, 0, 0): (T16, T16_OFF),
    (256, 256, 8, 6, 3, 1, 1, 0, 0, 0): (T16, T16_OFF),
    (256, 256, 8, 6, 3, 1, 1, 1, 0, 0): (T16, T16_OFF),
    # 3x3/s2: stem conv2, the fuse-layer chains and transitions (three planes stay on the generic
    # kernel, which measured faster there)
    (64, 64, 128, 96, 3, 2, 1, 0, 0, 0): (GEN, {}),
    (32, 32, 64, 48, 3, 2, 1, 0, 0, 0): (GEN, {}),
    (32, 64, 64, 48, 3, 2, 0, 0, 0, 0): (S2, S2_OFF),
    (256, 64, 64, 48, 3, 2, 1, 0, 0, 0): (GEN, {}),
    (32, 32, 32, 24, 3, 2, 1, 0, 0, 0): (GEN, {}),
    (32, 128, 32, 24, 3, 2, 0, 0, 0, 0): (S2, S2_OFF),
    (64, 64, 32, 24, 3, 2, 1, 0, 0, 0): (GEN, {}),
    (64, 128, 32, 24, 3, 2, 1, 0, 0, 0): (S2, S2_OFF),
    (64, 128, 32, 24, 3, 2, 0, 0, 0, 0): (S2, S2_OFF),
    (32, 256, 16, 12, 3, 2, 0, 0, 0, 0): (S2, S2_OFF),
    (64, 256, 16, 12, 3, 2, 0, 0, 0, 0): (S2, S2_OFF),
    (128, 256, 16, 12, 3, 2, 1, 0, 0, 0): (S2, S2_OFF),
    (128, 256, 16, 12, 3, 2, 0, 0, 0, 0): (S2, S2_OFF),
}

TB32, TB32S, BB32 = "tblock32_kernel", "tblock32s_kernel", "basic_block_c32_kernel"
TB64, TB64T = "tblock64_kernel", "tblock64_kernel:tiles"
# (route, cin, h, w): (kernel below one crop per CU, kernel from there on) under the default
# switches, then under each switch that changes them
BATCHED = {
    (R_BLOCK, 32, 64, 48): ((TB32, TB32S), {"no_tblock": (BB32, BB32), "no_tblock32s": (TB32, TB32)}),
    (R_BLOCK, 32, 32, 48): ((TB32, TB32), {"no_tblock": (BB32, BB32)}),  # other frame sizes: no streaming kernel
    (R_BLOCK, 32, 40, 48): ((BB32, BB32), {}),                            # H % 16 != 0
    (R_BLOCK, 64, 32, 24): ((TB64T, TB64), {}),
    (R_STEM2, 64, 256, 192): (("stem2_tile_kernel", "stem2_kernel"), {"stem2_tile": ("stem2_tile_kernel",) * 2}),
    (R_STEM, 4, 256, 192): (("stem_mfma_kernel",) * 2, {}),
    (R_STEM, 4, 128, 96): (("stem_kernel",) * 2, {}),
}


def parent_image_elems(cin, cout, h, w, ks, stride, relu, res, f32, cat):
    """What graph.cpp's t16_elems / tconv16.hip's tconv16_image_elems allocated before the
    selection decided it (they ignored the switches)."""
    if cat or f32 or ks != 3 or (stride == 1 and not relu):
        return 0
    s1 = stride == 1 and ((cin == 128 and cout == 128 and (h, w) == (16, 12)) or
                          (cin == 256 and cout % 128 == 0 and (h, w) == (8, 6)))
    s2 = stride == 2 and (((h, w) == (32, 24) and cout == 128 and cin == 64) or
                          ((h, w) == (16, 12) and cout % 128 == 0 and cin in (32, 64, 128)))
    return cout * 9 * cin if s1 or s2 else 0


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("ksel") / "kernel_select_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-I", CSRC,
                           os.path.join(ROOT, "tools", "kernel_select_check.cpp"), "-o", exe])

    def run(queries):
        """[(route, shape 10-tuple, batch, switches)] -> [(small, stream, at batch, image elements)]"""
        text = "".join(f"{r} {' '.join(map(str, shape))} {n} {CUS} 1 {' '.join(sw)}\n" for r, shape, n, sw in queries)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(queries)
        return [(a, b, c, int(d)) for a, b, c, d in (line.split() for line in out)]
    return run


def _settings():
    """(switches, batch): default and each kernel switch, with the crop-stream switch on and off,
    below and at the CU count."""
    for sw in [()] + [(s,) for s in SWITCHES + ["stem2_tile"]]:
        for stream in ((), ("crop_stream",)):
            for n in (7, CUS):
                yield sw + stream, n


def test_hrnet_convs_match_the_launcher_chains(ask):
    queries, want = [], []
    for shape, (default, by_switch) in CONVS.items():
        for sw, n in _settings():
            queries.append((R_CONV, shape, n, sw))
            want.append(by_switch.get(sw[0], default) if sw else default)
    got = ask(queries)
    for q, g, w in zip(queries, got, want):
        assert g[:3] == (w, w, w), f"conv {q[1]} batch {q[2]} switches {q[3]}: selected {g}, the chain gives {w}"


def test_batch_dependent_launches_match_the_launcher_chains(ask):
    queries, want = [], []
    for (route, cin, h, w), (default, by_switch) in BATCHED.items():
        shape = (cin, 64 if route != R_BLOCK else cin, h, w, 3, 1 if route == R_BLOCK else 2, 1, int(route == R_BLOCK), 0, 0)
        for sw, n in _settings():
            small, stream = by_switch.get(sw[0], default) if sw else default
            queries.append((route, shape, n, sw))
            want.append((small, stream, stream if "crop_stream" in sw or n >= CUS else small))
    got = ask(queries)
    for q, g, w in zip(queries, got, want):
        assert g[:3] == w, f"route {q[0]} {q[1]} batch {q[2]} switches {q[3]}: selected {g[:3]}, the chain gives {w}"


def test_weight_images_follow_the_selection(ask):
    shapes = list(CONVS)
    got = ask([(R_CONV, s, 7, ()) for s in shapes])
    assert sum(1 for g in got if g[3]) == 10  # 4 tconv16 shapes and 6 streamed-weight s2conv shapes
    for s, g in zip(shapes, got):
        assert g[3] == parent_image_elems(*s), f"conv {s}: image of {g[3]} elements for {g[2]}"
    # a switch that takes the reading kernel away takes the image with it
    for sw in ("no_tconv", "no_tconv16", "no_s2conv"):
        for s, g in zip(shapes, ask([(R_CONV, s, 7, (sw,)) for s in shapes])):
            reads = g[2] == T16 or (g[2] == S2 and parent_image_elems(*s))
            assert g[3] == (parent_image_elems(*s) if reads else 0), f"{sw}: conv {s} runs {g[2]} with {g[3]} image elements"


def test_table_lists_every_hrnet_conv():
    """CONVS is HRNet-W32's conv ops by distinct shape, plus the cat-fused conv3 and the residual
    conv of test_conv_planes_gpu's 64-channel 64x48 plane."""
    sys.path.insert(0, os.path.join(ROOT, "multi-camera_3d_pose_estimation_amd"))
    from mvpose import hrnet
    spec, _, _ = hrnet.build_hrnet_w32(hrnet.random_state_dict(7), dict(hrnet.DEFAULT_MICRO_BATCH))
    shapes = set()
    for op in spec.ops:
        if op["kind"] == hrnet.OP_CONV:
            h, w, _, _ = spec.tensors[op["ins"][0]]
            shapes.add((op["cin"], op["cout"], h, w, op["ks"], op["stride"], op["relu"], int(len(op["ins"]) > 1),
                        int(spec.tensors[op["out"]][3] == hrnet.DT_F32), 0))
    extra = {(128, 256, 64, 48, 1, 1, 1, 0, 0, 64), (64, 64, 64, 48, 3, 1, 1, 1, 0, 0)}
    assert shapes | extra == set(CONVS)
