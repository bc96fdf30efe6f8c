"""The graph's kernel selection (csrc/kernel_select.h) without a device: tools/kernel_select_check.cpp
is built with the host compiler and asked, for every conv of HRNet-W32 and the BasicBlock planes of
test_conv_planes_gpu.py, which kernel it selects under the default switches, under each kernel
switch, and with MVPOSE_CROP_STREAM on and off at a batch below and at the CU count.  The expected
answers are written out by hand from the launcher chains this selection replaced (launch_conv ->
head1x1 | conv1x1_direct (-> wide) | tconv (-> tconv16) | s2conv | generic; launch_basic_block_c32 ->
tblock32s | tblock32 | basic_block_c32_kernel; tblock64 and stem2 by crop_ranges_balanced).  The
weight image a selected kernel implies must be the one the old tconv16_image_elems formula,
restated below, allocated under the default switches.

The person detector's selection (csrc/det_select.h) is asked the same way, through the same
program: every distinct op shape of RTMDet-m at 640 and at the 160 and 128 sizes the GPU tests use,
under the default switches, under each value of each switch and on a part too small for the band
kernel, against answers written out by hand from the chains it replaced (launch_det_conv_gemm:
band | halo | fold | persistent GEMM | GEMM; det_launch_halo: 2-row | persistent LT 3 / 4 / 2 |
live-3 | tile; launch_det_head: staged | direct), and the weight image each selected kernel implies."""
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
def exe(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    out = str(tmp_path_factory.mktemp("ksel") / "kernel_select_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-I", CSRC,
                           os.path.join(ROOT, "tools", "kernel_select_check.cpp"), "-o", out])
    return out


@pytest.fixture(scope="module")
def ask(exe):
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


# ---------------------------------------------------------------------------- person detector
STEM, CONV, DW, CA, SPP, UP2, HEAD, DWPW = range(8)  # MVP_DET_*
NO_FOLD, FOLD_UP, FOLD_CA, FOLD_LB = range(4)         # DetFold
SMALL_PART = 8  # CUs: below 8 * n_nb for every band conv (n_nb >= 2), so none gets a band group
DET_SETTINGS = ["xcd=0", "band=0", "band=4", "pers=0", "pers=3", "pers_occ=1", "fold=0", "halo_pers=0", "halo_rows2=1",
                "live=0", "head_direct=1"]



# what a class of ops runs: the default, then each setting that changes it; "small": on SMALL_PART
def ONE(name):
    return {"default": name}


HALO_24 = {"default": "halo_pers_lt2", "halo_pers=0": "halo", "halo_rows2=1": "halo_2row"}  # 24 live couts of 32
# 48 live couts of 64: live == 48 goes to the persistent kernel before the live-3 tile form is asked
HALO_48 = {"default": "halo_pers_lt3", "halo_pers=0": "halo_live3", "halo_rows2=1": "halo_2row"}
GEMM3 = {"default": "gemm", "pers=3": "pers_gemm"}  # a 3x3 conv on the GEMM path
BAND = {"default": "band_8w", "band=4": "band_4w", "band=0": "gemm", "small": "gemm"}
PERS1 = {"default": "pers_gemm", "pers=0": "gemm"}  # a 1x1 conv
UP = {"default": "fold_up"}   # asked with the fold plan_folds gives it; with pers=0 or fold=0 plan_folds gives none
CAF = {"default": "fold_ca"}
HEADS = {"default": "head_staged", "head_direct=1": "head_direct"}


def band_or_gemm(h):
    """The 3x3/s1 convs with >= 96 input channels: the band kernel on the 80x80 / 40x40 planes."""
    return BAND if h in (80, 40) else GEMM3


# (kind, cin, cout, ks, stride, live couts, residual, fold): the planes (h = w) it has at 640, 160
# and 128, and what it runs (a function of the plane where that decides).  RTMDet-m's ops by
# distinct shape, with MVPOSE_DET_DWPW on and off; the 1x1 convs behind an upsample or an attention
# also as plan_folds hands them over.
DET_OPS = {
    (STEM, 4, 32, 3, 2, 0, 0, NO_FOLD): ((640, 160, 128), ONE("stem")),
    (STEM, 4, 32, 3, 2, 0, 0, FOLD_LB): ((640, 160, 128), ONE("letterbox_stem")),
    (CONV, 32, 32, 3, 1, 24, 0, NO_FOLD): ((320, 80, 64), HALO_24),  # stem.1: cin 32 is no band conv at 80
    (CONV, 32, 64, 3, 1, 48, 0, NO_FOLD): ((320, 80, 64), HALO_48),
    (CONV, 64, 96, 3, 2, 96, 0, NO_FOLD): ((320, 80, 64), GEMM3),
    (CONV, 96, 128, 1, 1, 112, 0, NO_FOLD): ((160, 40, 32), PERS1),
    (CONV, 64, 64, 3, 1, 48, 0, NO_FOLD): ((160, 40, 32), HALO_48),
    (DWPW, 64, 64, 5, 1, 0, 1, NO_FOLD): ((160, 40, 32), ONE("dwpw")),
    (CA, 128, 0, 0, 1, 0, 0, NO_FOLD): ((160, 40, 32), ONE("ca_pool")),
    (CONV, 128, 96, 1, 1, 96, 0, NO_FOLD): ((160, 40, 32), PERS1),
    (CONV, 128, 96, 1, 1, 96, 0, FOLD_CA): ((160, 40, 32), CAF),
    (CONV, 96, 192, 3, 2, 192, 0, NO_FOLD): ((160, 40, 32), GEMM3),
    (CONV, 192, 192, 1, 1, 192, 0, NO_FOLD): ((80, 40, 20, 16, 10, 8), PERS1),
    (CONV, 192, 192, 1, 1, 192, 0, FOLD_CA): ((80, 20, 16), CAF),
    (CONV, 96, 96, 3, 1, 96, 0, NO_FOLD): ((80, 20, 16), band_or_gemm),
    (DWPW, 96, 96, 5, 1, 0, 1, NO_FOLD): ((80, 20, 16), ONE("dwpw")),
    (DWPW, 96, 96, 5, 1, 0, 0, NO_FOLD): ((80, 20, 16), ONE("dwpw")),
    (CA, 192, 0, 0, 1, 0, 0, NO_FOLD): ((80, 20, 16), ONE("ca_pool")),
    (CONV, 192, 384, 3, 2, 384, 0, NO_FOLD): ((80, 20, 16), GEMM3),
    (CONV, 384, 384, 1, 1, 384, 0, NO_FOLD): ((40, 20, 10, 8, 5, 4), PERS1),
    (CONV, 384, 384, 1, 1, 384, 0, FOLD_CA): ((40, 10, 8), CAF),
    (CONV, 192, 192, 3, 1, 192, 0, NO_FOLD): ((80, 40, 20, 16, 10, 8, 5, 4), band_or_gemm),
    (DW, 192, 192, 5, 1, 0, 0, NO_FOLD): ((40, 10, 8), ONE("dw5")),
    (CONV, 192, 192, 1, 1, 192, 1, NO_FOLD): ((40, 10, 8), PERS1),
    (CA, 384, 0, 0, 1, 0, 0, NO_FOLD): ((40, 10, 8), ONE("ca_pool")),
    (CONV, 384, 768, 3, 2, 768, 0, NO_FOLD): ((40, 10, 8), GEMM3),
    (CONV, 768, 384, 1, 1, 384, 0, NO_FOLD): ((40, 20, 10, 8, 5, 4), PERS1),
    (CONV, 768, 384, 1, 1, 384, 0, FOLD_UP): ((40, 10, 8), UP),
    (SPP, 384, 0, 0, 1, 0, 0, NO_FOLD): ((20, 5, 4), ONE("spp")),
    (CONV, 1536, 768, 1, 1, 768, 0, NO_FOLD): ((20, 5, 4), PERS1),
    (CONV, 768, 768, 1, 1, 768, 0, NO_FOLD): ((20, 5, 4), PERS1),
    # the scale fold's tables hold 8 frames per 128-pixel tile: a 4x4 plane's tile spans 9
    (CONV, 768, 768, 1, 1, 768, 0, FOLD_CA): ((20, 5, 4), lambda h: ONE("none") if h == 4 else CAF),
    (CONV, 384, 384, 3, 1, 384, 0, NO_FOLD): ((20, 5, 4), GEMM3),
    (DW, 384, 384, 5, 1, 0, 0, NO_FOLD): ((20, 5, 4), ONE("dw5")),
    (CA, 768, 0, 0, 1, 0, 0, NO_FOLD): ((20, 5, 4), ONE("ca_pool")),
    (UP2, 384, 384, 0, 1, 0, 0, NO_FOLD): ((20, 5, 4), ONE("up2")),
    (CONV, 384, 192, 1, 1, 192, 0, NO_FOLD): ((80, 40, 20, 16, 10, 8), PERS1),
    (CONV, 384, 192, 1, 1, 192, 0, FOLD_UP): ((80, 20, 16), UP),
    (UP2, 192, 192, 0, 1, 0, 0, NO_FOLD): ((40, 10, 8), ONE("up2")),
    (CONV, 192, 192, 3, 2, 192, 0, NO_FOLD): ((80, 20, 16), GEMM3),
    (CONV, 384, 384, 3, 2, 384, 0, NO_FOLD): ((40, 10, 8), GEMM3),
    (CONV, 384, 192, 3, 1, 192, 0, NO_FOLD): ((40, 10, 8), band_or_gemm),
    (CONV, 768, 192, 3, 1, 192, 0, NO_FOLD): ((20, 5, 4), GEMM3),
    (CONV, 192, 384, 3, 1, 384, 0, NO_FOLD): ((80, 40, 20, 16, 10, 8, 5, 4), band_or_gemm),
    (HEAD, 384, 0, 1, 8, 0, 0, NO_FOLD): ((80, 20, 16), HEADS),
    (HEAD, 384, 0, 1, 16, 0, 0, NO_FOLD): ((40, 10, 8), HEADS),
    (HEAD, 384, 0, 1, 32, 0, 0, NO_FOLD): ((20, 5, 4), HEADS),
    # MVPOSE_DET_DWPW=0: the blocks' depthwise and pointwise convs apart
    (DW, 64, 64, 5, 1, 0, 0, NO_FOLD): ((160, 40, 32), ONE("dw5")),
    (CONV, 64, 64, 1, 1, 48, 1, NO_FOLD): ((160, 40, 32), PERS1),
    (DW, 96, 96, 5, 1, 0, 0, NO_FOLD): ((80, 20, 16), ONE("dw5")),
    (CONV, 96, 96, 1, 1, 96, 1, NO_FOLD): ((80, 20, 16), PERS1),
    (CONV, 96, 96, 1, 1, 96, 0, NO_FOLD): ((80, 20, 16), PERS1),
}


def _det_cases():
    """(op key, plane, what it runs there)"""
    for key, (planes, runs) in DET_OPS.items():
        for h in planes:
            yield key, h, runs(h) if callable(runs) else runs


@pytest.fixture(scope="module")
def ask_det(exe):
    def run(queries):
        """[(op key, plane, CUs, settings)] -> [(variant, image elements)]"""
        text = "".join(f"det {k[0]} {h} {h} {' '.join(map(str, k[1:]))} {cus} {' '.join(sw)}\n" for k, h, cus, sw in queries)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(queries)
        return [(a, int(b)) for a, b in (line.split() for line in out)]
    return run


def test_detector_ops_match_the_launcher_chains(ask_det):
    queries, want = [], []
    for key, h, runs in _det_cases():
        for sw in [()] + [(s,) for s in DET_SETTINGS]:
            queries.append((key, h, CUS, sw))
            want.append(runs.get(sw[0], runs["default"]) if sw else runs["default"])
        queries.append((key, h, SMALL_PART, ()))
        want.append(runs.get("small", runs["default"]))
        queries.append((key, h, SMALL_PART, ("pers=3",)))  # the band convs' fallback is the whole GEMM path
        want.append({"gemm": "pers_gemm"}.get(want[-1], want[-1]) if key[0] == CONV and key[3] == 3 else want[-1])
    got = ask_det(queries)
    for q, g, w in zip(queries, got, want):
        assert g[0] == w, f"op {q[0]} at {q[1]}x{q[1]}, {q[2]} CUs, switches {q[3]}: selected {g[0]}, the chain gives {w}"
    assert {w for w in want} >= {"band_8w", "band_4w", "halo_2row", "halo", "halo_live3", "halo_pers_lt2", "halo_pers_lt3",
                                 "fold_up", "fold_ca", "pers_gemm", "gemm", "head_staged", "head_direct"}


def test_detector_shapes_outside_rtmdet(ask_det):
    """The branches of the chains RTMDet-m does not reach."""
    full64 = (CONV, 64, 64, 3, 1, 64, 0, NO_FOLD)   # all 64 couts live: the persistent halo kernel's 4-tile form
    res48 = (CONV, 64, 64, 3, 1, 48, 1, NO_FOLD)    # a residual: neither the persistent nor the live-3 form
    live40 = (CONV, 64, 64, 3, 1, 40, 0, NO_FOLD)   # 33..47 live couts: the live-3 tile form, unless switched off
    c32_64 = (CONV, 64, 32, 3, 1, 32, 0, NO_FOLD)   # 64 -> 32: two input chunks have no persistent form
    got = ask_det([(full64, 64, CUS, ()), (full64, 64, CUS, ("halo_pers=0",)), (res48, 64, CUS, ()),
                   (live40, 64, CUS, ()), (live40, 64, CUS, ("live=0",)), (c32_64, 64, CUS, ()),
                   ((CONV, 192, 1056, 1, 1, 0, 0, NO_FOLD), 20, CUS, ()),   # > 1024 couts: no persistent GEMM
                   ((CONV, 96, 128, 1, 1, 112, 0, FOLD_CA), 40, CUS, ()),   # 128-cout tiles: no fold kernel
                   ((CONV, 48, 64, 1, 1, 0, 0, NO_FOLD), 20, CUS, ()),      # cin not a multiple of 32
                   ((CONV, 64, 64, 5, 1, 0, 0, NO_FOLD), 20, CUS, ()),      # 5x5
                   ((HEAD, 80, 0, 1, 8, 0, 0, NO_FOLD), 20, CUS, ()),       # 40 feature channels: not whole staging steps
                   ((DWPW, 128, 128, 5, 1, 0, 0, NO_FOLD), 20, CUS, ())])
    assert [g[0] for g in got] == ["halo_pers_lt4", "halo", "halo", "halo_live3", "halo", "halo", "gemm", "none", "none",
                                   "none", "head_direct", "none"]


def test_detector_weight_images_follow_the_selection(ask_det):
    """npad x K elements for exactly the GEMM, persistent GEMM, fold and dwpw ops, the band image's
    det_band_rows(npad) x K for the band ops, none for the others, under every setting."""
    queries = [(key, h, cus, sw) for key, h, _ in _det_cases() for cus in (CUS, SMALL_PART)
               for sw in [()] + [(s,) for s in DET_SETTINGS]]
    seen = set()
    for (key, h, cus, sw), (variant, elems) in zip(queries, ask_det(queries)):
        kind, cin, cout, ks = key[:4]
        npad = (cout + 31) // 32 * 32
        K = cin if kind == DWPW else ks * ks * cin
        if variant in ("gemm", "pers_gemm", "fold_up", "fold_ca", "dwpw"):
            want = npad * K
        elif variant in ("band_8w", "band_4w"):
            want = (npad + 63) // 64 * 64 * K
        else:
            want = 0
        assert elems == want, f"op {key} at {h}: {variant} with an image of {elems} elements, not {want}"
        seen.add((variant, elems > 0))
    assert ("band_8w", True) in seen and ("halo_pers_lt3", False) in seen and ("dwpw", True) in seen


def test_table_lists_every_rtmdet_op(monkeypatch):
    """DET_OPS is RTMDet-m's ops by distinct shape at 640, 160 and 128, fused dw + pw or apart."""
    sys.path.insert(0, os.path.join(ROOT, "multi-camera_3d_pose_estimation_amd"))
    from mvpose import rtmdet
    sd = rtmdet.random_state_dict(0)
    shapes = {}
    for size in (640, 160, 128):
        for dwpw in ("1", "0"):
            monkeypatch.setenv("MVPOSE_DET_DWPW", dwpw)
            spec, _ = rtmdet.build_rtmdet_m(sd, size)
            for k, op in enumerate(spec.ops):
                h, w = spec.tensors[op.in_.t][:2]
                assert h == w
                conv = op.kind == CONV
                key = (op.kind, op.in_.c, op.out.c if op.out.t >= 0 else 0, op.ks, op.stride, op.aux if conv else 0,
                       int(op.kind in (CONV, DWPW) and op.res.t >= 0))
                folds = {NO_FOLD}
                if k == 0:
                    folds.add(FOLD_LB)
                elif conv and op.ks == 1 and spec.ops[k - 1].kind == CA:
                    folds.add(FOLD_CA)
                elif conv and op.ks == 1 and spec.ops[k - 1].kind == UP2:
                    folds.add(FOLD_UP)
                for f in folds:
                    shapes.setdefault(key + (f,), set()).add(h)
    assert {k: tuple(sorted(v, reverse=True)) for k, v in shapes.items()} == {k: v[0] for k, v in DET_OPS.items()}
