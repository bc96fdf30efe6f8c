"""Every HRNet conv kernel family, bit for bit, on exactly summable data.

tests/exact_cases.py builds weights and inputs whose f32 partial sums are exact in any order
(tests/test_exact_cases.py proves each case's precondition on the CPU), so a conv's bf16 result
is one fixed array whatever the MFMA K order, tile shape or fusion.  Each test here builds a
ConvGraph from a spec helper with such weights, runs it, and requires torch.equal on the bit
patterns against the float64 reference — no tolerance: a dropped tap on one tile corner, a halo
row from the neighbouring crop, a wrong channel chunk or a truncating epilogue changes bits.
Each test also asserts through ConvGraph.launch_kernels that the family it names really ran.

The fuse layers (fuse_sum_n_kernel, and the wiring hrnet.fuse_layer shares with build_hrnet_w32)
run three ways: exact weights in both regimes; selection weights on ordinary non-integer data,
where the expected output is bf16(relu(((0 + t0) + t1) + ...)) in f32 in term order; and with
the heatmap head behind them, against head_chain's f32 fma chain.

family                   tests (ids abbreviated)
conv_mfma_kernel         test_basic_blocks[128x16x12|256x8x6|64x64x48 generic], test_stride2[generic],
                         test_stem[unfused], test_transition1[unfused-1], test_head[NO_HEAD1X1]
basic_block_c32_kernel   test_basic_blocks[32x64x48 generic]
tblock32_kernel          test_basic_blocks[32x64x48 tconv]
tblock32s_kernel         test_basic_blocks[32x64x48 tconv+stream], test_streaming_over_every_cu[tblock32s]
tblock64_kernel          test_basic_blocks[64x32x24 *]
tconv_kernel             test_basic_blocks[64x64x48 tconv, 128x16x12|256x8x6 tconv64], test_projections[256x32x64x48x3],
                         test_transition1[unfused-0], test_bottlenecks[unfused]
tconv16_kernel           test_basic_blocks[128x16x12|256x8x6 tconv]
s2conv_kernel            test_stride2[s2conv], test_siblings[unfused], test_fuse_layers
s2conv_kernel (siblings) test_siblings[fused] (one launch for all siblings)
conv1x1_kernel           test_projections[1x1], test_bottleneck_join[pair off], test_fuse_layers
conv1x1_pair_kernel      test_bottleneck_join[pair on]; its wide form: test_projections[64x256x64x48x1],
                         test_bottleneck_join[pair off]
bneck_kernel             test_bottlenecks[fused]
trans1_kernel            test_transition1[fused]
stem2_kernel             test_stem[fused stream], test_streaming_over_every_cu[stem2]
stem2_tile_kernel        test_stem[fused tile]
stem_mfma_kernel         test_stem[unfused]
fuse_sum_n_kernel        test_fuse_layers, test_fuse_layers_sum_order, test_head[NO_HEADFUSE]
head_fuse_kernel         test_head[fused]
head1x1_kernel           test_head[NO_HEADFUSE]
"""
import pytest
import torch

import exact_cases as ec

pytestmark = pytest.mark.gpu

SWITCHES = ("MVPOSE_NO_FUSE", "MVPOSE_NO_CATFUSE", "MVPOSE_NO_PAIRFUSE", "MVPOSE_NO_BNECK", "MVPOSE_NO_STEMFUSE",
            "MVPOSE_NO_TRANSFUSE", "MVPOSE_NO_SIBFUSE", "MVPOSE_NO_HEADFUSE", "MVPOSE_NO_TBLOCK", "MVPOSE_NO_TBLOCK64",
            "MVPOSE_NO_HEAD1X1", "MVPOSE_NO_TBLOCK32S", "MVPOSE_MICRO_BATCH", "MVPOSE_NO_TCONV", "MVPOSE_TCONV16",
            "MVPOSE_NO_S2CONV", "MVPOSE_CROP_STREAM", "MVPOSE_STEM2_TILE", "MVPOSE_S2_TILE")
# test_conv_planes_gpu.MODES
_OFF = {"MVPOSE_NO_TCONV": "1", "MVPOSE_NO_TBLOCK": "1"}
MODES = {"generic": dict(_OFF),
         "tconv": dict(_OFF, MVPOSE_NO_TCONV="0", MVPOSE_NO_TBLOCK="0"),
         "tconv64": dict(_OFF, MVPOSE_NO_TCONV="0", MVPOSE_NO_TBLOCK="0", MVPOSE_TCONV16="0")}
STREAM = {"MVPOSE_CROP_STREAM": "1"}


def _of(kind, **where):
    out = [c for c in ec.CASES if c.kind == kind and all(getattr(c, k) == v for k, v in where.items())]
    return pytest.mark.parametrize("case", out, ids=[c.id for c in out])


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _run(case, env, monkeypatch, n=None, tile=None):
    """Build the case's graph under the switches `env`, run its input, and return (device
    output, expected output, kernels).  tile: run the case's n-crop input and reference
    repeated up to `tile` crops."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mvpose import hrnet
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    want, _ = ec.reference(case, n)
    x = ec.inputs(case, n)
    if tile:
        reps = -(-tile // x.shape[0])
        x = x.repeat(reps, 1, 1, 1)[:tile].contiguous()
        want = want.repeat(reps, 1, 1, 1)[:tile].contiguous()
    spec, xi, yo, _ = ec.spec(case, ec.weights(case))
    g = hrnet.ConvGraph(spec, xi, yo, max_batch=x.shape[0])
    out = torch.full(want.shape, float("nan"), dtype=want.dtype, device="cuda")
    g.run(x.cuda(), out)
    torch.cuda.synchronize()
    kernels = g.launch_kernels(x.shape[0])
    g.close()
    return out.cpu(), want, kernels


def _assert_exact(got, want, kernels, nchw=False):
    """Bit patterns equal; on failure the count, the first ten (n, h, w, c) with got / want, and
    the kernels."""
    assert got.shape == want.shape
    if torch.equal(_bits(got), _bits(want)):
        return
    bad = (_bits(got) != _bits(want)).nonzero()
    lines = []
    for idx in bad[:10].tolist():
        pos = (idx[0], idx[2], idx[3], idx[1]) if nchw else tuple(idx)
        lines.append(f"  (n, h, w, c) = {pos}: got {got[tuple(idx)].item()!r}, want {want[tuple(idx)].item()!r}")
    pytest.fail(f"{bad.shape[0]} of {want.numel()} elements differ; first:\n" + "\n".join(lines) +
                f"\nkernels: {kernels}", pytrace=False)


# ------------------------------------------------------------ conv families --
def _block_kernel(c, h, mode, stream):
    if c == 32:
        return "basic_block_c32_kernel" if mode == "generic" else "tblock32s_kernel" if stream else "tblock32_kernel"
    if (c, h) == (64, 32):
        return "tblock64_kernel"
    if mode == "generic":
        return "conv_mfma_kernel"
    return "tconv16_kernel" if c in (128, 256) and mode == "tconv" else "tconv_kernel"


@pytest.mark.parametrize("mode", ["generic", "tconv", "tconv+stream", "tconv64"])
@_of("block")
def test_basic_blocks(case, mode, monkeypatch):
    """Two BasicBlocks on every branch plane under test_conv_planes_gpu's kernel modes; +stream
    forces the crop-streaming kernels (tblock32s, tblock64's crop ranges) at this small batch."""
    mode, _, stream = mode.partition("+")
    got, want, kernels = _run(case, dict(MODES[mode], **(STREAM if stream else {})), monkeypatch)
    assert set(kernels) == {_block_kernel(case.args[0], case.args[1], mode, bool(stream))}, kernels
    _assert_exact(got, want, kernels)


@pytest.mark.parametrize("family", sorted(ec.TILED))
def test_streaming_over_every_cu(family, monkeypatch):
    """tblock32s and stem2 at CU count + 3 crops (8 distinct crops repeated): every workgroup
    gets a crop range, some ranges two crops, so the row rings wrap across crop boundaries."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    case = ec.BY_ID[ec.TILED[family]]
    n = torch.cuda.get_device_properties(0).multi_processor_count + 3
    got, want, kernels = _run(case, MODES["tconv"], monkeypatch, n=ec.TILE_CROPS, tile=n)
    assert set(kernels) == {family + "_kernel"}, kernels
    _assert_exact(got, want, kernels)


@pytest.mark.parametrize("mode", ["s2conv", "generic"])
@_of("s2")
def test_stride2(case, mode, monkeypatch):
    """The nine 3x3/s2 planes of test_s2conv_gpu on s2conv.hip and on the generic kernel."""
    got, want, kernels = _run(case, {"MVPOSE_NO_S2CONV": "1" if mode == "generic" else "0"}, monkeypatch)
    cin, cout, h = case.args[:3]
    stays = (cin, cout, h) in ((64, 64, 128), (256, 64, 64), (64, 64, 32))  # planes s2conv.hip leaves to conv.hip
    assert kernels == ["conv_mfma_kernel" if mode == "generic" or stays else "s2conv_kernel"]
    _assert_exact(got, want, kernels)


@pytest.mark.parametrize("fused", [True, False])
@_of("sibling")
def test_siblings(case, fused, monkeypatch):
    """A fuse layer's 3x3/s2 siblings as one launch over cout-concatenated weights and one each."""
    got, want, kernels = _run(case, {"MVPOSE_NO_SIBFUSE": "0" if fused else "1"}, monkeypatch)
    if fused:
        assert kernels == ["s2conv_kernel"]
    else:
        assert len(kernels) == case.args[0] and kernels[0] == "s2conv_kernel", kernels
    _assert_exact(got, want, kernels)


@_of("projection")
def test_projections(case, monkeypatch):
    """y = relu(conv_b(x) + conv_a(x)): where the graph cat-fuses the two 1x1 convs (one launch)
    conv_a's output is never rounded, elsewhere it is a bf16 tensor."""
    got, want, kernels = _run(case, {}, monkeypatch)
    cin, cout, _, _, k = case.args
    assert len(kernels) == (1 if ec.cat_fused(cin, k) else 2), kernels
    family = "tconv_kernel" if k == 3 else "conv1x1_pair_kernel" if (cin, cout) == (64, 256) else "conv1x1_kernel"
    assert family in kernels, kernels
    _assert_exact(got, want, kernels)


@pytest.mark.parametrize("pair", [True, False])
@_of("join")
def test_bottleneck_join(case, pair, monkeypatch):
    """Layer1's join with the downsample cat-fused or a ReLU tensor, as one conv1x1_pair launch
    and as the wide 1x1 kernel followed by a plain 1x1 conv."""
    got, want, kernels = _run(case, {"MVPOSE_NO_PAIRFUSE": "0" if pair else "1"}, monkeypatch)
    cat = case.args[0]
    assert len(kernels) == (1 if cat else 2) + (0 if pair else 1), kernels
    assert "conv1x1_pair_kernel" in kernels and ("conv1x1_kernel" in kernels) == (not pair or not cat), kernels
    _assert_exact(got, want, kernels)


@pytest.mark.parametrize("fused", [True, False])
@_of("bottleneck")
def test_bottlenecks(case, fused, monkeypatch):
    """Layer1's Bottlenecks (four in the small regime, one in the rounding regime), with and
    without the first block's downsample, as whole-Bottleneck launches and as separate convs."""
    got, want, kernels = _run(case, {"MVPOSE_NO_BNECK": "0" if fused else "1"}, monkeypatch)
    assert ("bneck_kernel" in kernels) == fused and ("tconv_kernel" in kernels) == (not fused), kernels
    _assert_exact(got, want, kernels)


@pytest.mark.parametrize("mode,kernels_want", [("tile", ["stem2_tile_kernel"]), ("stream", ["stem2_kernel"]),
                                               ("unfused", ["stem_mfma_kernel", "conv_mfma_kernel"])])
@_of("stem")
def test_stem(case, mode, kernels_want, monkeypatch):
    """The stem's two 3x3/s2 convs: stem2.hip's tile and streaming kernels, and two launches."""
    env = {"tile": {"MVPOSE_STEM2_TILE": "1"}, "stream": STREAM, "unfused": {"MVPOSE_NO_STEMFUSE": "1"}}[mode]
    got, want, kernels = _run(case, env, monkeypatch)
    assert kernels == kernels_want
    _assert_exact(got, want, kernels)


@pytest.mark.parametrize("fused", [True, False])
@_of("transition")
def test_transition1(case, fused, monkeypatch):
    """transition1's 3x3/s1 -> 32 and 3x3/s2 -> 64 from one pass over the 256-ch tensor and apart."""
    got, want, kernels = _run(case, {"MVPOSE_NO_TRANSFUSE": "0" if fused else "1"}, monkeypatch)
    assert kernels == (["trans1_kernel"] if fused else ["tconv_kernel", "conv_mfma_kernel"])
    _assert_exact(got, want, kernels)


# -------------------------------------------------------------- fuse layers --
@_of("fuse")
def test_fuse_layers(case, monkeypatch):
    """All nine workload fuse layers (and two without the ReLU) from the input alone: lead-in,
    1x1 projections, 3x3/s2 chains, nearest upsample by 2^(j-i), sum, ReLU — hrnet.fuse_layer's
    wiring against exact_cases.fuse_layer_ref's, which the CPU tests hold to the oracle's."""
    got, want, kernels = _run(case, {}, monkeypatch)
    assert "fuse_sum_n_kernel" in kernels, kernels
    _assert_exact(got, want, kernels)


@_of("fusesel")
def test_fuse_layers_sum_order(case, monkeypatch):
    """Selection weights, non-integer input: every term is a signed copy of input values
    whatever kernel made it, so the output is bf16(relu(((0 + t0) + t1) + ...)) with f32 adds
    in term order and round-to-nearest-even — the order and the rounding, on ordinary data."""
    got, want, kernels = _run(case, {}, monkeypatch)
    assert "fuse_sum_n_kernel" in kernels, kernels
    _assert_exact(got, want, kernels)


# ------------------------------------------------------------- heatmap head --
HEAD_MODES = {"fused": ({}, "head_fuse_kernel"),
              "NO_HEADFUSE": ({"MVPOSE_NO_HEADFUSE": "1"}, "head1x1_kernel"),
              "NO_HEAD1X1": ({"MVPOSE_NO_HEAD1X1": "1"}, "conv_mfma_kernel")}


# the generic MFMA head sums in another order than the chain: exact integer data only
HEAD_RUNS = [(c, m) for c in ec.CASES if c.kind == "head" for m in HEAD_MODES
             if not (m == "NO_HEAD1X1" and c.regime == "selection")]


@pytest.mark.parametrize("case,mode", HEAD_RUNS, ids=[f"{c.id}-{m}" for c, m in HEAD_RUNS])
def test_head(case, mode, monkeypatch):
    """The head behind fuse layer 0.  Selection fuse weights, ordinary bf16 head weights and an
    f32 bias, non-integer input: head_fuse_kernel, and fuse_sum_n_kernel + head1x1_kernel, must
    give head_chain's f32 fma chain bit for bit.  The generic MFMA head gets exact integer
    data only (as do the other two)."""
    env, family = HEAD_MODES[mode]
    got, want, kernels = _run(case, env, monkeypatch)
    assert kernels[-1] == family and ("fuse_sum_n_kernel" in kernels) == (mode != "fused"), kernels
    _assert_exact(got, want, kernels, nchw=True)
