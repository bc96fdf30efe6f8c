"""Every person-detector kernel, bit for bit, on exactly summable data.

tests/det_exact_cases.py builds, per case, a detector of ONE op (behind a filler op, in front of a
small head level: what detnet.cpp's validation wants) with weights and inputs whose f32 partial
sums are exact in any order (tests/test_det_exact_cases.py proves each case's precondition on the
CPU), so the op's bf16 result is one fixed array whatever the K order, tile shape, ring depth or
fold.  Each test here creates that detector under the case's MVPOSE_DET_* switches, asserts through
launch_kernels() (and folded_ops() for the folds) that the variant the case names is the one that
runs, fills the whole output tensor with a NaN sentinel, runs the op and compares bit patterns with
the float64 reference: no tolerance under ACT_NONE and ACT_RELU; under ACT_SILU the expected bits
everywhere but at the undecidable elements (at most 2 % of a case), which may be either bf16
neighbour.  Inside the output view every stored channel is written (padding couts +0); outside it
the sentinel survives.  A dropped tap on one tile corner, a halo column from the neighbouring
frame, a ragged last tile never stored, a K chunk skipped on one cout block, a ReLU in front of the
residual: each changes bits.

variant (det_select.h)   test[cases]
gemm                     test_gemm[gemm-*]: MVPOSE_DET_PERS=0; 1x1 at every cout tile (32 .. 192, 96 -> 384), 3x3/s1,
                         3x3/s2 (odd planes), a residual on both forms, views at coff > 0 on both sides
pers_gemm                test_gemm[pers_gemm-*]: the same shapes (3x3: MVPOSE_DET_PERS=3); 75 pixels = fewer items
                         than workgroups; 96 -> 768 on 40x40 x 7 with MVPOSE_DET_PERS_OCC=1 = 352 items on 256 workgroups
fold_up, fold_ca         test_fold: [up(x) | y] with the upsample's slice left as sentinel; attention + 1x1 on 5x5 x 7
                         frames (a tile over 6 frames) and 20x20, the input tensor left unscaled
halo, halo_2row,         test_halo: 5x5, 9x70 (two column tiles, ragged both ways), 20x20; one and two chunks; with
halo_live3               a residual; 48 live couts of 64
halo_pers_lt2 / 3 / 4    test_halo_pers: 24 / 48 / 64 live couts; 160x160 x 5 frames = 300 tiles x 2 chunks on 256 workgroups
band_8w, band_4w         test_band: 96 -> 64, 96 -> 96, 192 -> 192 on 40x40, 96 -> 64 / 96 on 80x80, 3 frames, residuals
stem                     test_stem: sizes 64 and 96
dw5                      test_dw5: C = 32 .. 192 on 3x3, 5x5, 20x20, 25 distinct taps
dwpw                     test_dwpw: C = 64 (48 live couts) and 96 on 4x4 .. 33x33, with and without the identity
ca_pool, ca_fc, ca_scale test_ca: C = 64, 192, 768 on 4x4, 8x8 and 5x5, 2 and 9 frames, against the f32 restatement
spp, up2                 test_spp, test_up2
head_staged, head_direct test_head: F = 192 on 5x5 (stride 32) and 20x20 (stride 8); the logit bit for bit
"""
import numpy as np
import pytest
import torch

import det_exact_cases as dc

pytestmark = pytest.mark.gpu


def _of(family):
    out = [c for c in dc.CASES if c.family == family]
    return pytest.mark.parametrize("case", out, ids=[c.id for c in out])


def _kernels_of(spec, kernels, folded, k):
    """The launch records of op k among mvp_det_kernels' (detnet.cpp): the letterbox unless it is
    folded into the stem, every op but a folded upsample, an attention as pool, fc and, unless
    folded, scale."""
    from mvpose import rtmdet as D
    i = 0 if folded[0] == 2 else 1
    for j, op in enumerate(spec.ops):
        if op.kind == D.DET_UP2 and folded[j]:
            assert j != k
            continue
        n = 1 if op.kind != D.DET_CA else 2 if folded[j] else 3
        if j == k:
            return kernels[i:i + n]
        i += n
    raise AssertionError(k)


def _run(case, monkeypatch):
    """Create the case's detector under its switches, run its op on its inputs, and return (the
    output tensor's or the candidates' bit patterns, the detector's tensors after the run by id
    for the inputs, the kernels of the op, all kernels)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mvpose import rtmdet as D
    for k in dc.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    B = dc.build(case)
    n = case.n
    det = D.RTMDetector(spec=B.spec, max_batch=n)
    try:
        kernels, folded = det.launch_kernels(), det.folded_ops()
        mine = _kernels_of(B.spec, kernels, folded, B.op_index)
        assert mine[0] == case.variant == dc.expected_variant(case), (mine, case.variant, kernels)
        if case.op == "ca":
            assert mine == ["ca_pool", "ca_fc", "ca_scale"], mine
        if case.fold == "up":
            assert folded[B.op_index - 1] == 1 and "up2" not in kernels[2:-2], (folded, kernels)
        if case.fold == "ca":
            assert folded[B.begin] == 1 and _kernels_of(B.spec, kernels, folded, B.begin) == ["ca_pool", "ca_fc"], kernels
        for t, x in B.inputs.items():
            det.set_tensor(t, x.cuda())
        if case.op == "head":
            det.cand.view(torch.int32).fill_(dc.SENT32)
        frames = torch.zeros((n, 32, 32, 3), dtype=torch.uint8, device="cuda")
        det.run_ops(frames, B.begin, B.end)
        torch.cuda.synchronize()
        after = {t: det.tensor(t, n).cpu().view(torch.int16).numpy() for t in B.inputs}
        got = det.cand[:n].cpu().view(torch.int32).numpy() if case.op == "head" else after[B.out_t]
    finally:
        det.close()
    return got, after, mine, kernels


def _assert_exact(case, got, e, kernels):
    """Bit patterns equal (or, at an undecidable SiLU element, between the two neighbours); on
    failure the count, the first ten (n, h, w, c) with got / want, and the kernels."""
    assert got.shape == e.want.shape
    bad = dc.mismatches(got, e)
    if e.und is not None:
        print(f"{case.id}: {int(e.und.sum())} of {e.stats['numel']} elements undecidable")
    if not bad.any():
        return
    lines = []
    for idx in np.argwhere(bad)[:10]:
        idx = tuple(int(i) for i in idx)
        g, w = dc.bits_f64(got[idx].reshape(1))[0], dc.bits_f64(e.want[idx].reshape(1))[0]
        lines.append(f"  (n, h, w, c) = {idx}: got {g!r} ({int(got[idx]) & 0xFFFF:#06x}), want {w!r} "
                     f"({int(e.want[idx]) & 0xFFFF:#06x})" + (" undecidable" if e.und is not None and e.und[idx] else ""))
    pytest.fail(f"{case.id}: {int(bad.sum())} of {bad.size} elements differ; first:\n" + "\n".join(lines) +
                f"\nkernels: {kernels}", pytrace=False)


def _check(case, monkeypatch):
    got, after, mine, kernels = _run(case, monkeypatch)
    _assert_exact(case, got, dc.reference(case), mine)
    return after


@_of("gemm")
def test_gemm(case, monkeypatch):
    """det_conv_gemm_kernel and det_conv1x1_pers_kernel: 3 frames, so the flat 128-pixel tiles span
    frames and a tap that leaves one frame would land in the next."""
    _check(case, monkeypatch)


@_of("fold")
def test_fold(case, monkeypatch):
    """The persistent GEMM's folds.  fold_up: the upsample is not launched and its slice of the
    conv's input still holds the sentinel afterwards.  fold_ca: the scale pass is not launched and
    the conv's input tensor is left unscaled."""
    B = dc.build(case)
    after = _check(case, monkeypatch)
    x_t = B.op.in_.t
    assert np.array_equal(after[x_t], B.inputs[x_t].view(torch.int16).numpy()), "the fold wrote the conv's input"


@_of("halo")
def test_halo(case, monkeypatch):
    """det_conv_halo_kernel: 4-row tiles, 2-row tiles, and the 3-live-tile form."""
    _check(case, monkeypatch)


@_of("halo_pers")
def test_halo_pers(case, monkeypatch):
    """det_conv_halo_pers_kernel with 2, 3 and 4 live 16-cout tiles."""
    _check(case, monkeypatch)


@_of("band")
def test_band(case, monkeypatch):
    """det_conv_band_kernel, 8 and 4 waves."""
    _check(case, monkeypatch)


@_of("stem")
def test_stem(case, monkeypatch):
    """det_stem_kernel<false> on a given input (the letterbox fold is test_folds_bitwise's)."""
    _check(case, monkeypatch)


@_of("dw5")
def test_dw5(case, monkeypatch):
    _check(case, monkeypatch)


@_of("dwpw")
def test_dwpw(case, monkeypatch):
    """dwpw_kernel: the intermediate is rounded to bf16 as the unfused pair stores it."""
    _check(case, monkeypatch)


@_of("ca")
def test_ca(case, monkeypatch):
    """ca_pool_kernel, ca_fc_kernel and ca_scale_kernel against their arithmetic in numpy float32."""
    _check(case, monkeypatch)


@_of("spp")
def test_spp(case, monkeypatch):
    """Slices 1 .. 3 are the 5, 9 and 13 max pools of slice 0 (max is exact), slice 0 is unchanged."""
    _check(case, monkeypatch)


@_of("up2")
def test_up2(case, monkeypatch):
    B = dc.build(case)
    after = _check(case, monkeypatch)
    assert np.array_equal(after[B.op.in_.t], B.inputs[B.op.in_.t].view(torch.int16).numpy())


@_of("head")
def test_head(case, monkeypatch):
    """The logit (column 5) bit for bit and the other levels' rows untouched; score and box, which
    go through expf, to test_layer_by_layer's tolerances against float64."""
    got, _, mine, kernels = _run(case, monkeypatch)
    e = dc.reference(case)
    rows = e.rows
    other = np.ones(got.shape[1], bool)
    other[rows] = False
    assert np.all(got[:, other] == dc.SENT32), "rows of another level were written"
    bad = got[:, rows, 5] != e.want[:, rows, 5]
    if bad.any():
        lines = [f"  (n, prior) = {tuple(i)}: got {got[:, rows, 5][tuple(i)].view(np.float32)!r}, want "
                 f"{e.want[:, rows, 5][tuple(i)].view(np.float32)!r}" for i in np.argwhere(bad)[:10]]
        pytest.fail(f"{case.id}: {int(bad.sum())} of {bad.size} logits differ; first:\n" + "\n".join(lines) +
                    f"\nkernels: {mine}", pytrace=False)
    val = torch.from_numpy(np.ascontiguousarray(got[:, rows]).view(np.float32)).double()
    assert torch.allclose(val[..., 1:5], torch.from_numpy(e.box), rtol=1e-4, atol=1e-3)
    assert torch.allclose(val[..., 0], torch.from_numpy(e.score), rtol=1e-4, atol=1e-6)
