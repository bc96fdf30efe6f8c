"""RTMDet-m person detector (f1) on the GPU vs the oracle restatement.

Reference: PoseEstimator.predict -> mmdet inference_detector + the hand-off rule
(mmpose_pose_estimation.py:98-99, :234-250).  mmdet / mmcv / cv2 are absent, so parity
is against oracle/rtmdet_ref.py (parity unpinned against the libraries themselves):

* letterbox (cv2 INTER_LINEAR resize, pad 114, normalise) bit-exact;
* every op of the HIP graph, layer by layer, against tests/det_interp.py applied to the
  GPU's own inputs of that op (so each kernel is checked alone, with the device's bf16
  weights): SPP and upsample exact, convs / depthwise / attention / stem within bf16
  output rounding, head logits and boxes to f32 accuracy;
* per-frame selection (best row) exactly the argmax rule on the GPU's candidates;
* NMS exactly the oracle's post-processing on the GPU's candidates;
* end to end vs the fp32 oracle: the selected box agrees wherever the fp32 winner leads
  its runner-up by a margin that bf16 cannot overturn — on the seeded random weights and on
  the peaked (trained-like) head of rtmdet.peaked_state_dict.
"""
import ctypes

import numpy as np
import pytest
import torch

import det_interp
from mvpose import _lib, rtmdet as D
from oracle import rtmdet_ref as R

pytestmark = pytest.mark.gpu
PEAK_BAND = 3.0   # logits below the fp32 selection that count as the frame's peak region
SAT = 16.6355     # f32 sigmoid(x) == 1.0 above this logit (1 - 2^-24 rounds up)
# fixed decidability margin of the peaked end-to-end test: 2 x the median peak-region bf16 logit
# error measured in round 4 (0.865, profiles/r04d_det_peaked.log), committed as a constant
DECIDE_MARGIN = 1.74


def _frames(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


@pytest.fixture(scope="module")
def sd():
    return D.random_state_dict(0)


@pytest.fixture(scope="module")
def det640(sd):
    return D.RTMDetector(sd, max_batch=4)


@pytest.mark.parametrize("shape", [(720, 1280), (1080, 1920), (300, 500), (481, 641), (640, 480)])
def test_letterbox_bit_exact(shape):
    fr = _frames(2, *shape, seed=shape[0])
    out = torch.empty((2, 640, 640, 4), dtype=torch.bfloat16, device="cuda")
    mean = (ctypes.c_float * 3)(*R.MEAN)
    std = (ctypes.c_float * 3)(*R.STD)
    f = torch.from_numpy(fr).cuda()
    _lib.call("mvp_det_letterbox", ctypes.c_void_p(f.data_ptr()), 2, shape[0], shape[1], 640, mean, std,
              ctypes.c_void_p(out.data_ptr()), None)
    torch.cuda.synchronize()
    got = out.cpu()
    for i in range(2):
        img, _, _ = R.letterbox(fr[i], 640)
        ref = R.normalize(img)[0].permute(1, 2, 0).to(torch.bfloat16)
        assert torch.equal(got[i, ..., :3].view(torch.int16), ref.view(torch.int16)), (shape, i)
        assert (got[i, ..., 3] == 0).all()


@pytest.mark.parametrize("size,n", [(128, 2), (640, 1)])
def test_layer_by_layer(sd, size, n, monkeypatch):
    """Each op of the graph on the GPU's own inputs vs the interpreter (every kernel alone,
    at a small size with 2 frames and at the reference's 640).  The producer passes folded into
    their consumer convs are kept as launches here (MVPOSE_DET_FOLD=0: each op alone); the folds
    are test_folds_bitwise's."""
    monkeypatch.setenv("MVPOSE_DET_FOLD", "0")
    det = D.RTMDetector(sd, max_batch=n, size=size)
    spec = det.spec
    frames = torch.from_numpy(_frames(n, size * 9 // 8, 2 * size, seed=5)).cuda()
    worst = {}
    for k, op in enumerate(spec.ops):
        reads = {op.in_.t} | ({op.res.t} if op.kind == D.DET_CONV and op.res.t >= 0 else set())
        if k == 0:
            det.run_ops(frames, 0, 1)  # letterbox + op 0 (the stem does not modify its input)
        before = {t: det.tensor(t, n).float().cpu() for t in reads | {op.out.t} if t >= 0}
        if k > 0:
            det.run_ops(frames, k, k + 1)
        torch.cuda.synchronize()
        T = [before.get(t, torch.zeros((n,) + tuple(spec.tensors[t][:3]))) for t in range(len(spec.tensors))]
        cand = torch.zeros((n, spec.n_priors, 6))
        det_interp.apply_op(spec, T, op, cand, device_weights=True)
        if op.kind == D.DET_HEAD:
            rows = slice(op.aux, op.aux + spec.tensors[op.in_.t][0] * spec.tensors[op.in_.t][1])
            got = det.cand[:n, rows].cpu()
            ref = cand[:, rows]
            assert torch.allclose(got[..., 5], ref[..., 5], rtol=1e-4, atol=1e-4), k
            assert torch.allclose(got[..., 1:5], ref[..., 1:5], rtol=1e-4, atol=1e-3), k
            assert torch.allclose(got[..., 0], ref[..., 0], rtol=1e-4, atol=1e-6), k
            continue
        v = op.out if op.out.t >= 0 else op.in_
        lo, hi = v.coff, v.coff + v.c
        if op.kind == D.DET_SPP:
            hi = spec.tensors[v.t][2]
        got = det.tensor(v.t, n).float().cpu()[..., lo:hi]
        ref = T[v.t][..., lo:hi].to(torch.bfloat16).float()
        if op.kind in (D.DET_SPP, D.DET_UP2):
            assert torch.equal(got, ref), (k, spec.names[k])
            continue
        err = (got - ref).abs()
        scale = ref.abs().max().clamp(min=1.0)
        # output rounding: a bf16 ulp is 2^-8 of the value; accumulation order adds a few
        bad = err > (ref.abs() * 2 ** -6 + 2e-3 * scale)
        worst[spec.names[k]] = float(bad.float().mean())
        assert float(bad.float().mean()) < 1e-3, (k, spec.names[k], float(err.max()))
    det.close()


@pytest.mark.parametrize("size,n", [(128, 3), (640, 2)])
def test_halo_rows_bitwise(sd, size, n, monkeypatch):
    """The 3x3/s1 convs with <= 64 channels on 4-row halo tiles (det_conv_halo_kernel<BN,
    NCK, 4>, the default) against the 2-row tiles (MVPOSE_DET_HALO_ROWS=2): each output's K
    order and epilogue are the same, so every tensor of the forward and the candidates are
    bit-identical."""
    frames = torch.from_numpy(_frames(n, size * 9 // 8, 2 * size, seed=7)).cuda()
    outs = []
    # every tensor is compared: no folds (a folded producer's tensor is never written)
    monkeypatch.setenv("MVPOSE_DET_FOLD", "0")
    for rows in ("2", "4"):
        monkeypatch.setenv("MVPOSE_DET_HALO_ROWS", rows)
        det = D.RTMDetector(sd, max_batch=n, size=size)
        det.run_ops(frames, 0, len(det.spec.ops))
        torch.cuda.synchronize()
        ts = [det.tensor(t, n).cpu() for t in range(len(det.spec.tensors))]
        outs.append((ts, det.cand[:n].cpu()))
        det.close()
    (ta, ca), (tb, cb) = outs
    for t, (x, y) in enumerate(zip(ta, tb)):
        assert torch.equal(x.view(torch.int16), y.view(torch.int16)), (size, t)
    assert torch.equal(ca.view(torch.int32), cb.view(torch.int32))


@pytest.mark.parametrize("size,n", [(128, 3), (640, 2)])
def test_dwpw_fused_bitwise(sd, size, n, monkeypatch):
    """The CSPNeXt stage-1/2 blocks' conv2 as ONE launch (DET_DWPW: 5x5 depthwise + 1x1 pointwise,
    the depthwise output kept in LDS; det_dw.hip dwpw_kernel) against the unfused pair (dw5_kernel +
    the 1x1 GEMM, MVPOSE_DET_DWPW=0): the same fma chains, bf16 rounding of the intermediate, MFMA
    operands and K order, so the candidates of every prior and the selected boxes are
    bit-identical (at 128 the 4x4 .. 32x32 planes exercise the partial tiles)."""
    frames = torch.from_numpy(_frames(n, size * 9 // 8, 2 * size, seed=9)).cuda()
    out = {}
    for fuse in ("0", "1"):
        monkeypatch.setenv("MVPOSE_DET_DWPW", fuse)
        det = D.RTMDetector(sd, max_batch=n, size=size)
        kinds = [op.kind for op in det.spec.ops]
        assert (D.DET_DWPW in kinds) == (fuse == "1")
        r = det.detect(frames)
        torch.cuda.synchronize()
        out[fuse] = (r["cand"].cpu(), r["best"].cpu())
        det.close()
    assert torch.equal(out["0"][0].view(torch.int32), out["1"][0].view(torch.int32))
    assert torch.equal(out["0"][1].view(torch.int32), out["1"][1].view(torch.int32))


@pytest.mark.parametrize("size,n", [(128, 3), (640, 2)])
def test_live_couts_bitwise(sd, size, n, monkeypatch):
    """The 48-of-64-cout 3x3 convs (stem.2, stage-1 conv1: DetOp.aux = 48 live couts) on the
    halo kernel's live-tile form (det_conv_halo_kernel<64, *, 4, 3>: one output row per wave,
    the zero tile stored, not multiplied) against the full 64-cout form (MVPOSE_DET_LIVE=0):
    every tensor of the forward, padding channels included, is bit-identical."""
    frames = torch.from_numpy(_frames(n, size * 9 // 8, 2 * size, seed=21)).cuda()
    outs = []
    # every tensor is compared: no folds (a folded producer's tensor is never written)
    monkeypatch.setenv("MVPOSE_DET_FOLD", "0")
    for live in ("0", "1"):
        monkeypatch.setenv("MVPOSE_DET_LIVE", live)
        det = D.RTMDetector(sd, max_batch=n, size=size)
        live_ops = [k for k, op in enumerate(det.spec.ops) if op.kind == D.DET_CONV and 32 < op.aux < op.out.c]
        assert len(live_ops) >= 2, live_ops
        det.run_ops(frames, 0, len(det.spec.ops))
        torch.cuda.synchronize()
        ts = [det.tensor(t, n).cpu() for t in range(len(det.spec.tensors))]
        outs.append((ts, det.cand[:n].cpu()))
        det.close()
    (ta, ca), (tb, cb) = outs
    for t, (x, y) in enumerate(zip(ta, tb)):
        assert torch.equal(x.view(torch.int16), y.view(torch.int16)), (size, t)
    assert torch.equal(ca.view(torch.int32), cb.view(torch.int32))


@pytest.mark.parametrize("size,n,pers", [(128, 3, "1"), (640, 2, "1"), (128, 3, "3"), (640, 2, "3")])
def test_persistent_1x1_bitwise(sd, size, n, pers, monkeypatch):
    """The 1x1 and the GEMM-path 3x3 (s1 and s2) convs on the persistent GEMM
    (det_conv1x1_pers_kernel: 2 workgroups per CU walk (tile, cout block) items, weight
    fragments loaded into VGPRs, the pixel ring running across items; the default) against one
    tile per workgroup (det_conv_gemm_kernel, MVPOSE_DET_PERS=0): the same operands and MFMA
    sequence per output (K steps in (tap row, tap column, chunk) order), so every tensor of the
    forward is bit-identical (the 128 size: ragged last tiles, zero-padded taps at the borders,
    workgroups with no item)."""
    frames = torch.from_numpy(_frames(n, size * 9 // 8, 2 * size, seed=23)).cuda()
    outs = []
    monkeypatch.setenv("MVPOSE_DET_FOLD", "0")  # mode 0 has no folds (they need the persistent GEMM)
    for mode in ("0", pers):  # pers "1": the 1x1 convs (the default); "3": the 3x3 GEMM convs too
        monkeypatch.setenv("MVPOSE_DET_PERS", mode)
        det = D.RTMDetector(sd, max_batch=n, size=size)
        det.run_ops(frames, 0, len(det.spec.ops))
        torch.cuda.synchronize()
        ts = [det.tensor(t, n).cpu() for t in range(len(det.spec.tensors))]
        outs.append((ts, det.cand[:n].cpu()))
        det.close()
    (ta, ca), (tb, cb) = outs
    for t, (x, y) in enumerate(zip(ta, tb)):
        assert torch.equal(x.view(torch.int16), y.view(torch.int16)), (size, t)
    assert torch.equal(ca.view(torch.int32), cb.view(torch.int32))


@pytest.mark.parametrize("size,n,shape", [(160, 3, (180, 320)), (640, 2, (720, 1280)), (160, 2, (301, 499))])
def test_folds_bitwise(sd, size, n, shape, monkeypatch):
    """The neck's nearest-2x upsamples and the CSP layers' channel-attention scale pass folded into
    their consumer 1x1 convs (det_conv1x1_pers_kernel FM 1 / 2: the pixel DMA reads the
    half-resolution source; the scales are applied to the landed pixels in LDS with
    ca_scale_kernel's f32 product and bf16 rounding) against the unfolded launches
    (MVPOSE_DET_FOLD=0): the output of every op, run from the start up to it, and the candidates
    are bit-identical.  And the folds happened: the upsample slices stay unwritten and the
    attention tensors unscaled (160: 5x5 stride-32 planes, a 128-pixel tile over 7 frames).  The
    letterbox is folded into the stem too (det_stem_kernel<true> stages its input rows from the
    raw frames): 2x frames take the INTER_AREA fast path, 301 x 499 the bilinear one."""
    frames = torch.from_numpy(_frames(n, *shape, seed=31)).cuda()
    dets = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("MVPOSE_DET_FOLD", mode)
        dets[mode] = D.RTMDetector(sd, max_batch=n, size=size)
    spec = dets["0"].spec
    ops = spec.ops
    up_ops = [k for k, op in enumerate(ops) if op.kind == D.DET_UP2]
    ca_ops = [k for k, op in enumerate(ops) if op.kind == D.DET_CA]
    assert len(up_ops) == 2 and len(ca_ops) == 4, (up_ops, ca_ops)
    f0, f1 = dets["0"].folded_ops(), dets["1"].folded_ops()
    assert not any(f0) and [k for k, f in enumerate(f1) if f] == sorted([0] + up_ops + ca_ops), f1
    assert f1[0] == 2 and ops[0].kind == D.DET_STEM  # the letterbox inside the stem

    def view(det, v):
        return det.tensor(v.t, n)[..., v.coff:v.coff + v.c].cpu()

    def upto(det, k, v):
        det.run_ops(frames, 0, k)
        torch.cuda.synchronize()
        return view(det, v)

    for k in ca_ops:  # folded: the op leaves its tensor unscaled; unfolded: it scales it
        v = ops[k].in_
        b0, a0 = upto(dets["0"], k, v), upto(dets["0"], k + 1, v)
        b1, a1 = upto(dets["1"], k, v), upto(dets["1"], k + 1, v)
        assert torch.equal(b0.view(torch.int16), b1.view(torch.int16)), k
        assert torch.equal(a1.view(torch.int16), b1.view(torch.int16)), (k, "scale pass ran")
        assert not torch.equal(a0.view(torch.int16), b0.view(torch.int16)), k
    for k in up_ops:  # folded: the upsample slice is never written
        a0, a1 = upto(dets["0"], k + 1, ops[k].out), upto(dets["1"], k + 1, ops[k].out)
        assert not torch.equal(a0.view(torch.int16), a1.view(torch.int16)), (k, "upsample ran")
    for k, op in enumerate(ops):
        if op.kind in (D.DET_UP2, D.DET_CA, D.DET_HEAD, D.DET_SPP) or f1[k] == 1:
            continue  # no output of their own (or, folded, never written)
        a0, a1 = upto(dets["0"], k + 1, op.out), upto(dets["1"], k + 1, op.out)
        assert torch.equal(a0.view(torch.int16), a1.view(torch.int16)), (size, k, spec.names[k])
    r0, r1 = dets["0"].detect(frames), dets["1"].detect(frames)
    torch.cuda.synchronize()
    c0, b0 = r0["cand"].cpu(), r0["best"].cpu()
    assert torch.equal(c0.view(torch.int32), r1["cand"].cpu().view(torch.int32))
    assert torch.equal(b0.view(torch.int32), r1["best"].cpu().view(torch.int32))
    # asked for the letterboxed image, the folded graph letterboxes apart (the stem reads it back)
    dets["0"].run_ops(frames, 0, 1)  # the unfolded letterbox (+ the stem, which does not write its input)
    torch.cuda.synchronize()
    img0 = dets["0"].tensor(ops[0].in_.t, n).cpu()
    lb = torch.empty((n, size, size, 4), dtype=torch.bfloat16, device="cuda")
    r1b = dets["1"].detect(frames, letterboxed=lb)
    torch.cuda.synchronize()
    assert torch.equal(lb.cpu().view(torch.int16), img0.view(torch.int16))
    assert torch.equal(c0.view(torch.int32), r1b["cand"].cpu().view(torch.int32))
    for d in dets.values():
        d.close()


@pytest.mark.parametrize("size,n", [(128, 3), (640, 2)])
def test_halo_persistent_bitwise(sd, size, n, monkeypatch):
    """The 64-cout 3x3/s1 convs with one or two input chunks (stem.2, the stage-1 block conv1s)
    on the persistent halo kernel (det_conv_halo_pers_kernel: weights resident in LDS, 8-row
    tiles, the next step's halo DMA under the current one; the default) against the tile
    kernel (det_conv_halo_kernel, MVPOSE_DET_HALO_PERS=0): same operands and K order, so every
    tensor of the forward is bit-identical (128: planes narrower than a 64-column tile)."""
    frames = torch.from_numpy(_frames(n, size * 9 // 8, 2 * size, seed=29)).cuda()
    outs = []
    # every tensor is compared: no folds (a folded producer's tensor is never written)
    monkeypatch.setenv("MVPOSE_DET_FOLD", "0")
    for mode in ("0", "1"):
        monkeypatch.setenv("MVPOSE_DET_HALO_PERS", mode)
        det = D.RTMDetector(sd, max_batch=n, size=size)
        det.run_ops(frames, 0, len(det.spec.ops))
        torch.cuda.synchronize()
        ts = [det.tensor(t, n).cpu() for t in range(len(det.spec.tensors))]
        outs.append((ts, det.cand[:n].cpu()))
        det.close()
    (ta, ca), (tb, cb) = outs
    for t, (x, y) in enumerate(zip(ta, tb)):
        assert torch.equal(x.view(torch.int16), y.view(torch.int16)), (size, t)
    assert torch.equal(ca.view(torch.int32), cb.view(torch.int32))


def test_band_conv_vs_gemm(sd, monkeypatch):
    """The 3x3/s1 convs with >= 96 input channels on the 80x80 / 40x40 planes run on the
    band-halo kernel (det_conv_band_kernel, the default): each one, on the forward's own input,
    against the im2col GEMM kernel (MVPOSE_DET_BAND=0).  K order (chunk, tap, channel) vs (tap,
    chunk, channel): equal to f32 rounding, so the bf16 outputs agree to within a bf16 ulp where
    the f32 sums straddle a rounding boundary (3 frames: the bands' XCD groups are uneven).  A
    detector chooses its kernels when it is created, so there is one per MVPOSE_DET_BAND setting;
    the other two run each conv alone on a copy of the default detector's input (and residual)."""
    n = 3
    monkeypatch.setenv("MVPOSE_DET_FOLD", "1")
    dets = {}
    for band in ("0", "1", "4"):  # the GEMM kernel, the band kernel (8 waves), its 4-wave form
        monkeypatch.setenv("MVPOSE_DET_BAND", band)
        dets[band] = D.RTMDetector(sd, max_batch=n, size=640)
    monkeypatch.delenv("MVPOSE_DET_BAND")
    det = dets["1"]
    spec = det.spec
    frames = torch.from_numpy(_frames(n, 720, 1280, seed=9)).cuda()
    det.run_ops(frames, 0, len(spec.ops))
    torch.cuda.synchronize()
    eligible = [k for k, op in enumerate(spec.ops)
                if op.kind == D.DET_CONV and op.ks == 3 and op.stride == 1 and op.in_.c >= 96 and op.in_.c % 32 == 0
                and spec.tensors[op.in_.t][0] in (80, 40)]
    assert len(eligible) >= 21, eligible
    for k in eligible:
        op = spec.ops[k]
        lo, hi = op.out.coff, op.out.coff + op.out.c
        outs = {}
        for band, d in dets.items():
            if d is not det:
                for t in {op.in_.t, op.res.t} - {-1}:
                    d.set_tensor(t, det.tensor(t, n))
            d.run_ops(frames, k, k + 1)
            torch.cuda.synchronize()
            outs[band] = d.tensor(op.out.t, n).float().cpu()[..., lo:hi]
        # each output's MFMA sequence is the same in both band forms: bit-identical
        assert torch.equal(outs["1"], outs["4"]), spec.names[k]
        a, b = outs["1"], outs["0"]
        finite = bool(torch.isfinite(a).all())
        diff = (a - b).abs()
        scale = float(b.abs().max().clamp(min=1.0))
        # a bf16 ulp of the value, or of the f32 sum's cancellation (terms ~ scale) near zero
        n_bad = int((diff > b.abs() * 2 ** -7 + 2 ** -9 * scale).sum())
        frac_diff = float((diff > 0).float().mean())
        assert finite and n_bad == 0 and frac_diff < 0.05, (spec.names[k], n_bad, float(diff.max()), frac_diff)
    for d in dets.values():
        d.close()


@pytest.mark.parametrize("size,n", [(128, 3), (640, 2)])
def test_head_staged_bitwise(sd, size, n, monkeypatch):
    """The head predictions with the [cls | reg] features staged through LDS
    (det_head_staged_kernel, the default) against one lane per pixel reading HBM directly
    (MVPOSE_DET_HEAD_DIRECT=1): same fmaf chains in the same k order, bit-identical
    candidates."""
    frames = torch.from_numpy(_frames(n, size * 9 // 8, 2 * size, seed=8)).cuda()
    cands = []
    for direct in ("1", "0"):
        monkeypatch.setenv("MVPOSE_DET_HEAD_DIRECT", direct)
        det = D.RTMDetector(sd, max_batch=n, size=size)
        det.run_ops(frames, 0, len(det.spec.ops))
        torch.cuda.synchronize()
        cands.append(det.cand[:n].cpu())
        det.close()
    assert torch.isfinite(cands[1]).all()
    assert torch.equal(cands[0].view(torch.int32), cands[1].view(torch.int32))


def test_select_is_argmax_of_candidates(det640):
    fr = torch.from_numpy(_frames(3, 720, 1280, seed=11)).cuda()
    out = det640.detect(fr)
    torch.cuda.synchronize()
    cand = out["cand"].cpu()
    best = out["best"].cpu()
    fx, fy = det640.scale_factors(720, 1280)
    f32 = np.float32
    for i in range(3):
        c = cand[i].numpy()
        x1, y1, x2, y2 = c[:, 1] * f32(fx), c[:, 2] * f32(fy), c[:, 3] * f32(fx), c[:, 4] * f32(fy)
        ok = (c[:, 0] > f32(0.05)) & (x2 - x1 > 0) & (y2 - y1 > 0)
        j = int(np.flatnonzero(ok)[np.argmax(c[ok, 0])])  # first maximum = lowest prior index
        assert int(best[i, 5]) == j
        assert np.array_equal(best[i, :4].numpy(), np.array([x1[j], y1[j], x2[j], y2[j]], np.float32))
        assert float(best[i, 4]) == float(c[j, 0])


def test_select_none_below_score_thr(det640):
    fr = torch.from_numpy(_frames(2, 720, 1280, seed=12)).cuda()
    det640.cfg["score_thr"] = 2.0  # no sigmoid score passes
    try:
        out = det640.detect(fr)
        torch.cuda.synchronize()
        assert (out["best"][:, 4] == -1).all()
        assert np.isnan(D.RTMDetector.bboxes_for(out["best"])).all()
        assert all(len(d) == 0 for d in det640.nms(out))  # NMS over no survivors: empty lists
    finally:
        det640.cfg["score_thr"] = D.TEST_CFG["score_thr"]


def test_nms_matches_oracle_postprocess(det640):
    fr = torch.from_numpy(_frames(3, 720, 1280, seed=13)).cuda()
    out = det640.detect(fr)
    dets = det640.nms(out)
    cand = out["cand"].cpu()
    sf = (640 / 1280, 360 / 720)
    for i in range(3):
        b, s, _ = R.postprocess_candidates(cand[i, :, 0], cand[i, :, 1:5], det640.spec.level_off, sf)
        assert dets[i].shape[0] == len(s), (i, dets[i].shape, len(s))
        assert np.array_equal(dets[i][:, :4], b.numpy()), i
        assert np.array_equal(dets[i][:, 4], s.numpy()), i
        # the reference's selection = the GPU's per-frame best row
        sel = R.select_bbox(b, s, torch.zeros(len(s), dtype=torch.long))
        best = out["best"][i].cpu().numpy()
        if sel is not None:
            assert np.array_equal(sel, best[:4])


def test_end_to_end_vs_fp32_oracle(sd, det640):
    """bf16 GPU detector vs the fp32 restatement on the same frames.

    These seeded random weights amplify perturbations strongly (rounding only the input to
    bf16 moves single logits by up to ~1, tools/det_e2e_diag.py), so single logits differ by
    up to a few units while the bulk agrees: per frame the median |d logit| is small, the
    GPU's selected prior is near-optimal under fp32 (its fp32 logit within 4 of the fp32
    maximum), and where the fp32 winner leads by > 2.5 the GPU selects the same prior."""
    m = R.build_model(sd)
    n = 16
    frames = _frames(n, 720, 1280, seed=21)
    cands, bests = [], []
    for i0 in range(0, n, 4):
        out = det640.detect(torch.from_numpy(frames[i0:i0 + 4]).cuda())
        cands.append(out["cand"].cpu().clone())
        bests.append(out["best"].cpu().clone())
    cand, best = torch.cat(cands), torch.cat(bests).numpy()
    decided = agree = same = 0
    for i in range(n):
        with torch.no_grad():
            cs, _ = m(R.normalize(R.letterbox(frames[i], 640)[0]))
        lg = torch.cat([c[0, 0].reshape(-1) for c in cs])
        d = (cand[i, :, 5] - lg).abs()
        assert float(torch.median(d)) < 0.15 and float(d.mean()) < 0.4, (i, float(d.median()), float(d.mean()))
        gi = int(best[i, 5])
        t2 = torch.topk(lg, 2)
        assert float(lg[gi]) >= float(t2.values[0]) - 4.0, (i, float(lg[gi]), float(t2.values[0]))
        same += int(gi == int(t2.indices[0]))
        if float(t2.values[0] - t2.values[1]) > 2.5:
            decided += 1
            agree += int(gi == int(t2.indices[0]))
    print(f"same prior {same}/{n}, decided {decided}, agree {agree}")
    assert agree == decided


def test_end_to_end_peaked_vs_fp32_oracle():
    """The selected prior on a trained-like detector: rtmdet.peaked_state_dict (classification
    head fitted to one clear best prior per person, tools/train_peaked_rtmdet.py) on 64 skeleton
    frames the fit never saw.  The fp32 side selects as the reference does: the highest f32
    score among the priors that survive post-processing (score > score_thr, a box of positive
    size), the lowest index on ties.  A frame is decidable when every other valid prior is below
    the selection by more than the FIXED margin DECIDE_MARGIN (2 x round 4's measured median
    peak-region bf16 logit error, independent of the output under test), or a robustly
    saturated (score 1.0) tie with a later index.  There the GPU must select the same prior
    (>= 95 % of those frames), >= 40 frames must be decidable, and the bf16 path's peak-region
    logit error itself is bounded (its median within the margin)."""
    from mvpose import synthetic as syn
    sd = D.peaked_state_dict()
    m = R.build_model(sd)
    det = D.RTMDetector(sd, max_batch=8)
    n = 64
    frames, _ = syn.make_skeleton_frames(n, seed=77)
    cands, bests = [], []
    for i0 in range(0, n, 8):
        out = det.detect(torch.from_numpy(frames[i0:i0 + 8]).cuda())
        cands.append(out["cand"].cpu().clone())
        bests.append(out["best"].cpu().clone())
    det.close()
    cand, best = torch.cat(cands), torch.cat(bests).numpy()
    leads, agree, dmed, errs, decs = [], [], [], [], []
    for i in range(n):
        img, sf, _ = R.letterbox(frames[i], 640)
        with torch.no_grad():
            cs, bp = m(R.normalize(img))
        lg = torch.cat([c[0, 0].reshape(-1) for c in cs])
        dmed.append(float(torch.median((cand[i, :, 5] - lg).abs())))
        # the reference's selection is the first detection after post-processing: the best
        # prior among those with score > score_thr and a box of positive size (min_bbox_size 0)
        sc, bx = R.candidates(cs, bp)
        bx = bx * torch.tensor([1 / sf[0], 1 / sf[1]] * 2)
        ok = (sc > R.TEST_CFG["score_thr"]) & (bx[:, 2] - bx[:, 0] > 0) & (bx[:, 3] - bx[:, 1] > 0)
        # fp32 selection: the highest SCORE (sigmoid, f32) among valid priors, the lowest prior
        # index on ties (the stable sort) — f32 sigmoids of logits above ~16.64 are exactly 1.0,
        # so saturated peaks tie and the index decides, in mmdet and on the GPU alike
        scv = sc.masked_fill(~ok, -1.0)
        sel = int(torch.nonzero(scv == scv.max())[0])
        # the bf16 path's logit error where it matters, reported and bounded below: over the
        # frame's peak region (priors within PEAK_BAND of the selected logit), the largest
        # |GPU - fp32| logit difference
        near = lg >= lg[sel] - PEAK_BAND
        e = float((cand[i, :, 5] - lg).abs()[near].max())
        errs.append(e)
        # decidable by the fp32 logits alone: every other valid prior is clearly below the
        # selection (by the fixed margin), or a robust saturated tie the index decides (both
        # above SAT + margin, the other later)
        idx = torch.arange(len(lg))
        other = ok & (idx != sel)
        below = lg[sel] - lg > DECIDE_MARGIN
        tie = (lg > SAT + DECIDE_MARGIN) & (lg[sel] > SAT + DECIDE_MARGIN) & (idx > sel)
        lead = float((lg[sel] - lg[other & ~tie]).min()) if bool((other & ~tie).any()) else float("inf")
        leads.append(lead)
        decs.append(bool((below | tie | ~other).all()))
        agree.append(int(best[i, 5]) == sel)
        if not agree[-1]:
            gi = int(best[i, 5])
            print(f"frame {i}: GPU prior {gi} (fp32 {float(lg[gi]):.3f}, GPU {float(cand[i, gi, 5]):.3f}), fp32 "
                  f"selection {sel} (fp32 {float(lg[sel]):.3f}, GPU {float(cand[i, sel, 5]):.3f}), lead {lead:.3f}, "
                  f"peak-region error {e:.3f}, decidable {decs[-1]}")
    leads, agree, errs, dec = np.array(leads), np.array(agree), np.array(errs), np.array(decs)
    print(f"peaked detector: median |d logit| per frame {np.median(dmed):.3f} (max {max(dmed):.3f}); peak-region "
          f"|d logit| median {np.median(errs):.3f} (max {errs.max():.3f}); fp32 top-1 lead median "
          f"{np.median(leads):.2f}; decidable {dec.sum()}/{n}, agreement there "
          f"{agree[dec].mean():.3f}; agreement overall {agree.mean():.3f}")
    assert dec.sum() >= 40
    assert agree[dec].mean() >= 0.95
    assert np.median(errs) <= DECIDE_MARGIN


def test_pose_estimator_with_detector(det640):
    """PoseEstimator(using_detector) crops each frame to the detector's person box: batched
    (device argmax) and per-frame (NMS list + the reference's hand-off rule) agree, and
    equal BatchPoseEstimator.run with those boxes."""
    from mvpose import hrnet, synthetic as syn
    from mvpose.mmpose_pose_estimation import PoseEstimator
    from mvpose.pipeline import MultiViewPipeline
    sd_pose = hrnet.random_state_dict(5)
    pe = PoseEstimator(None, None, None, None, detector=det640, state_dict=sd_pose, max_frames=4)
    frames = _frames(4, 720, 1280, seed=31)
    out = pe.predict_batch(frames)
    boxes = D.RTMDetector.bboxes_for(det640.detect(torch.from_numpy(frames).cuda())["best"])
    assert np.isfinite(boxes).any()
    ref = pe.estimator((720, 1280)).run(torch.from_numpy(frames).cuda(), bboxes=boxes)
    assert torch.equal(out["keypoints"], ref["keypoints"])
    # per-frame: the NMS list through the reference's selection = the batched box
    for i in range(2):
        dets = det640(frames[i])
        from mvpose.mmpose_pose_estimation import select_person_bbox
        b = select_person_bbox(dets)
        if b is None:
            assert np.isnan(boxes[i]).all()
        else:
            np.testing.assert_array_equal(b, boxes[i].astype(np.float32))
    # the multi-view pipeline with the detector in front
    cams = syn.make_rig(2, seed=3)
    p = MultiViewPipeline(syn.reference_camera_params(cams), estimator=pe.estimator((720, 1280)), detector=det640)
    fr = torch.from_numpy(frames).cuda().reshape(2, 2, 720, 1280, 3)
    a = p.process(fr)
    k2a = a["kpts_2d"].clone()
    b = p.process(fr, bboxes=boxes.reshape(2, 2, 4))
    assert torch.equal(k2a, b["kpts_2d"])
