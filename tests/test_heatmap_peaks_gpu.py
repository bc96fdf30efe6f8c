"""GPU: mvp_heatmap_peaks against the numpy reference (tests/heatmap_peaks_ref.py), bit for bit:
every comparison the kernel makes is an exact f32 comparison and the decode arithmetic is the
oracle's, so no tolerance applies.  Maps: tests/heatmap_peaks_ref.make_maps."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import heatmap_peaks_ref as hp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mvpose import ops as _ops
    return _ops


@functools.lru_cache(maxsize=None)
def _case(shape):
    """A shape's maps and reference, made once for the tests that share them."""
    N, K, H, W, V = shape
    hm, cs, nan_free = hp.make_maps(N, K, H, W, seed=100 + H)
    return shape, hm, cs, nan_free, hp.PeakReference(hm, cs)


def _shape_id(s):
    return "x".join(map(str, s))


@pytest.fixture(scope="module", params=hp.SHAPES, ids=_shape_id)
def case(request):
    return _case(request.param)


# mvp_heatmap_decode takes maps of at least 3 x 3: the 1 x 1 shape has no decode to agree with
@pytest.fixture(scope="module", params=[s for s in hp.SHAPES if s[2] >= 3 and s[3] >= 3], ids=_shape_id)
def decode_case(request):
    return _case(request.param)


def _same(out, ref):
    """Bit-identical float32, NaN where the reference is NaN."""
    assert out.shape == ref.shape and out.dtype == ref.dtype
    same = (out == ref) | (np.isnan(out) & np.isnan(ref))
    assert same.all(), f"{(~same).sum()} of {same.size} values differ"


def test_against_the_reference(ops, case):
    """radius 1, 2, 3 x min_rel 0, 0.5 x max_peaks 1..4 at thr 0.1, and thr 0.01 (the background
    noise's maxima become peaks: far more peaks than slots) at radius 1."""
    (N, K, H, W, V), hm, cs, _, ref = case
    hd, cd = torch.tensor(hm, device="cuda"), torch.tensor(cs, device="cuda")
    filled = set()
    for radius, thr in ((1, hp.THR), (2, hp.THR), (3, hp.THR), (1, 0.01)):
        for min_rel in (0.0, 0.5):
            for M in (1, 2, 3, 4):
                peaks, counts = ops.heatmap_peaks(hd, cd, max_peaks=M, radius=radius, thr=thr, min_rel=min_rel, n_views=V)
                rp, rc = ref(M, radius, thr, min_rel, V)
                assert np.array_equal(counts.cpu().numpy(), rc), (radius, thr, min_rel, M)
                _same(peaks.cpu().numpy(), rp)
                filled |= set(rc.ravel().tolist())
    if H * W > 1:
        assert {0, 1, 4} <= filled


def test_first_peak_is_the_decode(ops, decode_case):
    """On every NaN-free map slot 0 equals mvp_heatmap_decode's keypoint and score bitwise wherever
    the score exceeds thr."""
    from mvpose import _lib
    (N, K, H, W, V), hm, cs, nan_free, _ = decode_case
    hd, cd = torch.tensor(hm, device="cuda"), torch.tensor(cs, device="cuda")
    kp = torch.empty((N, K, 2), dtype=torch.float32, device="cuda")
    sc = torch.empty((N, K), dtype=torch.float32, device="cuda")
    _lib.call("mvp_heatmap_decode", _lib.ptr(hd), None, N, K, H, W, None, 0, _lib.ptr(cd), 192, 256, None,
              _lib.ptr(kp), _lib.ptr(sc), None, None, 1, _lib.stream(hd.device))
    peaks, counts = ops.heatmap_peaks(hd, cd, max_peaks=2, thr=hp.THR, n_views=1)
    kp, sc, p0 = kp.cpu().numpy(), sc.cpu().numpy(), peaks[:, :, 0, :, 0].cpu().numpy()
    on = nan_free & (sc > hp.THR)
    assert on.any()
    assert (counts[..., 0].cpu().numpy()[on] >= 1).all()
    assert np.array_equal(p0[..., :2][on], kp[on]) and np.array_equal(p0[..., 2][on], sc[on])


def test_counts_null_and_views(ops):
    """counts_dev NULL; the (t, v) crop order lands in the last axis."""
    from mvpose import _lib
    N, K, H, W, V = hp.SHAPES[4]
    hm, cs, _ = hp.make_maps(N, K, H, W, seed=5)
    hd, cd = torch.tensor(hm, device="cuda"), torch.tensor(cs, device="cuda")
    want, _ = ops.heatmap_peaks(hd, cd, max_peaks=3, n_views=V)
    got = torch.full_like(want, 7.0)
    _lib.call("mvp_heatmap_peaks", _lib.ptr(hd), N, K, H, W, _lib.ptr(cd), 192, 256, 3, 1, ctypes.c_float(0.1),
              ctypes.c_float(0.3), V, _lib.ptr(got), None, _lib.stream(hd.device))
    _same(got.cpu().numpy(), want.cpu().numpy())
    flat, _ = ops.heatmap_peaks(hd, cd, max_peaks=3, n_views=1)            # (N, K, 3, 3, 1)
    _same(want.cpu().numpy(), flat[..., 0].reshape(N // V, V, K, 3, 3).permute(0, 2, 3, 4, 1).cpu().numpy())


@pytest.mark.parametrize("H,W", [(64, 64), (41, 100), (128, 96)])
def test_lds_budget_boundary(ops, H, W):
    """The map is staged in LDS while 4 waves x H*W*4 B fit the workgroup's 64 KB: 64 x 64 = 4096
    cells is the last size that does (the full 64 KB launch), 41 x 100 = 4100 cells the first that
    reads the map from memory, 128 x 96 far beyond.  5 maps: a ragged second workgroup."""
    hm, cs, _ = hp.make_maps(1, 5, H, W, seed=9)
    ref = hp.PeakReference(hm, cs)
    peaks, counts = ops.heatmap_peaks(torch.tensor(hm, device="cuda"), torch.tensor(cs, device="cuda"), max_peaks=4,
                                      radius=2, thr=hp.THR, min_rel=0.0)
    rp, rc = ref(4, 2, hp.THR, 0.0)
    assert np.array_equal(counts.cpu().numpy(), rc)
    _same(peaks.cpu().numpy(), rp)


def test_non_default_stream(ops):
    N, K, H, W, V = hp.SHAPES[0]
    hm, cs, _ = hp.make_maps(N, K, H, W, seed=3)
    hd, cd = torch.tensor(hm, device="cuda"), torch.tensor(cs, device="cuda")
    a = ops.heatmap_peaks(hd, cd)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        b = ops.heatmap_peaks(hd, cd)
    st.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
