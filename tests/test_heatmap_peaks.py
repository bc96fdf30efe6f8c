"""CPU: mvp_heatmap_peaks rejects bad arguments before any device work, and the numpy reference
the GPU test compares against agrees with the oracle's MSRAHeatmap decode on its first peak and
with a brute-force reading of the peak definition."""
import numpy as np
import pytest

import heatmap_peaks_ref as hp
from oracle import heatmap_ref


def _call(N=4, K=17, H=64, W=48, input_w=192, input_h=256, max_peaks=4, radius=1, thr=0.1, min_rel=0.3, V=1):
    from mvpose import _lib
    rc = _lib.lib.mvp_heatmap_peaks(None, N, K, H, W, None, input_w, input_h, max_peaks, radius, thr, min_rel, V,
                                    None, None, None)
    return rc, _lib.last_error()


@pytest.mark.parametrize("kw,msg", [
    (dict(max_peaks=0), "max_peaks=0"),
    (dict(max_peaks=5), "max_peaks=5"),
    (dict(radius=0), "radius=0"),
    (dict(radius=4), "radius=4"),
    (dict(thr=float("nan")), "thr is NaN"),
    (dict(min_rel=-0.1), "min_rel"),
    (dict(min_rel=1.5), "min_rel"),
    (dict(min_rel=float("nan")), "min_rel"),
    (dict(V=0), "V=0"),
    (dict(N=4, V=3), "V=3"),
    (dict(H=512, W=256), "H*W"),
    (dict(K=33), "K=33"),
    (dict(K=0), "K=0"),
    (dict(input_w=0), "input size"),
])
def test_bad_arguments_are_reported(kw, msg):
    rc, err = _call(**kw)
    assert rc == -1
    assert msg in err, err


def test_null_pointers_and_empty_batch():
    rc, err = _call()
    assert rc == -1 and "NULL device pointer" in err
    rc, _ = _call(N=0)                 # no maps: a no-op, before the pointer checks
    assert rc == 0


def _brute_force(hm, radius, thr):
    """The peak definition read cell by cell."""
    H, W = hm.shape
    found = []
    for y in range(H):
        for x in range(W):
            v, i = hm[y, x], y * W + x
            if np.isnan(v) or not v > np.float32(thr):
                continue
            ok = True
            for yy in range(max(y - radius, 0), min(y + radius, H - 1) + 1):
                for xx in range(max(x - radius, 0), min(x + radius, W - 1) + 1):
                    u, n = hm[yy, xx], yy * W + xx
                    if n != i and not (np.isnan(u) or v > u or (v == u and i < n)):
                        ok = False
            if ok:
                found.append((-float(v), i))
    return [i for _, i in sorted(found)]


@pytest.mark.parametrize("shape", hp.SHAPES[1:])
def test_reference_follows_the_definition(shape):
    N, K, H, W, V = shape
    hm, cs, _ = hp.make_maps(N, K, H, W, seed=7)
    for radius in (1, 2, 3):
        for thr in (hp.THR, 0.01):
            for n in range(N):
                for k in range(K):
                    assert list(hp.find_peaks(hm[n, k], radius, thr)) == _brute_force(hm[n, k], radius, thr)


def test_first_peak_is_the_decoded_argmax():
    """On NaN-free 64x48 maps whose maximum exceeds thr, slot 0 is heatmap_ref.msra_decode +
    keypoints_to_image, bit for bit; unfilled slots hold NaN, NaN, 0; the maps' contents are there."""
    N, K, H, W, V = hp.SHAPES[0]
    hm, cs, nan_free = hp.make_maps(N, K, H, W, seed=11)
    peaks, counts = hp.PeakReference(hm, cs)(4, 1, hp.THR, 0.0)
    assert peaks.shape == (N, K, 4, 3, 1) and counts.shape == (N, K, 1)
    seen = set()
    for n in range(N):
        kp, sc, _ = heatmap_ref.msra_decode(hm[n])
        img = heatmap_ref.keypoints_to_image(kp, cs[n, :2], cs[n, 2:])
        for k in range(K):
            c = counts[n, k, 0]
            seen.add(int(c))
            assert np.isnan(peaks[n, k, c:, :2, 0]).all() and (peaks[n, k, c:, 2, 0] == 0).all()
            assert (np.diff(peaks[n, k, :c, 2, 0]) <= 0).all()
            if nan_free[n, k] and sc[k] > hp.THR:
                assert c >= 1 and np.array_equal(peaks[n, k, 0, :2, 0], img[k]) and peaks[n, k, 0, 2, 0] == sc[k]
    assert {0, 1, 4} <= seen                                   # nothing above thr ... more peaks than slots
    half, chalf = hp.PeakReference(hm, cs)(4, 1, hp.THR, 0.5)
    assert (chalf <= counts).all() and (chalf < counts).any()
    kept = np.arange(4)[None, None, :, None] < chalf[:, :, None, :]
    assert (half[:, :, :, 2][kept] >= np.float32(0.5) * np.broadcast_to(half[:, :, :1, 2], kept.shape)[kept]).all()
