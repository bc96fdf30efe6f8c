"""Inputs of the mvp_triangulate_peaks tests, shared by the CPU check of their margins
(tests/test_triangulate_peaks.py) and the GPU comparison (tests/test_triangulate_peaks_gpu.py);
a case's reference result is computed once per process."""
import functools

import numpy as np

from mvpose import synthetic as syn
from tri_peaks_ref import INLIER_PX, PeaksReference

MIN_CONF = 0.2
FRAMES = 15                    # x 17 joints = 255 points: a block of 128, a second with a tail of lanes
CASES = [(3, 2), (3, 4), (4, 2), (4, 4), (8, 2), (8, 4)]      # (views, slots)
_SEED = {3: 101, 4: 102, 8: 103}


def _decoy(rng, xy):
    r, th = rng.uniform(80.0, 300.0), rng.uniform(0.0, 2 * np.pi)
    return xy + np.array([r * np.cos(th), r * np.sin(th)], np.float32)


def make_case(V, M, frames=FRAMES):
    """make_rig(V) / make_poses / 1 px noise.  Returns (cams, peaks (frames, 17, M, 3, V) float32,
    truth mask (frames, 17, V) bool, truth slot (frames, 17, V) int8, -1 outside the mask).

    An ordinary view holds the truth in a random slot r: the slots before it are not valid (a
    score below MIN_CONF or NaN coordinates), so the truth is the view's top candidate; the slots
    after it hold decoys 80-300 px away, or nothing.  Per point, up to 1 view (V = 3, 4) or 3
    views (V = 8) are bad instead:
        0  a valid decoy in a lower slot outranks the truth (which stays in the view)
        1  the truth is absent: decoys only
        2  the view is empty
    V = 3 takes kind 0 only, so that at least 3 views hold the truth at every point."""
    seed = _SEED[V] + 10 * M
    cams = syn.make_rig(V, seed=seed)
    k = syn.make_kpts_2d(syn.make_poses(frames, seed=seed + 1), cams, seed=seed + 2, noise_px=1.0)
    rng = np.random.default_rng(seed + 3)
    T, J = k.shape[:2]
    peaks = np.zeros((T, J, M, 3, V), np.float32)
    peaks[:, :, :, :2] = np.nan                                     # unfilled: x = y = NaN, score 0
    mask = np.zeros((T, J, V), bool)
    slot = np.full((T, J, V), -1, np.int8)
    max_bad = 3 if V == 8 else 1
    for t in range(T):
        for j in range(J):
            bad = rng.choice(V, size=rng.integers(0, max_bad + 1), replace=False)
            for v in range(V):
                xy = k[t, j, :2, v]
                kind = int(rng.integers(0, 1 if V == 3 else 3)) if v in bad else -1
                if kind == 2:
                    continue
                scores = np.sort(rng.uniform(0.3, 0.95, M))[::-1].astype(np.float32)
                if kind == 1:
                    for m in range(int(rng.integers(1, M + 1))):
                        peaks[t, j, m, :2, v], peaks[t, j, m, 2, v] = _decoy(rng, xy), scores[m]
                    continue
                r = int(rng.integers(1, M)) if kind == 0 else int(rng.integers(0, M))
                for m in range(r):
                    peaks[t, j, m, :2, v], peaks[t, j, m, 2, v] = _decoy(rng, xy), scores[m]
                    if kind != 0 and rng.integers(0, 2):
                        peaks[t, j, m, 2, v] = 0.05                 # below MIN_CONF
                    elif kind != 0:
                        peaks[t, j, m, 0, v] = np.nan               # NaN x beside a good score
                peaks[t, j, r, :2, v], peaks[t, j, r, 2, v] = xy, scores[r]
                for m in range(r + 1, int(rng.integers(r + 1, M + 1))):
                    peaks[t, j, m, :2, v], peaks[t, j, m, 2, v] = _decoy(rng, xy), scores[m]
                mask[t, j, v], slot[t, j, v] = True, r
    return cams, peaks, mask, slot


@functools.lru_cache(maxsize=None)
def case_with_reference(V, M):
    """(cams, peaks, truth mask, truth slot, reference, (xyz, mask, sel, err)) of make_case(V, M)
    over all V views at INLIER_PX / MIN_CONF; the arrays are shared: do not write to them."""
    cams, peaks, mask, slot = make_case(V, M)
    ref = PeaksReference(cams, list(range(V)))
    res = ref(peaks, inlier_px=INLIER_PX, min_conf=MIN_CONF)
    for a in (peaks, mask, slot) + res:
        a.setflags(write=False)
    return cams, peaks, mask, slot, ref, res
