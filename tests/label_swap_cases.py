"""Scenes for the label-swap tests: a moving synthetic subject seen by nv cameras with 1 px noise,
into which left/right exchanges are injected per unit and per view.

``scene(nv, T, seed, units, drops)`` -> dict(cams, cam_idx, pairs, units, clean (the keypoints
before the injection), kpts (after it), truth (T, U) uint8, gauss / gauss_clean (T, V, J, 6)
float64 random records exchanged with the keypoints)."""
import functools

import numpy as np

from mvpose import swaps, synthetic as syn


def inject(T, U, nv, seed):
    """Per unit and per view three runs, start in [T/10, T-2), length in [1, 25); a run that
    overlaps an already swapped frame of that unit (in any view) is skipped.  -> (T, U) uint8."""
    rng = np.random.default_rng(7000 + seed)
    truth = np.zeros((T, U), np.uint8)
    if T < 4:
        return truth
    for u in range(U):
        for v in range(nv):
            for _ in range(3):
                start = int(rng.integers(max(T // 10, 1), T - 2))
                stop = min(start + int(rng.integers(1, 25)), T)
                if truth[start:stop, u].any():
                    continue
                truth[start:stop, u] |= np.uint8(1 << v)
    return truth


def exchange(kpts, truth, cam_idx, pairs, units, gauss=None):
    """The injection itself (and its inverse): plain numpy, independent of label_swap_ref.apply."""
    out = kpts.copy()
    gout = None if gauss is None else gauss.copy()
    for t, u in zip(*np.nonzero(truth)):
        for a, col in enumerate(cam_idx):
            if not (truth[t, u] >> a) & 1:
                continue
            for (l, r), pu in zip(pairs, units):
                if pu != u:
                    continue
                out[t, [l, r], :, col] = kpts[t, [r, l], :, col]
                if gauss is not None:
                    gout[t, col, [l, r]] = gauss[t, col, [r, l]]
    return out, gout


@functools.lru_cache(maxsize=None)
def scene(nv, T, seed, units="limbs", drops=False):
    cams = syn.make_rig(nv, seed=0)
    clean = syn.make_kpts_2d(syn.make_poses(T, seed=seed, jitter=1.0), cams, seed=seed + 1, noise_px=1.0)
    rng = np.random.default_rng(9000 + seed)
    if drops:
        clean[:, :, 0, :][rng.uniform(size=(T, syn.N_JOINTS, nv)) < 0.1] = np.nan
    pairs, unit = swaps.preset(units)
    pairs, unit = pairs.tolist(), unit.tolist()
    cam_idx = list(range(nv))
    U = max(unit) + 1
    truth = inject(T, U, nv, seed)
    gauss_clean = rng.normal(size=(T, nv, syn.N_JOINTS, 6))
    kpts, gauss = exchange(clean, truth, cam_idx, pairs, unit, gauss_clean)
    for a in (clean, kpts, truth, gauss, gauss_clean):
        a.setflags(write=False)
    return dict(cams=cams, cam_idx=cam_idx, pairs=pairs, units=unit, clean=clean, kpts=kpts, truth=truth,
                gauss=gauss, gauss_clean=gauss_clean)


def same_bits(a, b):
    """Bit-for-bit equality of two float arrays (NaN payloads included)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# the no-drop scenes the CPU test and the GPU end-to-end test share: (nv, T, seed, units)
NO_DROP = [(nv, 120 if nv >= 7 else 240, seed, units)
           for nv in (2, 3, 4, 7, 8) for seed in (3, 4, 5, 6) for units in ("limbs", "body")]
