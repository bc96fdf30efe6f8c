"""Inputs of the tracking tests (mvp_track_people): people walking through a room as per-frame
groups in random slot order, with dropouts, lost joints and noise, and the cases the GPU test
compares against tests/track_ref.py.  Everything is continuous random data, so that no two costs
of a frame and no cost and its limit come closer than the margin tests/test_people_track.py asks."""
import functools

import numpy as np

import track_ref
from mvpose import synthetic as syn


def walk(T, J, seed, start, step):
    """(T, J, 3) float64: a skeleton whose root moves from start by step per frame.  J = 17: the
    articulated poses of synthetic.make_poses about its own slow root walk; else a rigid cloud."""
    if J == syn.N_JOINTS:
        body = syn.make_poses(T, seed=seed, jitter=0.0) - syn.SUBJECT_CENTER
    else:
        rng = np.random.default_rng(9000 + seed)
        body = rng.normal(0.0, 20.0, (1, J, 3)) + np.cumsum(rng.normal(0.0, 1.0, (T, 1, 3)), 0)
    return body + np.asarray(start, float) + np.arange(T)[:, None, None] * np.asarray(step, float)


def groups(tracks, spans, G, seed, noise=1.0, lost=0.10):
    """tracks: list of (T, J, 3); spans: per person the list of (first, last + 1) frame ranges the
    person is observed in -> (xyz (T, G, J, 3) float32, truth (T, G) int, -1 = empty slot): each
    frame's observed people in a random permutation of the slots, a fraction `lost` of the joints
    NaN (never a person's every joint) and `noise` cm of Gaussian noise."""
    T, J = tracks[0].shape[:2]
    rng = np.random.default_rng(5000 + seed)
    xyz = np.full((T, G, J, 3), np.nan, np.float32)
    truth = np.full((T, G), -1, int)
    for t in range(T):
        slots = rng.permutation(G)
        for p, (tr, sp) in enumerate(zip(tracks, spans)):
            if not any(a <= t < b for a, b in sp):
                continue
            obs = tr[t] + rng.normal(0.0, noise, (J, 3))
            gone = rng.uniform(size=J) < lost
            gone[rng.integers(J)] = False
            obs[gone] = np.nan
            xyz[t, slots[p]] = obs
            truth[t, slots[p]] = p
    return xyz, truth


@functools.lru_cache(maxsize=None)
def designed_scene():
    """T = 60, G = 4.  Persons 0 and 1 cross, 60 cm apart in z, at 5 cm per frame each (frame 30);
    person 0 drops out for frames 20-22 and person 1 for frames 40-41; person 2 enters at frame 10
    and leaves at frame 50.  Slots permuted per frame, 10 % of the joints lost, 1 cm of noise."""
    T = 60
    tracks = [walk(T, 17, 1, (-150.0, 0.0, 0.0), (5.0, 0.0, 0.0)),
              walk(T, 17, 2, (150.0, 0.0, 60.0), (-5.0, 0.0, 0.0)),
              walk(T, 17, 3, (0.0, 0.0, 300.0), (0.0, 0.0, 1.0))]
    spans = [[(0, 20), (23, T)], [(0, 40), (42, T)], [(10, 50)]]
    return groups(tracks, spans, 4, seed=11)


def _crowd(n_people, G, T, J, seed, max_drop):
    """n_people on a 150 cm grid, each with a slow drift and random dropouts of 1..max_drop frames."""
    rng = np.random.default_rng(3000 + seed)
    tracks, spans = [], []
    for p in range(n_people):
        start = (150.0 * (p % 3), 0.0, 150.0 * (p // 3))
        tracks.append(walk(T, J, 10 * seed + p, start, rng.normal(0.0, 1.5, 3)))
        sp, t = [], int(rng.integers(0, 3))
        while t < T:
            end = min(T, t + int(rng.integers(3, 12)))
            sp.append((t, end))
            t = end + int(rng.integers(1, max_drop + 1))
        spans.append(sp)
    return groups(tracks, spans, G, seed=seed)[0]


@functools.lru_cache(maxsize=None)
def gpu_cases():
    """name -> (xyz (T, G, J, 3) or (M, T, G, J, 3) float32, keyword arguments of the tracker)."""
    c = {}
    rng = np.random.default_rng(77)
    two = [walk(1, 17, 1, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)), walk(1, 17, 2, (100.0, 0.0, 0.0), (0.0, 0.0, 0.0))]
    c["T1_G3"] = (groups(two, [[(0, 1)], [(0, 1)]], 3, seed=1)[0], dict())
    pt = rng.normal(0.0, 10.0, (2, 1, 1, 3)).astype(np.float32)
    c["T2_G1_J1"] = (pt, dict(max_gap=0))
    for gap in (0, 1, 3, 5):
        c[f"scene_gap{gap}"] = (designed_scene()[0], dict(max_gap=gap))
    # all 1 024 combinations, 16 per lane, the ring at its largest
    c["G8_gap15_T40"] = (_crowd(7, 8, 40, 17, 2, 18), dict(max_gap=15, gap_growth=0.25))
    # J = 255, G = 7, max_gap = 1: 64 736 bytes of LDS; one more frame of gap or one more group is refused
    c["J255_G7_gap1"] = (_crowd(5, 7, 6, 255, 3, 1), dict(max_gap=1))
    # a group with 3 seen joints: it links to nothing and nothing links to it
    x = _crowd(4, 6, 24, 17, 4, 4)
    for t in (5, 6, 13):
        g = int(np.flatnonzero(np.isfinite(x[t]).all(-1).any(-1))[0])
        keep = np.flatnonzero(np.isfinite(x[t, g]).all(-1))[:3]
        row = np.full_like(x[t, g], np.nan)
        row[keep] = x[t, g, keep]
        x[t, g] = row
    c["min_joints5_G6_gap9"] = (x, dict(max_gap=9, min_joints=5))
    # a longer sequence: the ring of 4 slots goes round 32 times
    c["T130_G3_gap2"] = (_crowd(2, 3, 130, 17, 8, 3), dict(max_gap=2))
    c["all_nan"] =(np.full((5, 3, 17, 3), np.nan, np.float32), dict(max_gap=2))
    c["M3_G5_gap7"] = (np.stack([_crowd(3 + m, 5, 20, 17, 5 + m, 9) for m in range(3)]), dict(max_gap=7))
    return c


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement's result for a case; a list of per-sequence results for an (M, ...) case."""
    xyz, kw = gpu_cases()[name]
    if xyz.ndim == 5:
        return [track_ref.track(s, **kw) for s in xyz]
    return track_ref.track(xyz, **kw)
