"""Inputs of the association tests: several mvpose.synthetic people in one rig, each camera-frame
listing the people it sees in person slots of shuffled order.

``scene`` places G people on a 90 cm circle around the rig's subject centre, drops 15 % of the
(person, view, frame) sightings, shuffles the slot order per (frame, view) and sets 10 % of the
joints to NaN.  ``gpu_cases`` lists every input the GPU test compares against the restatement;
``reference`` runs tests/people_ref.py on a case once per process (the CPU test asserts the
comparison margins of exactly these inputs, the GPU test compares against the same results).
"""
import functools

import numpy as np

import people_ref
from mvpose import synthetic as syn

RADIUS_CM = 90.0


def scene(n_people, n_cams, P, T, seed, noise_px=1.0, J=17, drop=0.15, nan_joints=0.10):
    """-> (cams, kpts (T, P, J, 3, V) float32 with NaN for empty slots and lost joints,
    truth (T, V, P) int: the person in each slot, -1 for an empty slot)."""
    assert n_people <= P
    cams = syn.make_rig(n_cams, seed=seed)
    rng = np.random.default_rng(7000 + seed)
    kpts = np.full((T, P, J, 3, n_cams), np.nan, np.float32)
    truth = np.full((T, n_cams, P), -1, int)
    per_person = []
    for g in range(n_people):
        th = 2 * np.pi * g / n_people
        poses = syn.make_poses(T, seed=100 * seed + g, jitter=0.0)
        poses = poses + RADIUS_CM * np.array([np.cos(th), 0.0, np.sin(th)])
        # more than 17 joints: further copies of the skeleton, 12 cm apart
        reps = -(-J // syn.N_JOINTS)
        poses = np.concatenate([poses + 12.0 * r for r in range(reps)], axis=1)[:, :J]
        per_person.append(syn.make_kpts_2d(poses, cams, seed=100 * seed + 50 + g, noise_px=noise_px))
    seen = rng.uniform(size=(T, n_cams, n_people)) >= drop
    for t in range(T):
        for v in range(n_cams):
            slots = rng.permutation(P)
            for g in range(n_people):
                if seen[t, v, g]:
                    kpts[t, slots[g], :, :, v] = per_person[g][t, :, :, v]
                    truth[t, v, slots[g]] = g
    lost = rng.uniform(size=(T, P, J, n_cams)) < nan_joints
    kpts[:, :, :, 0, :][lost] = np.nan
    return cams, kpts, truth


def _data_case():
    """(4, 4) with an empty frame, a node with 3 joints, two usable nodes of one person with 3
    joints in common, and a slot whose confidences are all below min_conf = 0.35 (which also
    removes the joints of every other slot with a confidence under it)."""
    cams, k, truth = scene(3, 4, 4, 6, seed=31, drop=0.0)       # every person in every view
    k[0] = np.nan
    k[1, int(np.flatnonzero(truth[1, 0] == 0)[0]), 3:, 0, 0] = np.nan
    for v, keep in ((0, slice(0, 10)), (1, slice(7, 17))):
        for p in range(4):
            if truth[2, v, p] == 1:
                m = np.ones(17, bool)
                m[keep] = False
                k[2, p, m, 0, v] = np.nan
    k[3, :, :, 2, 2] = np.where(truth[3, 2][:, None] == 2, np.float32(0.1), k[3, :, :, 2, 2])
    return cams, k


@functools.lru_cache(maxsize=None)
def gpu_cases():
    """name -> (cams, kpts, cam_idx, keyword arguments of the association)."""
    c = {}

    def add(name, sc, cam_idx=None, **kw):
        cams, k = sc[0], sc[1]
        c[name] = (cams, k, tuple(range(len(cams))) if cam_idx is None else cam_idx, kw)

    add("nv2_P1_T5", scene(1, 2, 1, 5, seed=1))
    add("nv2_P3_T67", scene(2, 2, 3, 67, seed=2))
    add("nv3_P2_J1_T5_V5", scene(2, 5, 2, 5, seed=3, J=1, nan_joints=0.0), cam_idx=(3, 0, 4), min_joints=1)
    add("nv5_P3_J33_T5", scene(3, 5, 3, 5, seed=4, J=33))
    add("nv4_P4_T67", scene(4, 4, 4, 67, seed=5, noise_px=2.0))
    add("nv8_P8_T1", scene(6, 8, 8, 1, seed=6))
    add("nv2_P32_T1", scene(12, 2, 32, 1, seed=7))
    add("nv8_P8_J60_T2", scene(5, 8, 8, 2, seed=8, J=60))          # the pixels do not fit in LDS
    add("data", _data_case(), min_conf=0.35)
    add("singletons_nv4_P4", scene(3, 4, 4, 5, seed=9), max_cost_px=0.05)
    add("views_only_nv4_P4", scene(4, 4, 4, 5, seed=10), max_cost_px=1000.0, trunc_px=1e4)
    add("views_only_nv8_P8", scene(6, 8, 8, 1, seed=11), max_cost_px=1000.0, trunc_px=1e4)
    return c


@functools.lru_cache(maxsize=None)
def reference(name):
    cams, k, cam_idx, kw = gpu_cases()[name]
    return people_ref.associate(k, cams, list(cam_idx), **kw)


def same_partition(group, truth):
    """group (NV, P) from the association, truth (NV, P) person ids (-1 = empty): every occupied
    slot is labelled, and two slots share a group exactly when they show the same person."""
    g, p = group.ravel(), truth.ravel()
    occ = p >= 0
    if (g[occ] < 0).any() or (g[~occ] >= 0).any():
        return False
    g, p = g[occ], p[occ]
    return bool(((g[:, None] == g[None, :]) == (p[:, None] == p[None, :])).all())
