"""Inputs of the skeleton-fit tests (tests/test_skeleton_fit.py, tests/test_skeleton_fit_gpu.py), all
from mvpose.synthetic.  Nothing here touches the device."""
import functools
import json
import os

import numpy as np

import ba_cases
import skel_fit_ref as sk
import traj_fit_cases as tc
import traj_smooth_ref as ts
import tri_refine_ref as tr
from mvpose import synthetic as syn
from mvpose.refine import SEGMENTS

MIN_CONF = tc.MIN_CONF
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "body_part_lengths.json")) as _f:
    BODY_LENGTHS = json.load(_f)["my_lengths"]            # the reference's 12 segments, in its YAML's order
PAIRS17 = [SEGMENTS[name] for name in BODY_LENGTHS]
PAIRS4 = [(0, 1), (2, 1), (2, 3), (3, 0), (0, 2)]         # J = 4: a cycle and a diagonal, both orders of an end

# The GPU cases.  Shapes (T, G, J, nv, chunk): one frame; two; fewer frames than a chunk and more
# (T = 40 with chunk 4 crosses separators); the automatic chunk; one person and three; one joint, four,
# seventeen.  Patterns, by (group, joint[, frame]): drop = share of the views dropped at random;
# single = (chains, first frame, frames) seen by view 0 only; nan_seed / behind = (chain, frame) of a
# seed frame that is NaN / behind camera 0 (an invalid chain inside a valid group); dead_group = a
# group whose every seed is NaN; dead_len = (group, segment, value) lengths that are not live;
# zero = (chain a, chain b, frame): the seed of b is a's in that frame, so that r == 0 exactly at
# the seed; noise = the seed's standard deviation about the truth (150: trials are rejected).
CASES = [
    dict(T=1, G=1, J=1, nv=2, chunk=0, weights=tr.W_UNIT, lam=1.0, beta=1.0),            # T = 1: always invalid
    dict(T=2, G=3, J=4, nv=2, chunk=0, weights=tr.W_UNIT, lam=1.0, beta=1.0, zero=(4, 5, 1)),
    dict(T=7, G=1, J=17, nv=3, chunk=4, weights=tr.W_GAUSS, lam=1.0, beta=4.0, mask=True, V=4, cam_idx=[2, 0, 3],
         dead_len=[(0, 3, np.nan), (0, 8, -1.0)], zero=(5, 7, 3)),
    dict(T=7, G=3, J=4, nv=2, chunk=4, weights=tr.W_CONF, lam=1.0, beta=1.0, hub=1.5, drop=0.2, nan_seed=(6, 2),
         dead_group=2),
    dict(T=40, G=3, J=17, nv=2, chunk=4, weights=tr.W_CONF, lam=0.25, beta=1.0,
         single=((7, 9, 17 + 8, 34 + 13), 15, 12), dead_len=[(1, 0, np.inf), (1, 5, 0.0)], behind=(17 + 16, 0),
         nan_seed=(3, 20)),
    dict(T=130, G=1, J=17, nv=3, chunk=0, weights=tr.W_CONF, lam=1.0, beta=2.0, hub=2.0, drop=0.3, mask=True),
    dict(T=40, G=3, J=1, nv=2, chunk=0, weights=tr.W_CONF, lam=1.0, beta=1.0, drop=0.3, nan_seed=(1, 7)),
    # Seeds 150 cm (standard deviation) off.  test_skeleton_fit.py asserts what these reach: rejected
    # trials, a group that converges after rejections, groups that run out of their trials.
    dict(T=7, G=3, J=4, nv=2, chunk=4, weights=tr.W_CONF, lam=1.0, beta=1.0, noise=150.0, rng=19, tag="rough"),
    dict(T=7, G=3, J=4, nv=2, chunk=4, weights=tr.W_CONF, lam=1.0, beta=1.0, hub=1.5, noise=150.0, rng=19, tag="short",
         max_iter=3),
]
# TOL is large on purpose, as in traj_fit_cases.py: every run stops on a trial whose two comparisons
# are clear (test_skeleton_fit.py checks the margins).
MAX_ITER, TOL = 12, 1e-2
J1_CASE = 6                    # compared with ops.trajectory_fit on the same inputs
CHUNK_CASES = (4, 5)           # run with chunk 4 and with the automatic chunk


def case_id(kw):
    return f"T{kw['T']}-G{kw['G']}-J{kw['J']}-nv{kw['nv']}-chunk{kw['chunk']}" + (f"-{kw['tag']}" if "tag" in kw else "")


@functools.lru_cache(maxsize=None)
def case(i):
    """The inputs of CASES[i]: dict with cams, cam_idx, kpts (T, P, 3, V) f32, xyz0 (T, P, 3) f32, mask
    (T, P) uint8 bits or None, gauss or None, truth, J, pairs, lengths (G, n_seg) f32, and kw, the
    trajectory fit's keyword arguments."""
    kw = CASES[i]
    T, G, J, nv = kw["T"], kw["G"], kw["J"], kw["nv"]
    P = G * J
    V = kw.get("V", nv)
    cam_idx = list(kw.get("cam_idx", range(nv)))
    seed = kw["rng"] if "rng" in kw else 100 + 10 * i
    rng = np.random.default_rng(seed)
    cams = syn.make_rig(V, seed=3)
    truth = np.concatenate([syn.make_poses(T, seed=seed + g, jitter=1.0)[:, :J] + np.array([25.0 * g, 0.0, 15.0 * g])
                            for g in range(G)], 1)
    kpts = syn.make_kpts_2d(truth, cams, seed=seed + 1, noise_px=1.0)
    gauss = tc.make_gauss(kpts, rng) if kw["weights"] == tr.W_GAUSS else None
    xyz0 = (truth + rng.normal(0.0, kw.get("noise", 2.0), truth.shape)).astype(np.float32)
    pairs = {1: [], 4: PAIRS4, 17: PAIRS17}[J]
    # a person's lengths: the median over the frames, 1 % off
    tg = truth.reshape(T, G, J, 3)
    lengths = np.zeros((G, len(pairs)), np.float32)
    for s, (a, b) in enumerate(pairs):
        lengths[:, s] = np.median(np.linalg.norm(tg[:, :, b] - tg[:, :, a], axis=-1), 0) * rng.uniform(0.99, 1.01, G)
    for g, s, v in kw.get("dead_len", []):
        lengths[g, s] = v
    if kw.get("drop"):
        for t, p, j in zip(*np.nonzero(rng.uniform(size=(T, P, nv)) < kw["drop"])):
            tc.drop_view(kpts, gauss, t, p, cam_idx[j], int(rng.integers(2)))
    if "single" in kw:
        chains, t0, n = kw["single"]
        for p in chains:
            for t in range(t0, t0 + n):
                for j in range(1, nv):
                    tc.drop_view(kpts, gauss, t, p, cam_idx[j], (t + j) % 2)
    mask = None
    if kw.get("mask"):
        mask = np.full((T, P), (1 << nv) - 1, np.uint8)
        flat = mask.reshape(-1)
        for e in range(0, T * P, 7):
            flat[e] &= ~np.uint8(1 << int(rng.integers(nv)))
    if "zero" in kw:
        a, b, t = kw["zero"]
        xyz0[t, b] = xyz0[t, a]
    if "nan_seed" in kw:
        p, t = kw["nan_seed"]
        xyz0[t, p, 1] = np.nan
    if "dead_group" in kw:
        g = kw["dead_group"]
        xyz0[T // 2, g * J:(g + 1) * J, 0] = np.nan
    if "behind" in kw:
        p, t = kw["behind"]
        c0 = cams[cam_idx[0]]                                  # a point 400 behind the first listed camera
        xyz0[t, p] = (c0["R"].T @ (np.array([0.0, 0.0, -400.0]) - c0["T"].reshape(3))).astype(np.float32)
        kpts[t, p, :, cam_idx[0]] = kpts[(t + 1) % T, p, :, cam_idx[0]]          # and that camera's view is used
        kpts[t, p, 2, cam_idx[0]] = 0.9
    solver = dict(mask_bits=mask, weights=kw["weights"], gauss=gauss, min_conf=MIN_CONF, cov_floor=1.0,
                  huber_delta=kw.get("hub", 0.0))
    return {"cams": cams, "cam_idx": cam_idx, "kpts": np.ascontiguousarray(kpts), "xyz0": xyz0, "mask": mask,
            "gauss": gauss, "truth": truth, "J": J, "pairs": pairs, "lengths": lengths, "kw": solver, "lam": kw["lam"],
            "beta": kw["beta"], "chunk": kw["chunk"], "max_iter": kw.get("max_iter", MAX_ITER)}


@functools.lru_cache(maxsize=None)
def reference_fit(i):
    """The restatement's run of case i."""
    c = case(i)
    return sk.fit(c["kpts"], c["cams"], c["cam_idx"], c["xyz0"], c["J"], c["pairs"], c["lengths"], lambda_bone=c["beta"],
                  lambda_smooth=c["lam"], max_iter=c["max_iter"], tol=TOL, **c["kw"])


@functools.lru_cache(maxsize=None)
def reference_system(i):
    c = case(i)
    return sk.system(c["kpts"], c["cams"], c["cam_idx"], c["xyz0"], c["J"], c["pairs"], c["lengths"], c["beta"], **c["kw"])


# ------------------------------------------------------------------ the arm scene
ARM_GAP = (40, 80)             # camera 1 loses ARM_JOINTS in these frames
ARM_JOINTS = (7, 9)            # left elbow, left wrist
ARM_LAMBDA, ARM_BETA, ARM_TOL, ARM_MAX_ITER = 0.25, 1.0, 1e-4, 60
# The factor by which the restatement's fit with bones lowers the blind fill's RMS error over the gap
# frames of ARM_JOINTS (measured 5.17: 17.00 cm -> 3.29 cm, 18 trials; test_skeleton_fit.py asserts the restatement
# reaches the constant, the GPU test asks for half of it).
ARM_FACTOR = 5.1


@functools.lru_cache(maxsize=None)
def arm_scene(seed=0):
    """make_rig(2), make_poses(120, jitter=0), 1 px noise, camera 1 without ARM_JOINTS in ARM_GAP.
    Returns dict: cams, kpts (120, 17, 3, 2) f32, truth, tri (120, 17, 3) f32: the per-frame
    maximum-likelihood points of the two-view frames, NaN where a joint is lost; pairs and lengths:
    the 12 segments at their true lengths."""
    cams = syn.make_rig(2)
    truth = syn.make_poses(120, seed=seed, jitter=0.0)
    full = syn.make_kpts_2d(truth, cams, seed=seed + 1, noise_px=1.0)
    kpts = full.copy()
    kpts[ARM_GAP[0]:ARM_GAP[1], list(ARM_JOINTS), :2, 1] = np.nan
    flat = np.ascontiguousarray(full.reshape(-1, 3, 2))
    tri = tr.refine(flat, cams, [0, 1], ba_cases.linear_seed(flat, cams, [0, 1]), weights=tr.W_CONF)["xyz"]
    tri = tri.reshape(120, syn.N_JOINTS, 3).copy()
    tri[ARM_GAP[0]:ARM_GAP[1], list(ARM_JOINTS)] = np.nan
    lengths = np.array([np.linalg.norm(truth[0, b] - truth[0, a]) for a, b in PAIRS17], np.float32)
    return {"cams": cams, "kpts": kpts, "truth": truth, "tri": tri, "pairs": PAIRS17, "lengths": lengths}


def arm_rms(xyz, truth):
    """RMS error over the gap frames of ARM_JOINTS."""
    sel = list(ARM_JOINTS)
    d = np.asarray(xyz, np.float64)[ARM_GAP[0]:ARM_GAP[1]][:, sel] - truth[ARM_GAP[0]:ARM_GAP[1]][:, sel]
    return float(np.sqrt((d * d).sum(-1).mean()))


@functools.lru_cache(maxsize=None)
def arm_reference(beta=ARM_BETA, seed=0):
    """The restatement on the arm scene: the smoother's seed (the blind fill) and the fit from it."""
    a = arm_scene(seed)
    seed_xyz = ts.solve_dense(a["tri"], lambda_smooth=ARM_LAMBDA, sigma0=1.0).xyz
    fit = sk.fit(a["kpts"], a["cams"], [0, 1], seed_xyz, 17, a["pairs"], a["lengths"][None], lambda_bone=beta,
                 weights=tr.W_CONF, lambda_smooth=ARM_LAMBDA, max_iter=ARM_MAX_ITER, tol=ARM_TOL)
    return seed_xyz, fit
