"""Inputs of the tests of the trajectory fit with sub-frame camera offsets
(tests/test_trajectory_fit_lag.py, tests/test_trajectory_fit_lag_gpu.py), all from mvpose.synthetic,
with the patterns of tests/traj_fit_cases.py.  Nothing here touches the device."""
import functools

import numpy as np

import traj_fit_cases as tc
import traj_fit_lag_ref as tl
import tri_refine_ref as tr
from mvpose import synthetic as syn

MIN_CONF = tc.MIN_CONF
MAX_ITER, TOL = tc.MAX_ITER, tc.TOL      # TOL large on purpose, as there

# The GPU cases.  Shapes (T, P, nv, chunk) and patterns as in traj_fit_cases.CASES; frac: the views'
# offsets.  T = 1 (always invalid), 2 (valid only with two views that
# have no offset), 3; chunk 4 with T = 5, 6, 7, 8, 13: the lane period is 6, so
# the block between neighbouring frames lands inside a chunk, across the edge of a separator, inside
# a separator and behind the last one; T = 257: the tile sum has 256 frames; T = 200 with the
# automatic chunk; 1, 3, 65 chains; 2, 3, 4, 8 views; offsets all zero, some zero, one at 0.999.
# behind: the seed frame lies behind the first listed camera, whose offset 0.4 puts that frame's Y
# behind it too (and the frame before's in front).  seed: change it when a decision margin falls
# short.
CASES = [
    dict(T=1, P=1, nv=2, chunk=0, weights=tr.W_UNIT, lam=1.0, frac=(0.0, 0.5)),
    dict(T=2, P=3, nv=3, chunk=0, weights=tr.W_UNIT, lam=1.0, starved=2, frac=(0.0, 0.0, 0.4), seed=1),
    dict(T=3, P=1, nv=3, chunk=4, weights=tr.W_CONF, lam=0.25, frac=(0.25, 0.0, 0.999)),
    dict(T=5, P=17, nv=2, chunk=4, weights=tr.W_UNIT, lam=4.0, drop=0.3, nan_seed=(3, 2), frac=(0.0, 0.0)),
    dict(T=6, P=17, nv=3, chunk=4, weights=tr.W_GAUSS, lam=1.0, mask=True, V=4, cam_idx=[2, 0, 3],
         frac=(0.3, 0.0, 0.6)),
    dict(T=7, P=5, nv=2, chunk=4, weights=tr.W_CONF, lam=1.0, hub=1.5, behind=(1, 4), noise=40.0, frac=(0.4, 0.0)),
    dict(T=8, P=3, nv=2, chunk=4, weights=tr.W_UNIT, lam=1.0, frac=(0.0, 0.999)),
    dict(T=13, P=17, nv=4, chunk=4, weights=tr.W_CONF, lam=0.25, drop=0.3, mask=True, hub=1.5,
         blind=((2, 9), 4, 5), frac=(0.0, 0.4, 0.75, 0.1)),
    dict(T=40, P=65, nv=2, chunk=4, weights=tr.W_GAUSS, lam=4.0, single=(range(0, 65, 3), 15, 10),
         blind=((7, 40), 3, 5), nan_seed=(20, 39), behind=(33, 0), starved=64, frac=(0.4, 0.0)),
    dict(T=200, P=17, nv=8, chunk=0, weights=tr.W_CONF, lam=1.0, drop=0.3, hub=2.0, single=((5, 6), 100, 10),
         frac=(0.0, 0.4, 0.0, 0.75, 0.1, 0.0, 0.9, 0.5)),
    dict(T=257, P=3, nv=2, chunk=0, weights=tr.W_CONF, lam=1.0, frac=(0.2, 0.7)),
    # a seed 150 cm off (traj_fit_cases' "rough"): chain 0 rejects 5 trials and then converges in its
    # 11th, chain 4 rejects 3 and runs out of its 12 trials (0x4C); test_trajectory_fit_lag.py asserts
    # that this occurs.  Besides the margins the seed has to leave the restatement reproducible: from
    # 150 cm off a chain can start next to a camera's plane, with costs of 1e23 and more and matrices
    # singular to rounding, where changing lambda by 1e-13 of itself moves the result by tens of cm
    # (seed 255 does); such a chain checks nothing.  test_rough_case_is_well_conditioned holds this seed to it.
    dict(T=7, P=5, nv=2, chunk=4, weights=tr.W_CONF, lam=1.0, behind=(1, 4), noise=150.0, rng=349, tag="rough",
         frac=(0.4, 0.0)),
]
ROUGH = len(CASES) - 1


def case_id(kw):
    return f"T{kw['T']}-P{kw['P']}-nv{kw['nv']}-chunk{kw['chunk']}" + (f"-{kw['tag']}" if "tag" in kw else "")


def lerp(truth, a):
    """The path at the instants t + a, linear between the frames (the last frame: itself)."""
    nxt = np.concatenate([truth[1:], truth[-1:]])
    return (1.0 - a) * truth + a * nxt


def make_kpts(truth, cams, cam_idx, frac, seed, noise_px=1.0, at=None):
    """(T, P, 3, V) float32: listed view i sees the path at t + frac[i] (at(a): the path there;
    default linear between the frames), the other columns at t."""
    at = (lambda a: lerp(truth, a)) if at is None else at
    a_of = dict(zip(cam_idx, frac))
    kpts = np.empty(truth.shape[:2] + (3, len(cams)), np.float32)
    for v in range(len(cams)):
        kpts[..., v] = syn.make_kpts_2d(at(a_of.get(v, 0.0)), cams, seed=seed + 1 + 7 * v, noise_px=noise_px)[..., v]
    return kpts


@functools.lru_cache(maxsize=None)
def case(i):
    """The inputs of CASES[i], as traj_fit_cases.case returns them, plus frac."""
    kw = CASES[i]
    T, P, nv = kw["T"], kw["P"], kw["nv"]
    V = kw.get("V", nv)
    cam_idx = list(kw.get("cam_idx", range(nv)))
    frac = np.array(kw["frac"], np.float64)
    seed = kw["rng"] if "rng" in kw else kw.get("seed", 0) + 10 * i + 1000
    rng = np.random.default_rng(seed)
    cams = syn.make_rig(V, seed=3)
    truth = tc.people_poses(T, P, seed)
    kpts = make_kpts(truth, cams, cam_idx, frac, seed)
    gauss = tc.make_gauss(kpts, rng) if kw["weights"] == tr.W_GAUSS else None
    xyz0 = (truth + rng.normal(0.0, kw.get("noise", 2.0), truth.shape)).astype(np.float32)
    if kw.get("drop"):
        for t, p, j in zip(*np.nonzero(rng.uniform(size=(T, P, nv)) < kw["drop"])):
            tc.drop_view(kpts, gauss, t, p, cam_idx[j], int(rng.integers(2)))
    if "single" in kw:
        chains, t0, n = kw["single"]
        for p in chains:
            for t in range(t0, t0 + n):
                for j in range(1, nv):
                    tc.drop_view(kpts, gauss, t, p, cam_idx[j], (t + j) % 2)
    if "blind" in kw:
        chains, t0, n = kw["blind"]
        for p in chains:
            for t in range(t0, t0 + n):
                for j in range(nv):
                    tc.drop_view(kpts, gauss, t, p, cam_idx[j], (t + j) % 2)
    if "starved" in kw:
        for t in range(1, T):
            for j in range(1, nv):
                tc.drop_view(kpts, gauss, t, kw["starved"], cam_idx[j], 0)
    mask = None
    if kw.get("mask"):
        mask = np.full((T, P), (1 << nv) - 1, np.uint8)
        flat = mask.reshape(-1)
        for e in range(0, T * P, 7):
            flat[e] &= ~np.uint8(1 << int(rng.integers(nv)))
    if "nan_seed" in kw:
        p, t = kw["nan_seed"]
        xyz0[t, p, 1] = np.nan
    if "behind" in kw:
        p, t = kw["behind"]
        c0 = cams[cam_idx[0]]
        xyz0[t, p] = (c0["R"].T @ (np.array([0.0, 0.0, -400.0]) - c0["T"].reshape(3))).astype(np.float32)
        kpts[t, p, :, cam_idx[0]] = kpts[(t + 1) % T, p, :, cam_idx[0]]
        kpts[t, p, 2, cam_idx[0]] = 0.9
        if gauss is not None:
            gauss[t, cam_idx[0], p] = (kpts[t, p, 0, cam_idx[0]], kpts[t, p, 1, cam_idx[0]], 4.0, 0.5, 0.5, 3.0)
        if mask is not None:
            mask[t, p] |= 1
    solver = dict(mask_bits=mask, weights=kw["weights"], gauss=gauss, min_conf=MIN_CONF, cov_floor=1.0,
                  huber_delta=kw.get("hub", 0.0))
    return {"cams": cams, "cam_idx": cam_idx, "frac": frac, "kpts": np.ascontiguousarray(kpts), "xyz0": xyz0,
            "mask": mask, "gauss": gauss, "truth": truth, "kw": solver, "lam": kw["lam"], "chunk": kw["chunk"],
            "max_iter": kw.get("max_iter", MAX_ITER)}


@functools.lru_cache(maxsize=None)
def reference_fit(i):
    """The restatement's run of case i."""
    c = case(i)
    return tl.fit(c["kpts"], c["cams"], c["cam_idx"], c["frac"], c["xyz0"], lambda_smooth=c["lam"],
                  max_iter=c["max_iter"], tol=TOL, **c["kw"])


@functools.lru_cache(maxsize=None)
def reference_system(i):
    c = case(i)
    return tl.system(c["kpts"], c["cams"], c["cam_idx"], c["frac"], c["xyz0"], **c["kw"])


# ------------------------------------------------------------------ the accuracy scene
SCENE_T, SCENE_FPS, SCENE_HZ = 120, 30.0, 1.0
SCENE_FRAC = (0.0, 0.4, 0.75)          # planted
SCENE_LAMBDA = 0.25
SCENE_JOINTS = 4
SCENE_START = (0.3, 0.3)               # where the offset search starts for views 1 and 2
# What the restatement measures on the scene (test_trajectory_fit_lag.py asserts that it still
# does; the GPU test asks for half the ratio and twice the deviation):
#   RMS error of the fit with every offset zero, and with the planted ones, in cm
SCENE_RMS_ZERO, SCENE_RMS_TRUE = 2.16, 0.46
#   the offsets of views 1 and 2 that the search of sync.refine_frame_offsets recovers
SCENE_RECOVERED = (0.423, 0.777)


def scene_path(tau, joint):
    """Joint `joint` at the rig instants tau (frames): a 40 x 30 cm ellipse at SCENE_HZ, each joint
    with its own centre, phase and plane."""
    w = 2.0 * np.pi * SCENE_HZ / SCENE_FPS
    ph = 0.9 * joint
    c = syn.make_poses(1, seed=5, jitter=0.0)[0, 3 * joint]
    u = np.array([np.cos(0.5 * joint), 0.0, np.sin(0.5 * joint)])
    v = np.array([0.0, 1.0, 0.0])
    tau = np.asarray(tau, np.float64)[:, None]
    return c + 20.0 * np.cos(w * tau + ph) * u + 15.0 * np.sin(w * tau + ph) * v


@functools.lru_cache(maxsize=None)
def scene(hz=SCENE_HZ):
    """make_rig(3, seed=3), SCENE_JOINTS joints on scene_path, view i at t + SCENE_FRAC[i], 1 px
    noise.  Returns dict: cams, kpts (T, J, 3, 3) f32, truth (T, J, 3) at the integer instants, seed
    (T, J, 3) f32: the truth 2 cm (standard deviation) off."""
    cams = syn.make_rig(3, seed=3)
    t = np.arange(SCENE_T, dtype=np.float64)
    scale = hz / SCENE_HZ

    def at(a):
        return np.stack([scene_path((t + a) * scale, j) for j in range(SCENE_JOINTS)], 1)
    truth = at(0.0)
    kpts = make_kpts(truth, cams, [0, 1, 2], SCENE_FRAC, seed=77, at=at)
    rng = np.random.default_rng(78)
    seed = (truth + rng.normal(0.0, 2.0, truth.shape)).astype(np.float32)
    return {"cams": cams, "kpts": kpts, "truth": truth, "seed": seed}


def scene_rms(xyz, truth):
    """RMS error over the frames both have, the last frame left out (views with an offset do not
    see it)."""
    d = np.asarray(xyz, np.float64)[:-1] - truth[:-1]
    return float(np.sqrt((d * d).sum(-1).mean()))


def align(kpts, seed, s):
    """What sync.split_frame_offsets and sync.apply_frame_offsets do to the scene for offsets s:
    (kpts cut to the common instants, the seed at those instants, a, first rig instant)."""
    from mvpose import sync
    n, a = sync.split_frame_offsets(s)
    (k,), _ = sync.apply_frame_offsets([kpts], n, [3])
    lo = int(n.max())
    return np.ascontiguousarray(k), seed[lo:lo + k.shape[0]], a, lo


@functools.lru_cache(maxsize=None)
def scene_reference(hz=SCENE_HZ):
    """The restatement on the scene: the fit with zero offsets, with the planted ones, and the
    offset search from SCENE_START.  Returns (rms_zero, rms_true, s (3,), info)."""
    sc = scene(hz)

    def run(s):
        k, x0, a, lo = align(sc["kpts"], sc["seed"], s)
        r = tl.fit(k, sc["cams"], [0, 1, 2], a, x0, weights=tr.W_CONF, lambda_smooth=SCENE_LAMBDA, max_iter=30,
                   tol=1e-6)
        return r, lo

    def reduced(s):
        r, _ = run(s)
        ok = r["status"] != tl.INVALID
        ga = np.zeros(3)
        for p in np.flatnonzero(ok):
            ga = ga + r["dlag"][p, :, 0]
        return ga, float(r["cost"][ok, 1].sum())
    r0, _ = run(np.zeros(3))
    r1, _ = run(np.array(SCENE_FRAC))
    s, info = tl.newton_offsets(reduced, np.array((0.0,) + SCENE_START))
    return scene_rms(r0["X"], sc["truth"]), scene_rms(r1["X"], sc["truth"]), s, info
