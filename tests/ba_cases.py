"""Inputs of the bundle-adjustment tests (tests/test_bundle_adjust.py, tests/test_bundle_adjust_gpu.py),
all from mvpose.synthetic.  Nothing here touches the device."""
import functools

import numpy as np

import ba_ref
import tri_refine_ref as tr
from mvpose import synthetic as syn


def perturbed_rig(cams, which, deg, cm, seed):
    """The rig with the cameras `which` rotated by `deg` about a random axis and moved by `cm`."""
    rng = np.random.default_rng(seed)
    out = [dict(c) for c in cams]
    for v in which:
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        du = rng.normal(size=3)
        du *= cm / np.linalg.norm(du)
        out[v] = ba_ref.perturb(cams[v], np.concatenate([np.deg2rad(deg) * ax, du]))
    return out


def linear_seed(kpts, cams, cam_idx):
    """A plain fp64 DLT on distortion-free pixels of the listed views (the seed only has to be
    near): kpts (n, 3, V) -> (n, 3) f32."""
    n = kpts.shape[0]
    rows = []
    for col in cam_idx:
        c = cams[col]
        P = c["K"] @ np.hstack([c["R"], c["T"].reshape(3, 1)])
        x, y = kpts[:, 0, col].astype(np.float64), kpts[:, 1, col].astype(np.float64)
        rows += [x[:, None] * P[2] - P[0], y[:, None] * P[2] - P[1]]
    A = np.stack(rows, 1)
    _, _, vt = np.linalg.svd(A)
    h = vt[:, -1]
    return (h[:, :3] / h[:, 3:]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def recovery(n_frames=120, noise_px=0.5, seed=11):
    """make_rig(4), n_frames·17 points, cameras 2 and 3 perturbed by 1 degree and 3 cm; seeds from the
    perturbed cameras.  Returns dict: true (rig), cams (perturbed rig), kpts (n, 3, 4), xyz0 (n, 3),
    shape (T, J)."""
    true = syn.make_rig(4, seed=3)
    poses = syn.make_poses(n_frames, seed=seed)
    k4 = syn.make_kpts_2d(poses, true, seed=seed + 1, noise_px=noise_px)
    cams = perturbed_rig(true, (2, 3), 1.0, 3.0, seed + 2)
    kpts = np.ascontiguousarray(k4.reshape(-1, 3, 4))
    return {"true": true, "cams": cams, "kpts": kpts, "kpts4": k4, "xyz0": linear_seed(kpts, cams, [0, 1, 2, 3]),
            "shape": k4.shape[:2]}


# the runs of mvp_bundle_adjust that the GPU tests compare: name -> keyword arguments
RUNS = {
    "two_fixed": dict(cam_idx=[0, 1, 2, 3], free=[2, 3], weights=tr.W_UNIT, max_iter=30, tol=1e-3),
    "one_fixed_prior": dict(cam_idx=[0, 1, 2, 3], free=[1, 2, 3], weights=tr.W_CONF, trans_prior_sigma=3.0,
                            max_iter=30, tol=1e-3),
    "huber": dict(cam_idx=[0, 1, 2, 3], free=[2, 3], weights=tr.W_UNIT, huber_delta=1.5, max_iter=30, tol=1e-3),
}


@functools.lru_cache(maxsize=None)
def reference_run(name):
    """The restatement's run of RUNS[name] on the recovery inputs."""
    rc = recovery()
    kw = dict(RUNS[name])
    cam_idx, free = kw.pop("cam_idx"), kw.pop("free")
    return ba_ref.bundle_adjust(rc["kpts"], rc["cams"], cam_idx, free, rc["xyz0"], **kw)


def system_case(nv, free, n, V=None, cam_idx=None, weights=tr.W_UNIT, dirty=True, seed=5):
    """Inputs of one mvp_bundle_adjust_system comparison: n points seen by nv listed views of a rig of
    V cameras.  dirty: masked views, NaN keypoints, low-confidence views (min_conf = 0.35), points
    with one used view, a non-finite seed, a seed behind a camera.  Returns a dict."""
    V = V or nv
    cam_idx = list(cam_idx) if cam_idx is not None else list(range(nv))
    rng = np.random.default_rng(seed + 100 * nv + n)
    cams = syn.make_rig(V, seed=3)
    T = -(-n // syn.N_JOINTS)
    poses = syn.make_poses(T, seed=seed)
    k4 = syn.make_kpts_2d(poses, cams, seed=seed + 1, noise_px=0.5)
    kpts = np.ascontiguousarray(k4.reshape(-1, 3, V)[:n])
    xyz = (poses.reshape(-1, 3)[:n] + rng.normal(0.0, 0.5, (n, 3))).astype(np.float32)
    mask = None
    gauss = None
    if weights == tr.W_GAUSS:
        # heatmap layout (T, V, J, 6): needs whole frames
        assert n % syn.N_JOINTS == 0
        gauss = np.zeros((T, V, syn.N_JOINTS, 6))
        for v in range(V):
            gauss[:, v, :, 0] = k4[:, :, 0, v]
            gauss[:, v, :, 1] = k4[:, :, 1, v]
            a, d = rng.uniform(1.0, 9.0, (T, syn.N_JOINTS)), rng.uniform(1.0, 9.0, (T, syn.N_JOINTS))
            b = rng.uniform(-0.5, 0.5, (T, syn.N_JOINTS)) * np.sqrt(a * d)
            gauss[:, v, :, 2], gauss[:, v, :, 3], gauss[:, v, :, 4], gauss[:, v, :, 5] = a, b, b, d
    if dirty:
        mask = np.full(n, (1 << nv) - 1, np.uint8)
        for p in range(0, n, 7):
            mask[p] &= ~np.uint8(1 << int(rng.integers(nv)))
        for p in range(3, n, 11):
            kpts[p, int(rng.integers(2)), cam_idx[int(rng.integers(nv))]] = np.nan
        for p in range(5, n, 13):
            kpts[p, 2, cam_idx[int(rng.integers(nv))]] = 0.2          # below min_conf
        if n >= 40:
            mask[20] = 1 << (nv - 1)                                   # one used view
            xyz[25, 1] = np.inf                                        # a seed that is not finite
            xyz[30] = (0.0, 0.0, -400.0)                               # a seed behind camera 0
            if gauss is not None:
                gauss[0, cam_idx[0], 3] = 0.0                          # an empty heatmap's record
    return {"cams": cams, "kpts": kpts, "xyz": xyz, "mask": mask, "gauss": gauss, "cam_idx": cam_idx,
            "free": sorted(free), "weights": weights, "min_conf": 0.35 if dirty else 0.0, "shape": (T, syn.N_JOINTS)}


def reference_system(case, lam, hub, sigma):
    """The restatement's S, b, cost and counts of a system_case."""
    used, z, W = tr.views(case["kpts"], case["cam_idx"], case["mask"], case["weights"], case["gauss"], case["min_conf"], 1.0)
    act = ba_ref.active_points(case["xyz"], case["cams"], case["cam_idx"], used)
    gaps = []
    lin = ba_ref.system(case["xyz"].astype(np.float64), case["cams"], case["cams"], case["cam_idx"], case["free"], act,
                        used, z, W, lam, hub, sigma, gaps)
    return lin["S"], lin["b"], lin["cost"], int(act.sum()), int((used & act[:, None]).sum()), (min(gaps) if gaps else np.inf)


# mvp_bundle_adjust_system comparisons: system_case's arguments plus lam / hub / sigma.  Each shape
# is the smallest that reaches its path: one lane, a wave less one, a wave plus one, more than one
# pass of 256 workgroups of 64 (20 405 > 16 384); 6F + 1 <= 16, 32, 48 rows and the full 43.
SYSTEM_CASES = [
    dict(nv=4, free=[1, 2, 3], n=1, dirty=False),
    dict(nv=4, free=[1, 2, 3], n=63, lam=1e-3),
    dict(nv=4, free=[1, 2, 3], n=65, lam=1e-3, hub=1.0),
    dict(nv=8, free=[1, 2, 3, 4, 5, 6, 7], n=20405, lam=1e-3, hub=1.7, sigma=3.0, weights=tr.W_CONF),
    dict(nv=2, free=[1], n=130, sigma=3.0),
    dict(nv=3, free=[0, 2], n=130, lam=1e-3),
    dict(nv=4, free=[1, 3], n=130, hub=1.0),                       # non-contiguous free_mask
    dict(nv=3, free=[0, 2], n=130, V=4, cam_idx=[2, 0, 3], lam=1e-3, weights=tr.W_CONF),
    dict(nv=8, free=[0, 1, 2, 4, 5, 7], n=130, lam=1e-3, sigma=3.0),
    dict(nv=8, free=[0, 1, 2, 3, 4, 5, 6], n=130, hub=1.0, weights=tr.W_CONF),
    dict(nv=4, free=[2, 3], n=136, weights=tr.W_GAUSS, lam=1e-3, hub=1.0, sigma=3.0),
    dict(nv=4, free=[2, 3], n=136, weights=tr.W_GAUSS),
]


def case_args(kw):
    return {k: v for k, v in kw.items() if k not in ("lam", "hub", "sigma")}


def case_id(kw):
    return "-".join(f"{k}{'.'.join(map(str, v)) if isinstance(v, list) else v}" for k, v in kw.items())


@functools.lru_cache(maxsize=None)
def rough():
    """Inputs whose run rejects trials: 340 points of the recovery set, cameras 2 and 3 off by 10
    degrees and 30 cm, seeds 150 cm (standard deviation) off.  Returns dict: cams, kpts, xyz0, kw."""
    rc = recovery()
    n = 340
    cams = perturbed_rig(rc["true"], (2, 3), 10.0, 30.0, 3)
    rng = np.random.default_rng(3)
    xyz0 = (linear_seed(rc["kpts"][:n], cams, [0, 1, 2, 3]) + rng.normal(0.0, 150.0, (n, 3))).astype(np.float32)
    return {"cams": cams, "kpts": rc["kpts"][:n], "xyz0": xyz0,
            "kw": dict(weights=tr.W_CONF, max_iter=12, tol=1e-3)}


@functools.lru_cache(maxsize=None)
def rough_reference_run():
    r = rough()
    return ba_ref.bundle_adjust(r["kpts"], r["cams"], [0, 1, 2, 3], [2, 3], r["xyz0"], **r["kw"])
