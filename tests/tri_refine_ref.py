"""fp64 numpy restatement of mvp_triangulate_refine (the normative text is the comment in
include/mvpose.h): the same steps in the same order, vectorised over the points, with
synthetic.project as the forward model.  Nothing here touches the device."""
import numpy as np

from mvpose import synthetic as syn

W_UNIT, W_CONF, W_GAUSS = 0, 1, 2
FAILED, NOT_CONVERGED = 0x80, 0x40


def jacobian(X, cam):
    """d project(X, cam) / dX, (n, 2, 3), analytic; and P_z (n,)."""
    X = np.asarray(X, dtype=np.float64)
    R, T, K = cam["R"], cam["T"].reshape(3), cam["K"]
    k1, k2, p1, p2, k3 = cam["dist"].ravel()
    P = X @ R.T + T
    with np.errstate(all="ignore"):
        iz = 1.0 / P[:, 2]
        x, y = P[:, 0] * iz, P[:, 1] * iz
        r2 = x * x + y * y
        radial = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
        drad = k1 + 2 * k2 * r2 + 3 * k3 * r2 ** 2
        dxx = radial + 2 * x * x * drad + 2 * p1 * y + 6 * p2 * x
        dxy = 2 * x * y * drad + 2 * p1 * x + 2 * p2 * y
        dyy = radial + 2 * y * y * drad + 6 * p1 * y + 2 * p2 * x
        a00, a01 = K[0, 0] * dxx + K[0, 1] * dxy, K[0, 0] * dxy + K[0, 1] * dyy
        a10, a11 = K[1, 1] * dxy, K[1, 1] * dyy
        m0 = (R[0][None, :] - x[:, None] * R[2][None, :]) * iz[:, None]
        m1 = (R[1][None, :] - y[:, None] * R[2][None, :]) * iz[:, None]
        J = np.stack([a00[:, None] * m0 + a01[:, None] * m1, a10[:, None] * m0 + a11[:, None] * m1], axis=1)
    return J, P[:, 2]


def views(kpts, cam_idx, mask_bits, weights, gauss, min_conf, cov_floor):
    """used (n, NV) bool, z (n, NV, 2), W (n, NV, 2, 2) of the listed views."""
    kpts = np.asarray(kpts, dtype=np.float32)
    n, nv = kpts.shape[0], len(cam_idx)
    used = np.zeros((n, nv), bool)
    z = np.zeros((n, nv, 2))
    W = np.zeros((n, nv, 2, 2))
    min_conf, floor = np.float32(min_conf), float(np.float32(cov_floor))
    for i, col in enumerate(cam_idx):
        x, y, c = kpts[:, 0, col], kpts[:, 1, col], kpts[:, 2, col]
        with np.errstate(invalid="ignore"):
            ok = np.isfinite(x) & np.isfinite(y) & ~np.isnan(c) & (c >= min_conf)
        if mask_bits is not None:
            ok &= ((np.asarray(mask_bits).astype(np.uint32) >> i) & 1).astype(bool)
        zi = np.stack([x, y], -1).astype(np.float64)
        Wi = np.zeros((n, 2, 2))
        if weights == W_UNIT:
            Wi[:, 0, 0] = Wi[:, 1, 1] = 1.0
        elif weights == W_CONF:
            Wi[:, 0, 0] = Wi[:, 1, 1] = c.astype(np.float64)
        else:
            Jn = gauss.shape[2]
            g = np.asarray(gauss, dtype=np.float64)[:, col].reshape(n, 6)      # point p = t·J + j
            assert n % Jn == 0
            with np.errstate(all="ignore"):
                sa, sb, sd = g[:, 2] + floor, g[:, 3], g[:, 5] + floor
                det = sa * sd - sb * sb
                ok &= np.isfinite(g).all(1) & ~(g == 0).all(1) & (sa > 0) & (det > 0)
                Wi[:, 0, 0], Wi[:, 0, 1], Wi[:, 1, 0], Wi[:, 1, 1] = sd / det, -sb / det, -sb / det, sa / det
            zi = g[:, :2].copy()
        used[:, i] = ok
        z[ok, i] = zi[ok]
        W[ok, i] = Wi[ok]
    return used, z, W


def evaluate(X, cams, cam_idx, used, z, W):
    """f (n,), g (n, 3), H (n, 3, 3) at X; f = +inf where a used view is not in front."""
    n = X.shape[0]
    f, g, H = np.zeros(n), np.zeros((n, 3)), np.zeros((n, 3, 3))
    front = np.ones(n, bool)
    for i, col in enumerate(cam_idx):
        cam = cams[col]
        J, Pz = jacobian(X, cam)
        with np.errstate(all="ignore"):
            r = syn.project(X, cam) - z[:, i]
            infront = Pz > 0
            add = used[:, i] & infront
            front &= infront | ~used[:, i]
            Wr = np.einsum("nab,nb->na", W[:, i], r)
            WJ = np.einsum("nab,nbk->nak", W[:, i], J)
            f += np.where(add, 0.5 * np.einsum("na,na->n", r, Wr), 0.0)
            g += np.where(add[:, None], np.einsum("nak,na->nk", J, Wr), 0.0)
            H += np.where(add[:, None, None], np.einsum("nak,nal->nkl", J, WJ), 0.0)
    return np.where(front, f, np.inf), g, H


def _chol_solve(A, b):
    """Per-point Cholesky solve; pd False on a pivot that is not > 0 (solution then garbage)."""
    n = A.shape[0]
    x = np.zeros((n, 3))
    pd = np.zeros(n, bool)
    for p in range(n):
        try:
            if not np.isfinite(A[p]).all():
                continue
            L = np.linalg.cholesky(A[p])
            x[p] = np.linalg.solve(L.T, np.linalg.solve(L, b[p]))
            pd[p] = True
        except np.linalg.LinAlgError:
            pass
    return x, pd


def refine(kpts, cams, cam_idx, xyz0, mask_bits=None, weights=W_UNIT, gauss=None, min_conf=0.0, cov_floor=1.0,
           max_iter=10, tol=1e-7):
    """kpts (n, 3, V) f32, cams list of synthetic rig dicts, xyz0 (n, 3) f32, gauss (n/J, V, J, 6).
    Returns dict: xyz (n,3) f32, cov (n,6) f32, cost (n,) f32, status (n,) uint8, X (n,3) f64 (the
    unrounded final point), H (n,3,3) f64."""
    kpts = np.asarray(kpts, dtype=np.float32)
    xyz0 = np.asarray(xyz0, dtype=np.float32)
    n = kpts.shape[0]
    used, z, W = views(kpts, cam_idx, mask_bits, weights, gauss, min_conf, cov_floor)
    X = xyz0.astype(np.float64)
    alive = (used.sum(1) >= 2) & np.isfinite(X).all(1)
    failed = ~alive
    Xs = np.where(alive[:, None], X, 0.0)
    f, g, H = evaluate(Xs, cams, cam_idx, used, z, W)
    failed |= ~np.isfinite(f)
    alive &= np.isfinite(f)
    X = Xs
    lam = np.full(n, 1e-3)
    trials = np.zeros(n, np.int64)
    conv = np.zeros(n, bool)
    for _ in range(int(max_iter)):
        if not alive.any():
            break
        idx = np.arange(3)
        A = H.copy()
        A[:, idx, idx] *= (1.0 + lam)[:, None]
        delta, pd = _chol_solve(np.where(alive[:, None, None], A, np.eye(3)), -g)
        failed |= alive & ~pd
        alive &= pd
        delta = np.where(alive[:, None], delta, 0.0)
        step_ok = np.linalg.norm(delta, axis=1) <= tol * (np.linalg.norm(X, axis=1) + tol)
        Xn = X + delta
        fn, gn, Hn = evaluate(Xn, cams, cam_idx, used, z, W)
        with np.errstate(invalid="ignore"):
            accept = alive & np.isfinite(fn) & (fn <= f)
        lam = np.where(alive, np.where(accept, np.maximum(lam * 0.1, 1e-12), lam * 10.0), lam)
        trials += alive
        conv |= alive & step_ok
        X = np.where(accept[:, None], Xn, X)
        f = np.where(accept, fn, f)
        g = np.where(accept[:, None], gn, g)
        H = np.where(accept[:, None, None], Hn, H)
        alive &= ~conv
    cov = np.full((n, 3, 3), np.nan)
    for p in range(n):
        if failed[p] or not np.isfinite(H[p]).all():
            continue
        try:
            np.linalg.cholesky(H[p])
            cov[p] = np.linalg.inv(H[p])
        except np.linalg.LinAlgError:
            pass
    xyz = np.where(failed[:, None], xyz0, X.astype(np.float32))
    status = np.where(failed, FAILED, trials | np.where(conv, 0, NOT_CONVERGED)).astype(np.uint8)
    cost = np.where(failed, np.nan, f).astype(np.float32)
    cov6 = cov.reshape(n, 9)[:, [0, 1, 2, 4, 5, 8]].astype(np.float32)
    return {"xyz": xyz, "cov": cov6, "cost": cost, "status": status, "X": np.where(failed[:, None], np.nan, X),
            "H": H, "used": used}


# ------------------------------------------------------------------ shared test inputs
def dlt_seed(kpts, cams, cam_idx):
    """The OpenCV-semantics all-views DLT (oracle.cv_ref): kpts (T, J, 3, V) -> (T·J, 3) f32."""
    from oracle import cv_ref
    params = [(c["K"], c["R"], c["T"], c["dist"]) for c in cams]
    return np.asarray(cv_ref.triangulate_all_views(params, kpts, list(cam_idx)), dtype=np.float32).reshape(-1, 3)


def hetero_inputs(V=4, n_frames=12, seed=7):
    """The heteroscedastic inputs: make_rig(V, seed=3), n_frames·17 points, per-view noise drawn from
    anisotropic covariances with eigenvalues in {1, 4, 64} px² at a random orientation.
    Returns cams, gt (n,3), kpts (T,17,3,V) f32, gauss (T,V,17,6) f64 with the TRUE covariances."""
    rng = np.random.default_rng(seed + 1000)      # not the generator state make_poses(seed) starts from
    cams = syn.make_rig(V, seed=3)
    gt = syn.make_poses(n_frames, seed=seed)
    T, Jn = gt.shape[:2]
    kpts = np.zeros((T, Jn, 3, V), np.float32)
    gauss = np.zeros((T, V, Jn, 6))
    for v, cam in enumerate(cams):
        uv = syn.project(gt, cam)
        ev = rng.choice([1.0, 4.0, 64.0], size=(T, Jn, 2))
        th = rng.uniform(0, np.pi, (T, Jn))
        c, s = np.cos(th), np.sin(th)
        Rm = np.stack([np.stack([c, -s], -1), np.stack([s, c], -1)], -2)
        S = np.einsum("tjab,tjb,tjcb->tjac", Rm, ev, Rm)
        noise = np.einsum("tjab,tjb->tja", Rm, rng.normal(size=(T, Jn, 2)) * np.sqrt(ev))
        obs = uv + noise
        kpts[:, :, :2, v] = obs
        kpts[:, :, 2, v] = rng.uniform(0.3, 1.0, (T, Jn))
        # the Gaussian's mean is the float32 keypoint, so "unit" and "heatmap" see the same observation
        gauss[:, v, :, :2] = kpts[:, :, :2, v].astype(np.float64)
        gauss[:, v, :, 2], gauss[:, v, :, 3], gauss[:, v, :, 4], gauss[:, v, :, 5] = (
            S[..., 0, 0], S[..., 0, 1], S[..., 0, 1], S[..., 1, 1])
    return cams, gt.reshape(-1, 3), kpts, gauss
