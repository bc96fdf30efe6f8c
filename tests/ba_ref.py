"""fp64 numpy restatement of the bundle adjustment (mvp_bundle_adjust_system / mvp_bundle_adjust; the
normative text is the comment in include/mvpose.h): synthetic.project as the forward model, dense
Jacobians, the reduced camera system by plain linear algebra, and the Levenberg-Marquardt loop as
stated.  The used-view / observation / weight rule is tri_refine_ref.views (the text says it is
mvp_triangulate_refine's).  Nothing here touches the device."""
import numpy as np

import tri_refine_ref as tr
from mvpose import synthetic as syn

INACTIVE = 0x80


def skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def rodrigues(w):
    """exp([w]x); I + [w]x below 1e-12."""
    w = np.asarray(w, dtype=np.float64)
    th = np.linalg.norm(w)
    K = skew(w)
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1.0 - np.cos(th)) / th ** 2 * (K @ K)


def perturb(cam, dc):
    """The camera with R <- exp([dw]x)·R, T <- T + du, dc = (dw, du)."""
    out = dict(cam)
    out["R"] = rodrigues(dc[:3]) @ cam["R"]
    out["T"] = cam["T"].reshape(3, 1) + np.asarray(dc[3:], dtype=np.float64).reshape(3, 1)
    return out


def jacobians(X, cam):
    """J_X (n, 2, 3) = A·R, J_c (n, 2, 6) = A·[-[P - T]x, I], P_z (n,); A = d pixel / dP."""
    X = np.asarray(X, dtype=np.float64)
    R, T, K = cam["R"], cam["T"].reshape(3), cam["K"]
    k1, k2, p1, p2, k3 = cam["dist"].ravel()
    q = X @ R.T
    P = q + T
    n = X.shape[0]
    with np.errstate(all="ignore"):
        iz = 1.0 / P[:, 2]
        x, y = P[:, 0] * iz, P[:, 1] * iz
        r2 = x * x + y * y
        radial = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
        drad = k1 + 2 * k2 * r2 + 3 * k3 * r2 ** 2
        dxx = radial + 2 * x * x * drad + 2 * p1 * y + 6 * p2 * x
        dxy = 2 * x * y * drad + 2 * p1 * x + 2 * p2 * y
        dyy = radial + 2 * y * y * drad + 6 * p1 * y + 2 * p2 * x
        D = np.zeros((n, 2, 2))          # d pixel / d(x, y)
        D[:, 0, 0], D[:, 0, 1] = K[0, 0] * dxx + K[0, 1] * dxy, K[0, 0] * dxy + K[0, 1] * dyy
        D[:, 1, 0], D[:, 1, 1] = K[1, 1] * dxy, K[1, 1] * dyy
        N = np.zeros((n, 2, 3))          # d(x, y) / dP
        N[:, 0, 0] = N[:, 1, 1] = iz
        N[:, 0, 2], N[:, 1, 2] = -x * iz, -y * iz
        A = D @ N
        JX = A @ R
        mq = np.zeros((n, 3, 3))         # -[q]x
        mq[:, 0, 1], mq[:, 0, 2] = q[:, 2], -q[:, 1]
        mq[:, 1, 0], mq[:, 1, 2] = -q[:, 2], q[:, 0]
        mq[:, 2, 0], mq[:, 2, 1] = q[:, 1], -q[:, 0]
        Jc = np.concatenate([A @ mq, A], axis=2)
    return JX, Jc, P[:, 2]


def active_points(X, cams, cam_idx, used):
    """>= 2 used views, finite X, P_z > 0 in every used view."""
    X = np.asarray(X, dtype=np.float64)
    act = (used.sum(1) >= 2) & np.isfinite(X).all(1)
    Xs = np.where(act[:, None], X, 0.0)
    for i, col in enumerate(cam_idx):
        Pz = (Xs @ cams[col]["R"].T + cams[col]["T"].reshape(3))[:, 2]
        act &= ~used[:, i] | (Pz > 0)
    return act


def residual_terms(X, cam, z, W, hub):
    """r (n, 2), s (n,), omega (n,), rho (n,), P_z (n,) of one view."""
    with np.errstate(all="ignore"):
        r = syn.project(X, cam) - z
        Pz = (X @ cam["R"].T + cam["T"].reshape(3))[:, 2]
        s2 = np.einsum("na,nab,nb->n", r, W, r)
        s = np.sqrt(s2)
        quad = np.ones_like(s, bool) if not hub > 0 else ~(s > hub)
        om = np.where(quad, 1.0, hub / np.where(quad, 1.0, s))
        rho = np.where(quad, 0.5 * s2, hub * (s - 0.5 * hub))
    return r, s, om, rho, Pz


def prior_cost(cams, cams0, cam_idx, free, sigma):
    if not sigma > 0:
        return 0.0
    return sum(0.5 * float(((cams[cam_idx[i]]["T"] - cams0[cam_idx[i]]["T"]) ** 2).sum()) / sigma ** 2 for i in free)


def cost(X, cams, cam_idx, act, used, z, W, hub, huber_gap=None):
    """Σ rho over the used views of the active points; +inf when one of them has P_z <= 0."""
    f, front = 0.0, True
    Xs = np.where(act[:, None], X, 0.0)
    for i, col in enumerate(cam_idx):
        _, s, _, rho, Pz = residual_terms(Xs, cams[col], z[:, i], W[:, i], hub)
        u = act & used[:, i]
        front = front and bool((Pz[u] > 0).all())
        f += float(rho[u].sum())
        if huber_gap is not None and hub > 0 and u.any():
            huber_gap.append(float(np.abs(s[u] - hub).min() / hub))
    return f if front else np.inf


def system(X, cams, cams0, cam_idx, free, act, used, z, W, lam, hub, sigma, huber_gap=None):
    """The linearisation at (cams, X) with damping lam.  free: ascending view positions.  Returns a
    dict: S (6F, 6F), b (6F,), cost (Σ rho), pd (every V* and S positive definite), and the pieces
    the step needs."""
    n, F = X.shape[0], len(free)
    Xs = np.where(act[:, None], np.asarray(X, dtype=np.float64), 0.0)
    V, g = np.zeros((n, 3, 3)), np.zeros((n, 3))
    Wp = np.zeros((n, 6 * F, 3))
    U, gc = np.zeros((6 * F, 6 * F)), np.zeros(6 * F)
    f = 0.0
    for i, col in enumerate(cam_idx):
        cam = cams[col]
        r, s, om, rho, _ = residual_terms(Xs, cam, z[:, i], W[:, i], hub)
        JX, Jc, _ = jacobians(Xs, cam)
        u = act & used[:, i]
        if huber_gap is not None and hub > 0 and u.any():
            huber_gap.append(float(np.abs(s[u] - hub).min() / hub))
        Wt = np.where(u[:, None, None], om[:, None, None] * W[:, i], 0.0)
        r = np.where(u[:, None], r, 0.0)
        JX = np.where(u[:, None, None], JX, 0.0)
        Jc = np.where(u[:, None, None], Jc, 0.0)
        f += float(rho[u].sum())
        V += np.einsum("nak,nab,nbl->nkl", JX, Wt, JX)
        g += np.einsum("nak,nab,nb->nk", JX, Wt, r)
        if i in free:
            k = 6 * free.index(i)
            Wp[:, k:k + 6] = np.einsum("nak,nab,nbl->nkl", Jc, Wt, JX)
            U[k:k + 6, k:k + 6] = np.einsum("nak,nab,nbl->kl", Jc, Wt, Jc)
            gc[k:k + 6] = np.einsum("nak,nab,nb->k", Jc, Wt, r)
    idx = np.arange(3)
    Vs = V.copy()
    Vs[:, idx, idx] *= 1.0 + lam
    Vs[~act] = np.eye(3)
    pd = True
    try:
        np.linalg.cholesky(Vs)
        pd = bool(np.isfinite(Vs).all())
    except np.linalg.LinAlgError:
        pd = False
    Vinv = np.linalg.inv(Vs) if pd else np.full_like(Vs, np.nan)
    Us = U + lam * np.diag(np.diag(U))
    for k, i in enumerate(free):
        if sigma > 0:
            Us[6 * k + 3:6 * k + 6, 6 * k + 3:6 * k + 6] += np.eye(3) / sigma ** 2
            gc[6 * k + 3:6 * k + 6] += (cams[cam_idx[i]]["T"] - cams0[cam_idx[i]]["T"]).reshape(3) / sigma ** 2
    WV = np.einsum("nkl,nlm->nkm", Wp, Vinv)
    S = Us - np.einsum("nkm,njm->kj", WV, Wp)
    b = -gc + np.einsum("nkm,nm->k", WV, g)
    return {"S": S, "b": b, "cost": f, "pd": pd, "Wp": Wp, "Vinv": Vinv, "g": g}


def solve_step(lin):
    """dc, dX of a linearisation; ok False on a pivot of S that is not > 0."""
    if not lin["pd"] or not np.isfinite(lin["S"]).all():
        return None, None, False
    try:
        L = np.linalg.cholesky(lin["S"])
    except np.linalg.LinAlgError:
        return None, None, False
    dc = np.linalg.solve(L.T, np.linalg.solve(L, lin["b"]))
    dX = -np.einsum("nkl,nl->nk", lin["Vinv"], lin["g"] + np.einsum("nkm,k->nm", lin["Wp"], dc))
    return dc, dX, True


def bundle_adjust(kpts, cams, cam_idx, free, xyz0, mask_bits=None, weights=tr.W_UNIT, gauss=None, min_conf=0.0,
                  cov_floor=1.0, huber_delta=0.0, trans_prior_sigma=0.0, max_iter=30, tol=1e-6):
    """kpts (n, 3, V) f32, cams: list of rig dicts, free: view positions, xyz0 (n, 3) f32.  Returns a
    dict: cams (list of dicts), X (n, 3) f64, xyz (n, 3) f32, point_status, cov (6F, 6F), info (8,),
    margins (relative margins of the accept and stop comparisons), huber_gap (smallest |s - delta| /
    delta seen)."""
    kpts = np.asarray(kpts, dtype=np.float32)
    xyz0 = np.asarray(xyz0, dtype=np.float32)
    free = sorted(int(i) for i in free)
    hub = float(huber_delta) if huber_delta > 0 else 0.0
    sigma = float(trans_prior_sigma) if trans_prior_sigma > 0 else 0.0
    used, z, W = tr.views(kpts, cam_idx, mask_bits, weights, gauss, min_conf, cov_floor)
    cams0 = [dict(c) for c in cams]
    cur = [dict(c) for c in cams]
    act = active_points(xyz0, cams0, cam_idx, used)
    X = np.where(act[:, None], xyz0.astype(np.float64), 0.0)
    margins, gaps = [], []
    f = cost(X, cur, cam_idx, act, used, z, W, hub, gaps)
    f_seed = f
    lam, trials, accepted, status = 1e-3, 0, 0, 1
    starved = any((act & used[:, i]).sum() < 3 for i in free)
    if starved:
        status = 3
    while not starved and trials < max_iter:
        lin = system(X, cur, cams0, cam_idx, free, act, used, z, W, lam, hub, sigma, gaps)
        dc, dX, ok = solve_step(lin)
        trials += 1
        ft = np.inf
        if ok:
            trial = [dict(c) for c in cur]
            for k, i in enumerate(free):
                trial[cam_idx[i]] = perturb(cur[cam_idx[i]], dc[6 * k:6 * k + 6])
            Xt = X + np.where(act[:, None], dX, 0.0)
            ft = cost(Xt, trial, cam_idx, act, used, z, W, hub, gaps) + prior_cost(trial, cams0, cam_idx, free, sigma)
            if np.isfinite(ft):
                margins.append(abs(ft - f) / abs(f))
        if ok and np.isfinite(ft) and ft <= f:
            conv = (f - ft) <= tol * f
            margins.append(abs((f - ft) - tol * f) / abs(f))
            X, cur, f = Xt, trial, ft
            lam = max(lam * 0.1, 1e-12)
            accepted += 1
            if conv:
                status = 0
                break
        else:
            lam = lam * 10.0
            if lam > 1e12:
                status = 2
                break
    lin = system(X, cur, cams0, cam_idx, free, act, used, z, W, 0.0, hub, sigma)
    cov = np.full((6 * len(free),) * 2, np.nan)
    if lin["pd"] and np.isfinite(lin["S"]).all():
        try:
            np.linalg.cholesky(lin["S"])
            cov = np.linalg.inv(lin["S"])
        except np.linalg.LinAlgError:
            pass
    xyz = np.where(act[:, None], X.astype(np.float32), xyz0)
    info = np.array([f_seed, f, trials, accepted, status, lam, act.sum(), (used & act[:, None]).sum()], dtype=np.float64)
    return {"cams": cur, "X": X, "xyz": xyz, "point_status": np.where(act, 0, INACTIVE).astype(np.uint8), "cov": cov,
            "info": info, "margins": margins, "huber_gap": min(gaps) if gaps else np.inf, "active": act, "used": used}
