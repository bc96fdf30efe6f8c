"""fp64 numpy restatement of the trajectory fit (mvp_trajectory_fit_system / mvp_trajectory_fit; the
normative text is the comment in include/mvpose.h): synthetic.project as the forward model, analytic
Jacobians, per chain a dense 3T x 3T matrix and the Levenberg-Marquardt loop as stated.  The
used-view / observation / weight rule is tri_refine_ref.views, rho and omega are
ba_ref.residual_terms (the text says they are mvp_triangulate_refine's and mvp_bundle_adjust's).
Nothing here touches the device."""
import numpy as np

import ba_ref
import tri_refine_ref as tr

INVALID, NOT_CONVERGED = 0x80, 0x40


def views(kpts, cam_idx, mask_bits, weights, gauss, min_conf, cov_floor):
    """used (T, P, NV) bool, z (T, P, NV, 2), W (T, P, NV, 2, 2) of kpts (T, P, 3, V)."""
    kpts = np.asarray(kpts, dtype=np.float32)
    T, P, _, V = kpts.shape
    bits = None if mask_bits is None else np.asarray(mask_bits).reshape(-1)
    used, z, W = tr.views(kpts.reshape(-1, 3, V), cam_idx, bits, weights, gauss, min_conf, cov_floor)
    nv = len(cam_idx)
    return used.reshape(T, P, nv), z.reshape(T, P, nv, 2), W.reshape(T, P, nv, 2, 2)


def second_difference(T):
    """D₂, (T-2) x T."""
    D = np.zeros((max(T - 2, 0), T))
    for s in range(T - 2):
        D[s, s:s + 3] = (1.0, -2.0, 1.0)
    return D


def frame_terms(X, cams, cam_idx, used, z, W, hub):
    """At the points X (n, 3) with used (n, NV), z, W: rho (n,) = Σ_used rho, s2 (n,) = Σ_used s²,
    H (n, 3, 3) = Σ Jᵀ W̃ J, g (n, 3) = Σ Jᵀ W̃ r, front (n,): every used view has P_z > 0.  An unused
    view contributes exact zeros whatever X is."""
    n = X.shape[0]
    rho, s2 = np.zeros(n), np.zeros(n)
    H, g = np.zeros((n, 3, 3)), np.zeros((n, 3))
    front = np.ones(n, bool)
    for i, col in enumerate(cam_idx):
        cam = cams[col]
        u = used[:, i]
        r, s, om, rh, Pz = ba_ref.residual_terms(X, cam, z[:, i], W[:, i], hub)
        J, _ = tr.jacobian(X, cam)
        with np.errstate(all="ignore"):
            Wt = om[:, None, None] * W[:, i]
            Hi = np.einsum("nak,nab,nbl->nkl", J, Wt, J)
            gi = np.einsum("nak,nab,nb->nk", J, Wt, r)
            front &= ~u | (Pz > 0)
            rho += np.where(u, rh, 0.0)
            s2 += np.where(u, s * s, 0.0)
            H += np.where(u[:, None, None], Hi, 0.0)
            g += np.where(u[:, None], gi, 0.0)
    return rho, s2, H, g, front


def system(kpts, cams, cam_idx, xyz, mask_bits=None, weights=tr.W_CONF, gauss=None, min_conf=0.0, cov_floor=1.0,
           huber_delta=0.0):
    """mvp_trajectory_fit_system: H (T, P, 6), g (T, P, 3), nviews (T, P), cost (P, 2)."""
    used, z, W = views(kpts, cam_idx, mask_bits, weights, gauss, min_conf, cov_floor)
    T, P, nv = used.shape
    hub = float(huber_delta) if huber_delta > 0 else 0.0
    X = np.asarray(xyz, dtype=np.float32).astype(np.float64)
    rho, _, H, g, front = frame_terms(X.reshape(-1, 3), cams, cam_idx, used.reshape(-1, nv), z.reshape(-1, nv, 2),
                                      W.reshape(-1, nv, 2, 2), hub)
    H6 = H.reshape(T, P, 9)[..., [0, 1, 2, 4, 5, 8]]
    with np.errstate(all="ignore"):
        c = np.where(front, rho, np.inf).reshape(T, P)
        d = X[2:] - 2 * X[1:-1] + X[:-2] if T > 2 else np.zeros((0, P, 3))
        cost = np.stack([c.sum(0), 0.5 * (d * d).sum((0, 2))], -1)
    return H6, g.reshape(T, P, 3), used.sum(-1).astype(np.uint8), cost


class Chain:
    """One chain's problem: cost and linearisation at a state X (T, 3)."""

    def __init__(self, cams, cam_idx, used, z, W, hub, lam):
        self.cams, self.cam_idx, self.used, self.z, self.W, self.hub, self.lam = cams, cam_idx, used, z, W, hub, lam
        T = used.shape[0]
        D = second_difference(T)
        self.K3 = np.kron(D.T @ D, np.eye(3))
        self.D3 = np.kron(D, np.eye(3))

    def cost(self, X):
        rho, s2, _, _, front = frame_terms(X, self.cams, self.cam_idx, self.used, self.z, self.W, self.hub)
        d = self.D3 @ X.ravel()
        f = float(rho.sum()) + 0.5 * self.lam * float(d @ d)
        return (f if front.all() else np.inf), s2

    def linearise(self, X):
        """A (3T, 3T) and G (3T,)."""
        _, _, H, g, _ = frame_terms(X, self.cams, self.cam_idx, self.used, self.z, self.W, self.hub)
        T = X.shape[0]
        A = self.lam * self.K3
        for t in range(T):
            A[3 * t:3 * t + 3, 3 * t:3 * t + 3] += H[t]
        return A, g.ravel() + self.lam * (self.K3 @ X.ravel())


def fit_chain(ch, seed32, max_iter, tol):
    """The Levenberg-Marquardt loop of one chain.  Returns dict: X (T, 3) f64, status, cost (2,),
    s2 (T,), margins, rejected (trials that were not accepted)."""
    T = seed32.shape[0]
    X = seed32.astype(np.float64)
    nan = {"X": X, "status": INVALID, "cost": np.array([np.nan, np.nan]), "s2": np.full(T, np.nan), "margins": [],
           "rejected": 0}
    if not np.isfinite(seed32).all():
        return nan
    _, _, _, _, front = frame_terms(X, ch.cams, ch.cam_idx, ch.used, ch.z, ch.W, ch.hub)
    if not front.all() or (ch.used.sum(1) >= 2).sum() < 2:
        return nan
    f, s2 = ch.cost(X)
    if not np.isfinite(f):
        return nan
    f_seed, mu, trials, conv, margins, rejected = f, 1e-3, 0, False, [], 0
    while trials < max_iter:
        A, G = ch.linearise(X)
        M = A + mu * np.diag(np.diag(A))
        ok = bool(np.isfinite(M).all())
        if ok:
            try:
                L = np.linalg.cholesky(M)
                delta = np.linalg.solve(L.T, np.linalg.solve(L, -G))
            except np.linalg.LinAlgError:
                ok = False
        trials += 1
        ft = np.inf
        if ok:
            Xt = X + delta.reshape(T, 3)
            ft, s2t = ch.cost(Xt)
            if np.isfinite(ft):
                margins.append(abs(ft - f) / abs(f))
        if ok and np.isfinite(ft) and ft <= f:
            conv = (f - ft) <= tol * f
            margins.append(abs((f - ft) - tol * f) / abs(f))
            X, f, s2 = Xt, ft, s2t
            mu = max(mu * 0.1, 1e-12)
            if conv:
                break
        else:
            mu = mu * 10.0
            rejected += 1
            if mu > 1e12:
                break
    return {"X": X, "status": trials | (0 if conv else NOT_CONVERGED), "cost": np.array([f_seed, f]), "s2": s2,
            "margins": margins, "rejected": rejected}


def fit(kpts, cams, cam_idx, xyz0, mask_bits=None, weights=tr.W_CONF, gauss=None, min_conf=0.0, cov_floor=1.0,
        huber_delta=0.0, lambda_smooth=1.0, max_iter=30, tol=1e-6):
    """mvp_trajectory_fit on kpts (T, P, 3, V) f32 from the seed xyz0 (T, P, 3) f32.  Returns dict: X
    (T, P, 3) f64, xyz (T, P, 3) f32, resid (T, P) f32, nviews (T, P), cost (P, 2), status (P,),
    margins (the relative margins of every accept and convergence comparison), rejected (P,)."""
    used, z, W = views(kpts, cam_idx, mask_bits, weights, gauss, min_conf, cov_floor)
    T, P, nv = used.shape
    hub = float(huber_delta) if huber_delta > 0 else 0.0
    xyz0 = np.asarray(xyz0, dtype=np.float32)
    X = np.zeros((T, P, 3))
    xyz = xyz0.copy()
    resid = np.full((T, P), np.nan, np.float32)
    cost = np.full((P, 2), np.nan)
    status = np.zeros(P, np.uint8)
    rejected = np.zeros(P, np.int64)
    margins = []
    for p in range(P):
        ch = Chain(cams, cam_idx, used[:, p], z[:, p], W[:, p], hub, float(lambda_smooth))
        r = fit_chain(ch, xyz0[:, p], max_iter, tol)
        X[:, p], status[p], cost[p], rejected[p] = r["X"], r["status"], r["cost"], r["rejected"]
        margins += r["margins"]
        if r["status"] != INVALID:
            xyz[:, p] = r["X"].astype(np.float32)
            resid[:, p] = np.where(used[:, p].sum(1) > 0, r["s2"], np.nan).astype(np.float32)
    return {"X": X, "xyz": xyz, "resid": resid, "nviews": used.sum(-1).astype(np.uint8), "cost": cost,
            "status": status, "margins": margins, "rejected": rejected}
