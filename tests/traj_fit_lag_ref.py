"""fp64 numpy restatement of the trajectory fit with sub-frame camera offsets
(mvp_trajectory_fit_lag_system / mvp_trajectory_fit_lag; the normative text is the comment in
include/mvpose.h), on traj_fit_ref's pieces: its used-view rule, its per-view terms, its dense
matrices.  View i's frame t scores Y = (1 − a_i)·X_t + a_i·X_{t+1}; with every a_i = 0 each sum here
is formed as traj_fit_ref forms it, so the two agree bit for bit.  Also the host algorithm of
sync.refine_frame_offsets, restated on this fit.  Nothing here touches the device."""
import numpy as np

import traj_fit_ref as tf
import tri_refine_ref as tr

INVALID, NOT_CONVERGED = tf.INVALID, tf.NOT_CONVERGED


def check_frac(frac, nv):
    a = np.asarray(frac, np.float64).reshape(-1)
    assert a.shape == (nv,) and np.isfinite(a).all() and (a >= 0).all() and (a < 1).all(), a
    return a


def lag_used(used, a):
    """The used set with the added rule: a view with a > 0 is not used in the last frame.
    used (T, ..., NV)."""
    used = used.copy()
    used[-1] &= ~(a > 0)
    return used


def view_terms(X, a, cams, cam_idx, used, z, W, hub):
    """One chain at the state X (T, 3), used (T, NV) (lag_used's): per view i the terms of its
    observations at their Y.  Returns rho, s2 (T, NV), H (T, NV, 3, 3), g (T, NV, 3), front (T, NV):
    exact zeros (front True) where the view is not used."""
    T, nv = used.shape
    Xn = np.concatenate([X[1:], X[-1:]])
    rho, s2 = np.zeros((T, nv)), np.zeros((T, nv))
    H, g, front = np.zeros((T, nv, 3, 3)), np.zeros((T, nv, 3)), np.ones((T, nv), bool)
    for i in range(nv):
        with np.errstate(all="ignore"):
            Y = X if a[i] == 0 else (1.0 - a[i]) * X + a[i] * Xn
        rho[:, i], s2[:, i], H[:, i], g[:, i], front[:, i] = tf.frame_terms(
            Y, cams, cam_idx[i:i + 1], used[:, i:i + 1], z[:, i:i + 1], W[:, i:i + 1], hub)
    return rho, s2, H, g, front


def node_terms(a, H, g):
    """The nodes' H̃ (T, 3, 3), g̃ (T, 3) and the pairs' C (T, 3, 3; row T-1 zero) from the views'
    terms: node t takes (1−a)²·H_i, (1−a)·g_i of frame t and a²·H_i, a·g_i of frame t−1."""
    T, nv = H.shape[:2]
    Hn, gn, C = np.zeros((T, 3, 3)), np.zeros((T, 3)), np.zeros((T, 3, 3))
    for i in range(nv):
        b = 1.0 - a[i]
        Hn += (b * b) * H[:, i]
        gn += b * g[:, i]
        if a[i] > 0:
            C += (a[i] * b) * H[:, i]
            Hn[1:] += (a[i] * a[i]) * H[:-1, i]
            gn[1:] += a[i] * g[:-1, i]
    return Hn, gn, C


def dlag_terms(X, used, H, g):
    """(NV, 2): ga = Σ_t dᵀW̃r, ha = Σ_t dᵀW̃d, d = J·(X_{t+1} − X_t), over the used (t, i), t + 1 < T."""
    D = X[1:] - X[:-1]
    u = used[:-1]
    with np.errstate(all="ignore"):
        ga = np.where(u, np.einsum("tk,tik->ti", D, g[:-1]), 0.0).sum(0)
        ha = np.where(u, np.einsum("tk,tikl,tl->ti", D, H[:-1], D), 0.0).sum(0)
    return np.stack([ga, ha], -1)


class Chain(tf.Chain):
    """One chain's problem with the offsets a (NV,): cost, linearisation and offset derivative."""

    def __init__(self, cams, cam_idx, used, z, W, hub, lam, a):
        self.a = check_frac(a, used.shape[1])
        super().__init__(cams, list(cam_idx), lag_used(used, self.a), z, W, hub, lam)

    def terms(self, X):
        return view_terms(X, self.a, self.cams, self.cam_idx, self.used, self.z, self.W, self.hub)

    def cost(self, X):
        rho, s2, _, _, front = self.terms(X)
        d = self.D3 @ X.ravel()
        f = float(rho.sum(1).sum()) + 0.5 * self.lam * float(d @ d)
        return (f if front.all() else np.inf), s2.sum(1)

    def linearise(self, X):
        """A (3T, 3T) and G (3T,)."""
        _, _, H, g, _ = self.terms(X)
        Hn, gn, C = node_terms(self.a, H, g)
        T = X.shape[0]
        A = self.lam * self.K3
        for t in range(T):
            A[3 * t:3 * t + 3, 3 * t:3 * t + 3] += Hn[t]
        if (self.a > 0).any():
            for t in range(T - 1):
                A[3 * t:3 * t + 3, 3 * t + 3:3 * t + 6] += C[t]
                A[3 * t + 3:3 * t + 6, 3 * t:3 * t + 3] += C[t].T
        return A, gn.ravel() + self.lam * (self.K3 @ X.ravel())

    def dlag(self, X):
        _, _, H, g, _ = self.terms(X)
        return dlag_terms(X, self.used, H, g)


def fit_chain(ch, seed32, max_iter, tol):
    """traj_fit_ref.fit_chain with the validity rule read at the seed's Ys.  Returns its dict."""
    T = seed32.shape[0]
    X = seed32.astype(np.float64)
    nan = {"X": X, "status": INVALID, "cost": np.array([np.nan, np.nan]), "s2": np.full(T, np.nan), "margins": [],
           "rejected": 0}
    if not np.isfinite(seed32).all():
        return nan
    front = ch.terms(X)[4]
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


def system(kpts, cams, cam_idx, frac, xyz, mask_bits=None, weights=tr.W_CONF, gauss=None, min_conf=0.0, cov_floor=1.0,
           huber_delta=0.0):
    """mvp_trajectory_fit_lag_system: H (T, P, 6), C (T, P, 6), g (T, P, 3), nviews (T, P), cost (P, 2),
    dlag (P, NV, 2)."""
    used, z, W = tf.views(kpts, cam_idx, mask_bits, weights, gauss, min_conf, cov_floor)
    T, P, nv = used.shape
    a = check_frac(frac, nv)
    used = lag_used(used, a)
    hub = float(huber_delta) if huber_delta > 0 else 0.0
    X = np.asarray(xyz, dtype=np.float32).astype(np.float64)
    H6, C6, gg = np.zeros((T, P, 6)), np.zeros((T, P, 6)), np.zeros((T, P, 3))
    c, dlag = np.zeros((T, P)), np.zeros((P, nv, 2))
    idx = [0, 1, 2, 4, 5, 8]
    for p in range(P):
        rho, _, H, g, front = view_terms(X[:, p], a, cams, list(cam_idx), used[:, p], z[:, p], W[:, p], hub)
        Hn, gn, C = node_terms(a, H, g)
        H6[:, p], C6[:, p], gg[:, p] = Hn.reshape(T, 9)[:, idx], C.reshape(T, 9)[:, idx], gn
        with np.errstate(all="ignore"):
            c[:, p] = np.where(front.all(1), rho.sum(1), np.inf)
        dlag[p] = dlag_terms(X[:, p], used[:, p], H, g)
    with np.errstate(all="ignore"):
        d = X[2:] - 2 * X[1:-1] + X[:-2] if T > 2 else np.zeros((0, P, 3))
        cost = np.stack([c.sum(0), 0.5 * (d * d).sum((0, 2))], -1)
    return H6, C6, gg, used.sum(-1).astype(np.uint8), cost, dlag


def fit(kpts, cams, cam_idx, frac, xyz0, mask_bits=None, weights=tr.W_CONF, gauss=None, min_conf=0.0, cov_floor=1.0,
        huber_delta=0.0, lambda_smooth=1.0, max_iter=30, tol=1e-6):
    """mvp_trajectory_fit_lag.  Returns traj_fit_ref.fit's dict, plus dlag (P, NV, 2), NaN for an invalid
    chain."""
    used, z, W = tf.views(kpts, cam_idx, mask_bits, weights, gauss, min_conf, cov_floor)
    T, P, nv = used.shape
    a = check_frac(frac, nv)
    hub = float(huber_delta) if huber_delta > 0 else 0.0
    xyz0 = np.asarray(xyz0, dtype=np.float32)
    X = np.zeros((T, P, 3))
    xyz = xyz0.copy()
    resid = np.full((T, P), np.nan, np.float32)
    cost = np.full((P, 2), np.nan)
    status = np.zeros(P, np.uint8)
    rejected = np.zeros(P, np.int64)
    dlag = np.full((P, nv, 2), np.nan)
    margins = []
    for p in range(P):
        ch = Chain(cams, cam_idx, used[:, p], z[:, p], W[:, p], hub, float(lambda_smooth), a)
        r = fit_chain(ch, xyz0[:, p], max_iter, tol)
        X[:, p], status[p], cost[p], rejected[p] = r["X"], r["status"], r["cost"], r["rejected"]
        margins += r["margins"]
        if r["status"] != INVALID:
            xyz[:, p] = r["X"].astype(np.float32)
            resid[:, p] = np.where(ch.used.sum(1) > 0, r["s2"], np.nan).astype(np.float32)
            dlag[p] = ch.dlag(r["X"])
    return {"X": X, "xyz": xyz, "resid": resid, "nviews": lag_used(used, a).sum(-1).astype(np.uint8), "cost": cost,
            "status": status, "margins": margins, "rejected": rejected, "dlag": dlag}


# ------------------------------------------------------------------ the offsets from fits alone
def newton_offsets(reduced_gradient, s0, rounds=4, h=0.02, stop=0.01):
    """The host algorithm of sync.refine_frame_offsets on any fit: reduced_gradient(s) -> (ga (NV,),
    cost) of a fit with the offsets s (split, aligned and fitted by the caller), ga summed over the
    valid chains in ascending order.  View 0 stays; per round a Newton step on ga of the others,
    its Jacobian from central differences of ga between 2·(NV−1) further fits at s_j ± h, the step
    limited to half a frame.  Stops after `rounds` rounds or on a step below `stop` frames.
    Returns (s, info): info["cost"] every round's cost and the final one, info["step"] the steps."""
    s = np.array(s0, np.float64)
    nv = s.size
    costs, steps = [], []
    for _ in range(rounds):
        g0, f0 = reduced_gradient(s)
        costs.append(f0)
        Jm = np.zeros((nv - 1, nv - 1))
        for j in range(1, nv):
            sp, sm = s.copy(), s.copy()
            sp[j] += h
            sm[j] -= h
            Jm[:, j - 1] = (reduced_gradient(sp)[0][1:] - reduced_gradient(sm)[0][1:]) / (2 * h)
        step = -np.linalg.solve(Jm, g0[1:])
        step = np.clip(step, -0.5, 0.5)
        s[1:] += step
        steps.append(float(np.abs(step).max()))
        if steps[-1] < stop:
            break
    costs.append(reduced_gradient(s)[1])
    return s, {"cost": costs, "step": steps}
