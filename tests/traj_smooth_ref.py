"""fp64 numpy restatement of mvp_trajectory_smooth, written from the contract in include/mvpose.h
(the reference project has no counterpart).

Per chain p: frame (t, p) is observed when its coordinates are finite, valid[t][p] != 0 (where
given) and, where a covariance is given, its six numbers are finite and S = cov + cov_floor·I has
three Cholesky pivots > 0.  W_t = S⁻¹ (I / sigma0² without cov) on observed frames, 0 elsewhere.
The output solves (blockdiag(W) + λ·(D₂ᵀD₂ ⊗ I₃)) X = blockdiag(W) z.  A chain with fewer than 2
observed frames, or with a pivot of the factorisation not > 0, fails: input bits out, NaN resid,
status 0x80.

solve_dense builds the matrix and calls np.linalg.solve; solve_banded is a sequential block-
pentadiagonal LDLᵀ solve vectorised over the chains, for long T.  Both return a Result.  Also here:
the Huber reweighting loop and the max_gap mask of mvpose.refine.smooth_trajectory."""
from collections import namedtuple

import numpy as np

Result = namedtuple("Result", "xyz resid observed status x64")
# xyz (T, P, 3) float32; resid (T, P) float64 (NaN where unobserved / failed); observed (T, P) bool;
# status (P,) uint8; x64 (T, P, 3) the fp64 solution before rounding (NaN for failed chains)


def _cov6(cov):
    cov = np.asarray(cov)
    if cov.shape[-2:] == (3, 3):
        return np.stack([cov[..., 0, 0], cov[..., 0, 1], cov[..., 0, 2], cov[..., 1, 1], cov[..., 1, 2],
                         cov[..., 2, 2]], -1)
    return cov


def weights(xyz, cov=None, valid=None, sigma0=1.0, cov_floor=0.0):
    """-> W (T, P, 3, 3) float64, z (T, P, 3) float64 (0 where unobserved), observed (T, P) bool."""
    xyz = np.asarray(xyz, np.float32)
    T, P = xyz.shape[:2]
    obs = np.isfinite(xyz).all(-1)
    if valid is not None:
        obs &= np.asarray(valid) != 0
    W = np.zeros((T, P, 3, 3))
    if cov is not None:
        c = _cov6(cov).astype(np.float32)
        obs &= np.isfinite(c).all(-1)
        s = c.astype(np.float64)
        fl = float(np.float32(cov_floor))
        with np.errstate(all="ignore"):
            sxx, sxy, sxz, syy, syz, szz = (s[..., 0] + fl, s[..., 1], s[..., 2], s[..., 3] + fl, s[..., 4],
                                            s[..., 5] + fl)
            d0 = sxx
            l10, l20 = sxy / np.sqrt(d0), sxz / np.sqrt(d0)
            d1 = syy - l10 * l10
            l21 = (syz - l20 * l10) / np.sqrt(d1)
            d2 = szz - l20 * l20 - l21 * l21
            obs &= (d0 > 0) & (d1 > 0) & (d2 > 0)
        S = np.stack([np.stack([sxx, sxy, sxz], -1), np.stack([sxy, syy, syz], -1), np.stack([sxz, syz, szz], -1)], -2)
        W[obs] = np.linalg.inv(S[obs])
    else:
        W[obs] = np.eye(3) / float(np.float32(sigma0)) ** 2
    z = np.where(obs[..., None], xyz.astype(np.float64), 0.0)
    return W, z, obs


def _finish(xyz, W, z, obs, X, failed):
    xyz = np.asarray(xyz, np.float32)
    d = X - z
    resid = np.einsum("tpi,tpij,tpj->tp", d, W, d)
    resid[~obs] = np.nan
    resid[:, failed] = np.nan
    out = X.astype(np.float32)
    out[:, failed] = xyz[:, failed]
    x64 = X.copy()
    x64[:, failed] = np.nan
    return Result(out, resid, obs, np.where(failed, 0x80, 0).astype(np.uint8), x64)


def solve_dense(xyz, cov=None, valid=None, lambda_smooth=1.0, sigma0=1.0, cov_floor=0.0):
    W, z, obs = weights(xyz, cov, valid, sigma0, cov_floor)
    T, P = obs.shape
    D2 = np.zeros((max(T - 2, 0), T))
    for r in range(T - 2):
        D2[r, r:r + 3] = (1.0, -2.0, 1.0)
    K = np.kron(D2.T @ D2, np.eye(3)) * float(lambda_smooth)
    X = np.zeros((T, P, 3))
    failed = obs.sum(0) < 2
    for p in range(P):
        if failed[p]:
            continue
        A = K.copy()
        for t in range(T):
            A[3 * t:3 * t + 3, 3 * t:3 * t + 3] += W[t, p]
        b = np.einsum("tij,tj->ti", W[:, p], z[:, p]).reshape(-1)
        try:
            np.linalg.cholesky(A)
        except np.linalg.LinAlgError:
            failed[p] = True
            continue
        X[:, p] = np.linalg.solve(A, b).reshape(T, 3)
    return _finish(xyz, W, z, obs, X, failed)


def _pivots_ok(D):
    with np.errstate(all="ignore"):
        d0 = D[:, 0, 0]
        l10, l20 = D[:, 1, 0] / np.sqrt(d0), D[:, 2, 0] / np.sqrt(d0)
        d1 = D[:, 1, 1] - l10 * l10
        l21 = (D[:, 2, 1] - l20 * l10) / np.sqrt(d1)
        d2 = D[:, 2, 2] - l20 * l20 - l21 * l21
        return (d0 > 0) & (d1 > 0) & (d2 > 0)


def solve_banded(xyz, cov=None, valid=None, lambda_smooth=1.0, sigma0=1.0, cov_floor=0.0):
    W, z, obs = weights(xyz, cov, valid, sigma0, cov_floor)
    T, P = obs.shape
    lam = float(lambda_smooth)
    kd, k1, k2 = np.zeros(T), np.zeros(T), np.zeros(T)     # K[t][t], K[t][t+1], K[t][t+2]
    if T >= 3:
        kd[:-2] += 1
        kd[1:-1] += 4
        kd[2:] += 1
        k1[:-2] += -2
        k1[1:-1] += -2
        k2[:-2] += 1
    failed = obs.sum(0) < 2
    eye = np.eye(3)
    A = W + lam * kd[:, None, None, None] * eye
    A[:, failed] = eye            # keeps the batch solvable; these chains return their input
    b = np.einsum("tpij,tpj->tpi", W, z)
    Dinv = np.zeros((T, P, 3, 3))
    L1 = np.zeros((T, P, 3, 3))
    L2 = np.zeros((T, P, 3, 3))
    y = np.zeros((T, P, 3))
    Dm = np.zeros((T, P, 3, 3))
    for t in range(T):
        D = A[t].copy()
        yt = b[t].copy()
        if t >= 2:
            L2[t] = (lam * k2[t - 2]) * Dinv[t - 2]
        if t >= 1:
            E = (lam * k1[t - 1]) * eye
            if t >= 2:
                E = E - L2[t] @ Dm[t - 2] @ L1[t - 1].transpose(0, 2, 1)
            L1[t] = E @ Dinv[t - 1]
            D -= L1[t] @ Dm[t - 1] @ L1[t].transpose(0, 2, 1)
            yt -= np.einsum("pij,pj->pi", L1[t], y[t - 1])
        if t >= 2:
            D -= L2[t] @ Dm[t - 2] @ L2[t].transpose(0, 2, 1)
            yt -= np.einsum("pij,pj->pi", L2[t], y[t - 2])
        D = 0.5 * (D + D.transpose(0, 2, 1))
        bad = ~_pivots_ok(D) & ~failed
        if bad.any():
            failed = failed | bad
        D[failed] = eye
        Dm[t] = D
        Dinv[t] = np.linalg.inv(D)
        y[t] = yt
    X = np.zeros((T, P, 3))
    for t in range(T - 1, -1, -1):
        xt = np.einsum("pij,pj->pi", Dinv[t], y[t])
        if t + 1 < T:
            xt -= np.einsum("pji,pj->pi", L1[t + 1], X[t + 1])
        if t + 2 < T:
            xt -= np.einsum("pji,pj->pi", L2[t + 2], X[t + 2])
        X[t] = xt
    return _finish(xyz, W, z, obs, X, failed)


def gap_mask(observed, max_gap):
    """(T, P) bool: frames inside a run of unobserved frames longer than max_gap; leading and
    trailing runs count."""
    observed = np.asarray(observed, bool)
    T, P = observed.shape
    mask = np.zeros((T, P), bool)
    for p in range(P):
        t = 0
        while t < T:
            if observed[t, p]:
                t += 1
                continue
            e = t
            while e < T and not observed[e, p]:
                e += 1
            if e - t > max_gap:
                mask[t:e, p] = True
            t = e
    return mask


def smooth_trajectory(points, cov=None, status=None, lambda_smooth=1.0, sigma0=1.0, cov_floor=0.0, robust_k=None,
                      robust_iters=3, max_gap=None, solver=solve_banded):
    """mvpose.refine.smooth_trajectory restated: -> (points (T, P, 3) float32, Result of the last
    solve with resid against the original weights).  The loop's float32 steps are the device
    path's: the covariance that is scaled is float32(cov + cov_floor·I) or float32(sigma0)²·I, the
    scale max(1, sqrt(resid·scale) / robust_k) is formed in float32 from the float32 resid."""
    points = np.asarray(points, np.float32)
    T, P = points.shape[:2]
    valid = None if status is None else (np.asarray(status).astype(np.int32) & 0x80) == 0
    kw = dict(lambda_smooth=lambda_smooth, sigma0=sigma0)
    diag = np.array([1, 0, 0, 1, 0, 1], np.float32)
    if robust_k is None:
        res = solver(points, cov, valid, cov_floor=cov_floor, **kw)
        resid = res.resid
    else:
        if cov is not None:
            base = _cov6(cov).astype(np.float32) + np.float32(cov_floor) * diag
            res = solver(points, base, valid, cov_floor=0.0, **kw)
        else:
            base = np.broadcast_to(np.float32(sigma0) ** 2 * diag, (T, P, 6)).astype(np.float32)
            res = solver(points, None, valid, cov_floor=0.0, **kw)
        scale = np.ones((T, P), np.float32)
        k = np.float32(robust_k)
        for _ in range(int(robust_iters)):
            with np.errstate(invalid="ignore"):
                d = np.sqrt(res.resid.astype(np.float32) * scale)
                scale = np.where(d > k, d / k, np.float32(1)).astype(np.float32)
            res = solver(points, base * scale[..., None], valid, cov_floor=0.0, **kw)
        resid = res.resid.astype(np.float32) * scale
    out = res.xyz.copy()
    if max_gap is not None:
        out[gap_mask(res.observed, max_gap)] = np.nan
    return out, res._replace(resid=resid)


def make_case(T, P, seed=0, knock=0.2, long_gap=None, sigma=(0.05, 2.0)):
    """The GPU tests' input recipe: ground truth (100 + 50 sin(t/9), 200 + 30 cos(t/13),
    900 + 0.2 t) plus a per-chain offset, noise from a random rotation with per-axis σ in
    `sigma`, the true covariances rounded to float32 and symmetrised, a fraction `knock` of the
    frames knocked out (NaN xyz / NaN covariance / a covariance with a negative eigenvalue /
    valid = 0, a quarter each), and in chain 0 one gap of long_gap frames (valid = 0).
    -> dict(truth (T, P, 3) float64, xyz float32, cov (T, P, 3, 3) float32, valid (T, P) uint8)."""
    rng = np.random.default_rng(seed)
    t = np.arange(T, dtype=np.float64)
    truth = np.stack([100 + 50 * np.sin(t / 9), 200 + 30 * np.cos(t / 13), 900 + 0.2 * t], -1)[:, None, :]
    truth = truth + rng.uniform(-20, 20, (1, P, 3))
    if 0.2 * T > 80:    # long recordings: centre z on 0 (part of the per-chain offset) so that |coordinates| < 1024
        truth[..., 2] -= 900 + 0.1 * T
    Q, _ = np.linalg.qr(rng.normal(size=(T, P, 3, 3)))
    sig = rng.uniform(sigma[0], sigma[1], (T, P, 3))
    cov = np.einsum("tpij,tpj,tpkj->tpik", Q, sig ** 2, Q)
    noise = np.einsum("tpij,tpj->tpi", Q, sig * rng.normal(size=(T, P, 3)))
    xyz = (truth + noise).astype(np.float32)
    cov = cov.astype(np.float32)
    cov = ((cov + cov.transpose(0, 1, 3, 2)) * np.float32(0.5)).astype(np.float32)
    valid = np.ones((T, P), np.uint8)
    u = rng.uniform(size=(T, P))
    kind = rng.integers(0, 4, (T, P))
    ko = u < knock
    xyz[ko & (kind == 0), 1] = np.nan
    cov[ko & (kind == 1), 0, 2] = np.nan
    neg = ko & (kind == 2)
    cov[neg] = (cov[neg] - np.float32(2.0) * np.trace(cov[neg], axis1=-2, axis2=-1)[:, None, None]
                * np.eye(3, dtype=np.float32))
    valid[ko & (kind == 3)] = 0
    if long_gap is not None and T > long_gap + 4:
        s = min(3, T - long_gap - 2)
        valid[s:s + long_gap, 0] = 0
    return {"truth": truth, "xyz": xyz, "cov": cov, "valid": valid}
