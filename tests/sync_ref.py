"""fp64 numpy restatement of pose-based frame synchronisation, written from include/mvpose.h
("Epipolar lag-cost scan") and from the docstrings of mvpose/sync.py, not from the kernel.

* ``undistort_f32``: OpenCV 4.9 undistortPoints (5 iterations, P = K) in fp64, rounded to f32.
* ``fundamental``: F_ab = K_b⁻ᵀ [t]ₓ R K_a⁻¹.
* ``lag_cost``: sum / cnt of the truncated squared Sampson distances per pair and lag.
* ``solve_offsets``: the per-pair rule and the global least-squares fit.
* ``shifted_case``: mvpose.synthetic keypoints of cameras whose frame t shows instant t + s_v.
"""
import numpy as np

from mvpose import synthetic as syn


def undistort_f32(u, v, K, dist):
    """(u, v) float32 arrays -> the float32 undistorted pixels (cvUndistortPointsInternal with
    R = I, P = K, 5 iterations, 5 coefficients; fp64 throughout, one rounding at the end)."""
    K = np.asarray(K, np.float64)
    k0, k1, k2, k3, k4 = np.asarray(dist, np.float64).ravel()[:5]
    u = np.asarray(u, np.float32).astype(np.float64)
    v = np.asarray(v, np.float32).astype(np.float64)
    ifx, ify = 1.0 / K[0, 0], 1.0 / K[1, 1]
    with np.errstate(all="ignore"):
        x0 = (u - K[0, 2]) * ifx
        y0 = (v - K[1, 2]) * ify
        x, y = x0.copy(), y0.copy()
        neg = np.zeros(x.shape, bool)
        for _ in range(5):
            r2 = x * x + y * y
            icdist = 1.0 / (1 + ((k4 * r2 + k1) * r2 + k0) * r2)
            neg |= icdist < 0
            dx = 2 * k2 * x * y + k3 * (r2 + 2 * x * x)
            dy = k2 * (r2 + 2 * y * y) + 2 * k3 * x * y
            x = (x0 - dx) * icdist
            y = (y0 - dy) * icdist
        x = np.where(neg, x0, x)      # OpenCV breaks out with the initial guess
        y = np.where(neg, y0, y)
        xx = K[0, 0] * x + K[0, 1] * y + K[0, 2]
        yy = K[1, 0] * x + K[1, 1] * y + K[1, 2]
        ww = 1.0 / (K[2, 0] * x + K[2, 1] * y + K[2, 2])
        return (xx * ww).astype(np.float32), (yy * ww).astype(np.float32)


def fundamental(ca, cb):
    """x_bᵀ F x_a = 0 for cameras {K, R, T}: F = K_b⁻ᵀ [t]ₓ R K_a⁻¹, R = R_b R_aᵀ, t = T_b − R T_a."""
    R = cb["R"] @ ca["R"].T
    t = cb["T"].reshape(3) - R @ ca["T"].reshape(3)
    tx = np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])
    return np.linalg.inv(cb["K"]).T @ tx @ R @ np.linalg.inv(ca["K"])


def ideal_points(kpts, cams, cam_idx, min_conf=0.0):
    """-> (NV, T, J, 3) float64 homogeneous ideal pixels, NaN rows for unusable keypoints."""
    kpts = np.asarray(kpts, np.float32)
    T, J = kpts.shape[:2]
    out = np.full((len(cam_idx), T, J, 3), np.nan)
    for i, c in enumerate(cam_idx):
        x, y, conf = kpts[:, :, 0, c], kpts[:, :, 1, c], kpts[:, :, 2, c]
        ux, uy = undistort_f32(x, y, cams[c]["K"], cams[c]["dist"])
        with np.errstate(invalid="ignore"):
            ok = np.isfinite(x) & np.isfinite(y) & ~np.isnan(conf) & (conf >= np.float32(min_conf))
        out[i, ..., 0] = np.where(ok, ux.astype(np.float64), np.nan)
        out[i, ..., 1] = np.where(ok, uy.astype(np.float64), np.nan)
        out[i, ..., 2] = np.where(ok, 1.0, np.nan)
    return out


def sampson2(F, xa, xb):
    """Squared Sampson distances of (..., 3) homogeneous points; NaN / inf where undefined."""
    with np.errstate(all="ignore"):
        la = xa @ F.T          # F x_a
        lb = xb @ F            # Fᵀ x_b
        num = (xb * la).sum(-1)
        den = la[..., 0] ** 2 + la[..., 1] ** 2 + lb[..., 0] ** 2 + lb[..., 1] ** 2
        d2 = num * num / den
        return np.where(den != 0, d2, np.nan)


def lag_cost(kpts, cams, cam_idx, max_lag, min_conf=0.0, trunc_px=20.0):
    """-> (sum (NP, 2L+1) float64, cnt (NP, 2L+1) int64, pairs)."""
    x = ideal_points(kpts, cams, cam_idx, min_conf)
    nv, T = x.shape[:2]
    L = int(max_lag)
    assert 0 <= L < T
    pairs = [(a, b) for a in range(nv) for b in range(a + 1, nv)]
    tau2 = float(trunc_px) ** 2
    s = np.zeros((len(pairs), 2 * L + 1))
    n = np.zeros((len(pairs), 2 * L + 1), np.int64)
    for p, (a, b) in enumerate(pairs):
        F = fundamental(cams[cam_idx[a]], cams[cam_idx[b]])
        for lag in range(-L, L + 1):
            lo, hi = max(0, -lag), min(T, T - lag)       # frames t of a with 0 <= t + lag < T
            d2 = sampson2(F, x[a, lo:hi], x[b, lo + lag:hi + lag])
            ok = np.isfinite(d2)
            s[p, lag + L] = np.minimum(d2[ok], tau2).sum()
            n[p, lag + L] = int(ok.sum())
    return s, n, pairs


def solve_offsets(s, n, pairs, n_views, n_terms, min_overlap=0.5, min_contrast=2.0):
    """The pair rule and the global fit -> dict(offsets: float array with NaN for cameras not
    connected to camera 0, s, lag, sub, contrast, accepted, reason)."""
    n_pairs, n_lags = s.shape
    L = (n_lags - 1) // 2
    res = {"lag": [None] * n_pairs, "sub": [np.nan] * n_pairs, "contrast": [np.nan] * n_pairs,
           "accepted": [False] * n_pairs, "reason": [""] * n_pairs}
    for p in range(n_pairs):
        lags = [k for k in range(n_lags) if n[p, k] >= min_overlap * n_terms and n[p, k] > 0]
        if not lags:
            res["reason"][p] = "overlap"
            continue
        mean = {k: s[p, k] / n[p, k] for k in lags}
        k = min(lags, key=lambda q: (mean[q], q))
        res["lag"][p] = k - L
        res["sub"][p] = float(k - L)
        if k - 1 in mean and k + 1 in mean:
            m0, m1, m2 = mean[k - 1], mean[k], mean[k + 1]
            if m0 - 2 * m1 + m2 > 0:
                res["sub"][p] = (k - L) + 0.5 * (m0 - m2) / (m0 - 2 * m1 + m2)
        res["contrast"][p] = np.median(list(mean.values())) / mean[k] if mean[k] > 0 else np.inf
        if res["contrast"][p] < min_contrast:
            res["reason"][p] = "contrast"
        elif k in (lags[0], lags[-1]):
            res["reason"][p] = "edge"
        else:
            res["accepted"][p] = True
    reach = {0}
    grown = True
    while grown:
        grown = False
        for p, (a, b) in enumerate(pairs):
            if res["accepted"][p] and (a in reach) != (b in reach):
                reach |= {a, b}
                grown = True
    sol = np.full(n_views, np.nan)
    sol[0] = 0.0
    free = sorted(reach - {0})
    if free:
        # normal equations of min Σ (s_a − s_b − sub_ab)² over the accepted pairs inside `reach`, s_0 = 0
        N = np.zeros((len(free), len(free)))
        r = np.zeros(len(free))
        for p, (a, b) in enumerate(pairs):
            if not res["accepted"][p] or a not in reach:
                continue
            for v, sign in ((a, 1.0), (b, -1.0)):
                if v == 0:
                    continue
                i = free.index(v)
                r[i] += sign * res["sub"][p]
                for w, sw in ((a, 1.0), (b, -1.0)):
                    if w != 0:
                        N[i, free.index(w)] += sign * sw
        sol[free] = np.linalg.solve(N, r)
    res["s"] = sol
    res["offsets"] = np.round(sol)
    return res


def shifted_case(T, offsets, seed=0, n_cams=4, jitter=0.0, noise_px=1.0, still=False, rig_seed=0):
    """(cams, kpts (T, 17, 3, V) float32): camera v's frame t shows the subject at instant
    t + offsets[v] (fractional offsets: poses linearly interpolated between instants)."""
    offsets = np.asarray(offsets, np.float64)
    cams = syn.make_rig(n_cams, seed=rig_seed)
    lo = int(np.floor(offsets.min()))
    n_inst = T + int(np.ceil(offsets.max())) - lo + 1
    poses = syn.make_poses(n_inst, seed=seed, jitter=jitter)
    if still:
        poses = np.repeat(poses[:1], n_inst, axis=0)
    rng = np.random.default_rng(1000 + seed)
    k = np.empty((T, syn.N_JOINTS, 3, n_cams), np.float32)
    for v, cam in enumerate(cams):
        tau = np.arange(T) + offsets[v] - lo
        i0 = np.floor(tau).astype(int)
        w = (tau - i0)[:, None, None]
        pv = (1 - w) * poses[i0] + w * poses[np.minimum(i0 + 1, n_inst - 1)]
        uv = syn.project(pv, cam) + rng.normal(0.0, noise_px, (T, syn.N_JOINTS, 2))
        k[:, :, 0, v] = uv[..., 0]
        k[:, :, 1, v] = uv[..., 1]
        k[:, :, 2, v] = rng.uniform(0.3, 1.0, (T, syn.N_JOINTS))
    return cams, k
