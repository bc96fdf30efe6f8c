"""fp64 numpy restatement of the left/right label-swap decision, written from include/mvpose.h
("Left/right label swaps per camera"), not from the kernel.  Built on sync_ref's ideal pixels,
fundamental matrix and Sampson distance.

* ``cost_tables``: n, same, cross, keep, change, prior.
* ``solve``: the recursion over the 2^nv states and the backtrack, per unit.
* ``apply``: the exchange of the (x, y, conf) records and of the heatmap Gaussians.
* ``fix``: the three in a row.
"""
import numpy as np

import sync_ref


def check_args(T, J, nv, pairs, units, trunc_px=20.0, motion_trunc_px=40.0, motion_weight=1.0, swap_prior_px=2.0,
               min_conf=0.0):
    """The argument rules of the header; raises ValueError."""
    pairs = np.asarray(pairs)
    units = np.asarray(units)
    ns = len(units)
    if T < 1 or T * J >= 2 ** 31:
        raise ValueError("T")
    if not 2 <= nv <= 8:
        raise ValueError("nv")
    if not 1 <= ns <= 64 or pairs.shape != (ns, 2):
        raise ValueError("pairs")
    flat = pairs.ravel().tolist()
    if min(flat) < 0 or max(flat) >= J or len(set(flat)) != 2 * ns:
        raise ValueError("pairs")
    U = int(units.max()) + 1
    if units.min() < 0 or sorted(set(units.tolist())) != list(range(U)):
        raise ValueError("units")
    for name, v, strict in (("trunc_px", trunc_px, True), ("motion_trunc_px", motion_trunc_px, True),
                            ("motion_weight", motion_weight, False), ("swap_prior_px", swap_prior_px, False)):
        if not np.isfinite(v) or v < 0 or (strict and v == 0):
            raise ValueError(name)
    if np.isnan(min_conf):
        raise ValueError("min_conf")
    return U


def cost_tables(kpts, cams, cam_idx, pairs, units, min_conf=0.0, trunc_px=20.0, motion_trunc_px=40.0,
                motion_weight=1.0, swap_prior_px=2.0):
    """-> dict(n (T, U, nv) int32; same, cross (T, U, NP); keep, change, prior (T, U, nv) float64)."""
    kpts = np.asarray(kpts, np.float32)
    T, J = kpts.shape[:2]
    nv = len(cam_idx)
    U = check_args(T, J, nv, pairs, units, trunc_px, motion_trunc_px, motion_weight, swap_prior_px, min_conf)
    tau2 = float(np.float32(trunc_px)) ** 2
    mu2 = float(np.float32(motion_trunc_px)) ** 2
    w = float(np.float32(motion_weight))
    prior2 = float(np.float32(swap_prior_px)) ** 2
    x = sync_ref.ideal_points(kpts, cams, cam_idx, min_conf)          # (nv, T, J, 3)
    raw = np.stack([kpts[..., c] for c in cam_idx])                    # (nv, T, J, 3)
    with np.errstate(invalid="ignore"):
        usable = (np.isfinite(raw[..., 0]) & np.isfinite(raw[..., 1]) & ~np.isnan(raw[..., 2])
                  & (raw[..., 2] >= np.float32(min_conf)) & ~np.isnan(x[..., 0]))   # ... and has an ideal pixel
    q = np.stack([kpts[:, :, :2, c].astype(np.float64) for c in cam_idx])   # (nv, T, J, 2) raw pixels
    vp = [(a, b) for a in range(nv) for b in range(a + 1, nv)]
    F = [sync_ref.fundamental(cams[cam_idx[a]], cams[cam_idx[b]]) for a, b in vp]
    n = np.zeros((T, U, nv), np.int32)
    same, cross = np.zeros((T, U, len(vp))), np.zeros((T, U, len(vp)))
    keep, change = np.zeros((T, U, nv)), np.zeros((T, U, nv))

    def d2min(a, b, lim):
        return np.minimum(((a - b) ** 2).sum(-1), lim)

    for k, ((l, r), u) in enumerate(zip(np.asarray(pairs).tolist(), np.asarray(units).tolist())):
        complete = usable[:, :, l] & usable[:, :, r]                   # (nv, T)
        n[:, u, :] += complete.T
        for p, (a, b) in enumerate(vp):
            d = [sync_ref.sampson2(F[p], x[a][:, i], x[b][:, j]) for i, j in ((l, l), (r, r), (l, r), (r, l))]
            ok = complete[a] & complete[b] & np.all(np.isfinite(d), axis=0)
            d = [np.where(ok, np.minimum(np.nan_to_num(v), tau2), 0.0) for v in d]
            same[:, u, p] += d[0] + d[1]
            cross[:, u, p] += d[2] + d[3]
        for a in range(nv):
            both = complete[a, 1:] & complete[a, :-1]
            with np.errstate(invalid="ignore", over="ignore"):
                kp = d2min(q[a, 1:, l], q[a, :-1, l], mu2) + d2min(q[a, 1:, r], q[a, :-1, r], mu2)
                ch = d2min(q[a, 1:, l], q[a, :-1, r], mu2) + d2min(q[a, 1:, r], q[a, :-1, l], mu2)
            keep[1:, u, a] += np.where(both, kp, 0.0)
            change[1:, u, a] += np.where(both, ch, 0.0)
    return dict(n=n, same=same, cross=cross, keep=w * keep, change=w * change, prior=prior2 * n.astype(np.float64))


def frame_cost(same, cross, prior, nv):
    """E(t, s) of one frame and unit for all states: (2^nv,) float64, added in the stated order."""
    s = np.arange(1 << nv)
    E = np.zeros(1 << nv)
    for a in range(nv):
        E = np.where((s >> a) & 1, E + prior[a], E)
    p = 0
    for a in range(nv):
        for b in range(a + 1, nv):
            E = E + np.where(((s >> a) ^ (s >> b)) & 1, cross[p], same[p])
            p += 1
    return E


def solve(same, cross, keep, change, prior):
    """Tables (T, U, ·) -> (swap (T, U) uint8, cost (U,) float64)."""
    T, U, nv = keep.shape
    S = 1 << nv
    s = np.arange(S)
    swap = np.zeros((T, U), np.uint8)
    cost = np.zeros(U)
    for u in range(U):
        bp = np.zeros((T, S), np.uint8)
        D = frame_cost(same[0, u], cross[0, u], prior[0, u], nv)
        for t in range(1, T):
            G, flip = D, np.zeros(S, np.int64)
            for a in range(nv):
                k = G + keep[t, u, a]
                c = G[s ^ (1 << a)] + change[t, u, a]
                take = c < k
                G, flip = np.where(take, c, k), np.where(take, flip[s ^ (1 << a)] | (1 << a), flip)
            D = G + frame_cost(same[t, u], cross[t, u], prior[t, u], nv)
            bp[t] = flip
        st = int(np.argmin(D))            # the first, so the smallest, state that attains the minimum
        cost[u] = D[st]
        for t in range(T - 1, -1, -1):
            swap[t, u] = st
            st ^= int(bp[t, st])
    return swap, cost


def apply(kpts, swap, cam_idx, pairs, units, gauss=None):
    """-> (kpts with the records exchanged, gauss (T, V, J, C) likewise or None); copies."""
    out = np.array(kpts, copy=True)
    gout = None if gauss is None else np.array(gauss, copy=True)
    for (l, r), u in zip(np.asarray(pairs).tolist(), np.asarray(units).tolist()):
        for a, col in enumerate(cam_idx):
            on = np.flatnonzero((swap[:, u] >> a) & 1)
            out[on, l, :, col], out[on, r, :, col] = kpts[on, r, :, col], kpts[on, l, :, col]
            if gauss is not None:
                gout[on, col, l], gout[on, col, r] = gauss[on, col, r], gauss[on, col, l]
    return out, gout


def fix(kpts, cams, cam_idx, pairs, units, gauss=None, **kw):
    """-> (kpts_fixed, gauss_fixed, swap)."""
    t = cost_tables(kpts, cams, cam_idx, pairs, units, **kw)
    swap, _ = solve(t["same"], t["cross"], t["keep"], t["change"], t["prior"])
    fixed, gfixed = apply(kpts, swap, cam_idx, pairs, units, gauss)
    return fixed, gfixed, swap
