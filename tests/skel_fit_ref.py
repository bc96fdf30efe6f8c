"""fp64 numpy restatement of the skeleton fit (mvp_skeleton_fit_system / mvp_skeleton_fit; the
normative text is the comment in include/mvpose.h): the trajectory fit's restatement per chain
(traj_fit_ref.Chain: synthetic.project as the forward model, tri_refine_ref's view rule,
ba_ref's rho and omega), the bone terms as stated, per chain a dense 3T x 3T matrix, and the
Levenberg-Marquardt loop per group.  Nothing here touches the device."""
import numpy as np

import traj_fit_ref as tf
import tri_refine_ref as tr

INVALID, NOT_CONVERGED = tf.INVALID, tf.NOT_CONVERGED


def live_length(L):
    """A length is live when it is finite and > 0."""
    L = np.asarray(L, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.isfinite(L) & (L > 0)


def bone_terms(X, pairs, L, live, beta):
    """The bone terms of one group at X (T, J, 3) over the segments s with live[s]: half (float) =
    ½ Σ_t Σ_s (r − L)²; g (T, J, 3): β·(r − L)·n at end b, its negative at end a; H (T, J, 3, 3):
    2β·[n nᵀ + max(0, 1 − L/r)·(I − n nᵀ)] at both ends; r (T, n_seg) (NaN for a segment that is
    not live).  A term with r == 0 has no gradient and no curvature."""
    T, J, _ = X.shape
    g, H = np.zeros((T, J, 3)), np.zeros((T, J, 3, 3))
    r_all = np.full((T, len(pairs)), np.nan)
    half = 0.0
    eye = np.eye(3)
    for s, (a, b) in enumerate(pairs):
        if not live[s]:
            continue
        with np.errstate(all="ignore"):
            d = X[:, b] - X[:, a]
            r = np.sqrt((d * d).sum(-1))
            e = r - L[s]
            half += 0.5 * float((e * e).sum())
            nz = r != 0.0
            n = d / np.where(nz, r, 1.0)[:, None]
            nn = n[:, :, None] * n[:, None, :]
            w = np.maximum(0.0, 1.0 - L[s] / np.where(nz, r, 1.0))
            blk = np.where(nz[:, None, None], 2.0 * beta * (nn + w[:, None, None] * (eye - nn)), 0.0)
            gb = np.where(nz[:, None], beta * e[:, None] * n, 0.0)
        g[:, b] += gb
        g[:, a] -= gb
        H[:, a] += blk
        H[:, b] += blk
        r_all[:, s] = r
    return half, g, H, r_all


def system(kpts, cams, cam_idx, xyz, J, pairs, lengths, lambda_bone, **kw):
    """mvp_skeleton_fit_system: H (T, P, 6), g (T, P, 3), nviews (T, P), cost (G, 3)."""
    H6, g, nviews, cost_p = tf.system(kpts, cams, cam_idx, xyz, **kw)
    T, P, _ = g.shape
    G = P // J
    L = np.asarray(lengths, dtype=np.float32).astype(np.float64).reshape(G, -1)
    X = np.asarray(xyz, dtype=np.float32).astype(np.float64).reshape(T, G, J, 3)
    H6, g = H6.reshape(T, G, J, 6).copy(), g.reshape(T, G, J, 3).copy()
    cost = np.zeros((G, 3))
    with np.errstate(all="ignore"):
        for gi in range(G):
            half, gb, Hb, _ = bone_terms(X[:, gi], pairs, L[gi], live_length(L[gi]), lambda_bone)
            g[:, gi] += gb
            H6[:, gi] += Hb.reshape(T, J, 9)[..., [0, 1, 2, 4, 5, 8]]
            cp = cost_p[gi * J:(gi + 1) * J]
            cost[gi] = (cp[:, 0].sum(), cp[:, 1].sum(), half)
    return H6.reshape(T, P, 6), g.reshape(T, P, 3), nviews, cost


class Group:
    """One person's problem: chains[j] is the joint's traj_fit_ref.Chain, or None for an invalid
    chain; a segment is live when its length is and both its chains are valid."""

    def __init__(self, chains, pairs, L, beta):
        self.chains, self.pairs, self.L, self.beta = chains, [tuple(int(v) for v in p) for p in pairs], L, float(beta)
        ok = live_length(L) if len(self.pairs) else np.zeros(0, bool)
        self.live = np.array([bool(ok[s]) and chains[a] is not None and chains[b] is not None
                              for s, (a, b) in enumerate(self.pairs)], bool)
        self.valid = [j for j, c in enumerate(chains) if c is not None]

    def cost(self, X):
        """f_g, its bone part (β applied), s2 (T, J) (NaN columns for invalid chains), r (T, n_seg)."""
        T, J, _ = X.shape
        s2 = np.full((T, J), np.nan)
        f = 0.0
        for j in self.valid:
            fj, s2[:, j] = self.chains[j].cost(X[:, j])
            f += fj
        half, _, _, r = bone_terms(X, self.pairs, self.L, self.live, self.beta)
        return f + self.beta * half, self.beta * half, s2, r

    def linearise(self, X):
        """{j: (A_j (3T, 3T), G_j (3T,))} over the valid chains."""
        T = X.shape[0]
        _, gb, Hb, _ = bone_terms(X, self.pairs, self.L, self.live, self.beta)
        out = {}
        for j in self.valid:
            A, Gj = self.chains[j].linearise(X[:, j])
            for t in range(T):
                A[3 * t:3 * t + 3, 3 * t:3 * t + 3] += Hb[t, j]
            out[j] = (A, Gj + gb[:, j].ravel())
        return out

    def dense(self, X):
        """The group's whole matrix (3TJ, 3TJ) and gradient (3TJ,), unknowns ordered chain by chain
        (chain j's block at 3T·j); invalid chains leave zeros."""
        T, J, _ = X.shape
        M, G = np.zeros((3 * T * J, 3 * T * J)), np.zeros(3 * T * J)
        for j, (A, Gj) in self.linearise(X).items():
            M[3 * T * j:3 * T * (j + 1), 3 * T * j:3 * T * (j + 1)] = A
            G[3 * T * j:3 * T * (j + 1)] = Gj
        return M, G


def fit_group(gr, seed32, max_iter, tol):
    """The Levenberg-Marquardt loop of one group from seed32 (T, J, 3) f32.  Returns dict: X (T, J, 3)
    f64, status, cost (4,), s2 (T, J), r (T, n_seg) at the result, margins, rejected, r_seen: every
    r / L of a live segment at every state and trial the loop evaluated."""
    T, J, _ = seed32.shape
    X = seed32.astype(np.float64)
    nan = {"X": X, "status": INVALID, "cost": np.full(4, np.nan), "s2": np.full((T, J), np.nan),
           "r": np.full((T, len(gr.pairs)), np.nan), "margins": [], "rejected": 0, "r_seen": []}
    if not gr.valid:
        return nan
    f, fb, s2, r = gr.cost(X)
    if not np.isfinite(f):
        return nan
    r_seen = [r[:, gr.live] / gr.L[gr.live]]
    f_seed, b_seed, mu, trials, conv, margins, rejected = f, fb, 1e-3, 0, False, [], 0
    while trials < max_iter:
        lin = gr.linearise(X)
        ok = True
        Xt = X.copy()
        for j, (A, G) in lin.items():
            M = A + mu * np.diag(np.diag(A))
            if not np.isfinite(M).all():
                ok = False
                break
            try:
                Lc = np.linalg.cholesky(M)
            except np.linalg.LinAlgError:
                ok = False
                break
            Xt[:, j] = X[:, j] + np.linalg.solve(Lc.T, np.linalg.solve(Lc, -G)).reshape(T, 3)
        trials += 1
        ft = np.inf
        if ok:
            ft, fbt, s2t, rt = gr.cost(Xt)
            if np.isfinite(ft):
                margins.append(abs(ft - f) / abs(f))
                r_seen.append(rt[:, gr.live] / gr.L[gr.live])
        if ok and np.isfinite(ft) and ft <= f:
            conv = (f - ft) <= tol * f
            margins.append(abs((f - ft) - tol * f) / abs(f))
            X, f, fb, s2, r = Xt, ft, fbt, s2t, rt
            mu = max(mu * 0.1, 1e-12)
            if conv:
                break
        else:
            mu = mu * 10.0
            rejected += 1
            if mu > 1e12:
                break
    return {"X": X, "status": trials | (0 if conv else NOT_CONVERGED), "cost": np.array([f_seed, f, b_seed, fb]),
            "s2": s2, "r": r, "margins": margins, "rejected": rejected, "r_seen": r_seen}


def chain_is_valid(ch, seed32):
    """The seed finite in every frame, in front of every used view, and at least 2 frames with at
    least 2 used views."""
    if not np.isfinite(seed32).all():
        return False
    _, _, _, _, front = tf.frame_terms(seed32.astype(np.float64), ch.cams, ch.cam_idx, ch.used, ch.z, ch.W, ch.hub)
    return bool(front.all()) and int((ch.used.sum(1) >= 2).sum()) >= 2


def fit(kpts, cams, cam_idx, xyz0, J, pairs, lengths, lambda_bone=1.0, mask_bits=None, weights=tr.W_CONF, gauss=None,
        min_conf=0.0, cov_floor=1.0, huber_delta=0.0, lambda_smooth=1.0, max_iter=30, tol=1e-6):
    """mvp_skeleton_fit on kpts (T, P, 3, V) f32 from the seed xyz0 (T, P, 3) f32, P = G·J, lengths
    (G, n_seg).  Returns dict: X (T, P, 3) f64, xyz (T, P, 3) f32, resid (T, P) f32, nviews (T, P),
    bone (T, G, n_seg) f32, cost (G, 4), group_status (G,), chain_status (P,), margins, rejected (G,),
    r_seen (list of r / L arrays)."""
    used, z, W = tf.views(kpts, cam_idx, mask_bits, weights, gauss, min_conf, cov_floor)
    T, P, nv = used.shape
    G = P // J
    hub = float(huber_delta) if huber_delta > 0 else 0.0
    xyz0 = np.asarray(xyz0, dtype=np.float32)
    pairs = [tuple(int(v) for v in p) for p in np.asarray(pairs, dtype=np.int64).reshape(-1, 2)]
    L = np.asarray(lengths, dtype=np.float32).astype(np.float64).reshape(G, len(pairs))
    X = xyz0.astype(np.float64)
    xyz = xyz0.copy()
    resid = np.full((T, P), np.nan, np.float32)
    bone = np.full((T, G, len(pairs)), np.nan, np.float32)
    cost = np.full((G, 4), np.nan)
    gstatus = np.zeros(G, np.uint8)
    cstatus = np.full(P, INVALID, np.uint8)
    rejected = np.zeros(G, np.int64)
    margins, r_seen = [], []
    for g in range(G):
        sl = slice(g * J, (g + 1) * J)
        chains = []
        for p in range(g * J, (g + 1) * J):
            ch = tf.Chain(cams, cam_idx, used[:, p], z[:, p], W[:, p], hub, float(lambda_smooth))
            chains.append(ch if chain_is_valid(ch, xyz0[:, p]) else None)
        gr = Group(chains, pairs, L[g], lambda_bone)
        r = fit_group(gr, xyz0[:, sl], max_iter, tol)
        gstatus[g], cost[g], rejected[g] = r["status"], r["cost"], r["rejected"]
        margins += r["margins"]
        r_seen += r["r_seen"]
        if r["status"] == INVALID:
            continue
        for j in gr.valid:
            p = g * J + j
            cstatus[p] = 0
            X[:, p] = r["X"][:, j]
            xyz[:, p] = r["X"][:, j].astype(np.float32)
            resid[:, p] = np.where(used[:, p].sum(1) > 0, r["s2"][:, j], np.nan).astype(np.float32)
        bone[:, g, gr.live] = (r["r"][:, gr.live] - L[g][gr.live]).astype(np.float32)
    return {"X": X, "xyz": xyz, "resid": resid, "nviews": used.sum(-1).astype(np.uint8), "bone": bone, "cost": cost,
            "group_status": gstatus, "chain_status": cstatus, "margins": margins, "rejected": rejected,
            "r_seen": r_seen}
