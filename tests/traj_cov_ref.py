"""fp64 numpy reference of mvp_trajectory_smooth_cov and mvp_trajectory_fit_cov, written from the
contract in include/mvpose.h (the reference project has no counterpart).

Per chain, A = blockdiag(W) + λ·(D₂ᵀD₂ ⊗ I₃) with W the smoother's weights (traj_smooth_ref.weights)
or the fit's H̃ blocks, and Σ = A⁻¹.  The calls return Σ_{t,t} and Σ_{t,t+1}.

dense       np.linalg.inv of the symmetrised A, one chain.
banded      a sequential block-pentadiagonal LDLᵀ and the Takahashi recursion back over it, vectorised
            over the chains, for long T; every symmetric block is symmetrised where it is formed.
self_error  how far two fp64 evaluations of the same inverse lie apart (np.linalg.inv against the
            route through np.linalg.cholesky), in the GPU tests' normalisation: the tests' bound is
            meaningful where this is far below it.
Also here: the GPU tests' bound and the smoother cases the CPU and GPU files share."""
import functools

import numpy as np

import traj_smooth_ref as ts

BOUND = 2.0 ** -23   # of sqrt(Σii Σjj): |Σij| <= sqrt(Σii Σjj), rounding to f32 costs 2^-24 of it, and an
                     # fp64 discrepancy of 1e-9 moves a rounding by at most one more half-ulp


def full6(h6):
    """(..., 6) (xx, xy, xz, yy, yz, zz) -> (..., 3, 3)."""
    h6 = np.asarray(h6)
    return h6[..., [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(h6.shape[:-1] + (3, 3))


def matrix(W, lam):
    """A of one chain, W (T, 3, 3), built as traj_smooth_ref.solve_dense builds it, symmetrised."""
    T = W.shape[0]
    D2 = np.zeros((max(T - 2, 0), T))
    for r in range(T - 2):
        D2[r, r:r + 3] = (1.0, -2.0, 1.0)
    A = np.kron(D2.T @ D2, np.eye(3)) * float(lam)
    for t in range(T):
        A[3 * t:3 * t + 3, 3 * t:3 * t + 3] += W[t]
    return 0.5 * (A + A.T)


def _blocks(S, T):
    diag = np.stack([S[3 * t:3 * t + 3, 3 * t:3 * t + 3] for t in range(T)])
    cross = np.full((T, 3, 3), np.nan)
    for t in range(T - 1):
        cross[t] = S[3 * t:3 * t + 3, 3 * t + 3:3 * t + 6]
    return diag, cross


def dense(W, lam):
    """One chain, W (T, 3, 3) -> (Σ_{t,t} (T, 3, 3), Σ_{t,t+1} (T, 3, 3), the last NaN)."""
    W = np.asarray(W, np.float64)
    return _blocks(np.linalg.inv(matrix(W, lam)), W.shape[0])


def dense_chains(W, lam, ok=None):
    """dense over the chains of W (T, P, 3, 3); NaN for the chains where ok is False."""
    T, P = W.shape[:2]
    diag, cross = np.full((T, P, 3, 3), np.nan), np.full((T, P, 3, 3), np.nan)
    for p in range(P):
        if ok is None or ok[p]:
            diag[:, p], cross[:, p] = dense(W[:, p], lam)
    return diag, cross


def banded(W, lam, ok=None):
    """All chains at once, W (T, P, 3, 3) -> (Σ_{t,t}, Σ_{t,t+1}) (T, P, 3, 3); NaN where not ok."""
    W = np.asarray(W, np.float64)
    T, P = W.shape[:2]
    lam = float(lam)
    ok = np.ones(P, bool) if ok is None else np.asarray(ok, bool)
    kd, k1, k2 = np.zeros(T), np.zeros(T), np.zeros(T)     # K[t][t], K[t][t+1], K[t][t+2]
    if T >= 3:
        kd[:-2] += 1
        kd[1:-1] += 4
        kd[2:] += 1
        k1[:-2] += -2
        k1[1:-1] += -2
        k2[:-2] += 1
    eye = np.eye(3)
    sym = lambda M: 0.5 * (M + M.transpose(0, 2, 1))
    A = sym((W + lam * kd[:, None, None, None] * eye).reshape(T * P, 3, 3)).reshape(T, P, 3, 3)
    A[:, ~ok] = eye
    Dinv, Dm = np.zeros((T, P, 3, 3)), np.zeros((T, P, 3, 3))
    L1, L2 = np.zeros((T, P, 3, 3)), np.zeros((T, P, 3, 3))
    for t in range(T):
        D = A[t].copy()
        if t >= 2:
            L2[t] = (lam * k2[t - 2]) * Dinv[t - 2]
        if t >= 1:
            E = (lam * k1[t - 1]) * eye
            if t >= 2:
                E = E - L2[t] @ Dm[t - 2] @ L1[t - 1].transpose(0, 2, 1)
            L1[t] = E @ Dinv[t - 1]
            D = D - sym(L1[t] @ Dm[t - 1] @ L1[t].transpose(0, 2, 1))
        if t >= 2:
            D = D - sym(L2[t] @ Dm[t - 2] @ L2[t].transpose(0, 2, 1))
        Dm[t] = sym(D)
        Dinv[t] = sym(np.linalg.inv(Dm[t]))
    # Takahashi: Σ = D⁻¹ L⁻¹ + (I − Lᵀ) Σ, rows from the last up; L[k][t] is L1[t+1], L2[t+2]
    S0, S1, S2 = np.zeros((T, P, 3, 3)), np.full((T, P, 3, 3), np.nan), np.zeros((T, P, 3, 3))
    tr = lambda M: M.transpose(0, 2, 1)
    for t in range(T - 1, -1, -1):
        s = Dinv[t].copy()
        if t + 2 < T:
            S2[t] = -tr(L1[t + 1]) @ S1[t + 1] - tr(L2[t + 2]) @ S0[t + 2]
        if t + 1 < T:
            S1[t] = -tr(L1[t + 1]) @ S0[t + 1]
            if t + 2 < T:
                S1[t] -= tr(L2[t + 2]) @ tr(S1[t + 1])
            s = s - tr(L1[t + 1]) @ tr(S1[t])
        if t + 2 < T:
            s = s - tr(L2[t + 2]) @ tr(S2[t])
        S0[t] = sym(s)
    S0[:, ~ok] = np.nan
    S1[:, ~ok] = np.nan
    return S0, S1


def norm_error(diag, cross, diag0, cross0):
    """The largest |x − x0| / sqrt(Σii Σjj) over all entries of the blocks, Σii and Σjj the reference's
    (diag0's) diagonal entries of the two frames; NaN patterns must agree."""
    diag, cross, diag0, cross0 = (np.asarray(a, np.float64) for a in (diag, cross, diag0, cross0))
    assert np.array_equal(np.isnan(diag), np.isnan(diag0)), "NaN pattern of Σ_tt"
    assert np.array_equal(np.isnan(cross), np.isnan(cross0)), "NaN pattern of Σ_t,t+1"
    with np.errstate(invalid="ignore"):
        d = np.sqrt(np.einsum("...ii->...i", diag0))
        e0 = np.abs(diag - diag0) / (d[..., :, None] * d[..., None, :])
        nxt = np.concatenate([d[1:], np.full_like(d[:1], np.nan)])
        e1 = np.abs(cross - cross0) / (d[..., :, None] * nxt[..., None, :])
    return float(max(np.nanmax(e0, initial=0.0), np.nanmax(e1, initial=0.0)))


def self_error(W, lam):
    """One chain, W (T, 3, 3): norm_error between np.linalg.inv(A) and L⁻ᵀ L⁻¹ of np.linalg.cholesky(A)."""
    W = np.asarray(W, np.float64)
    T = W.shape[0]
    A = matrix(W, lam)
    Li = np.linalg.inv(np.linalg.cholesky(A))
    a, b = _blocks(np.linalg.inv(A), T), _blocks(Li.T @ Li, T)
    return norm_error(b[0], b[1], a[0], a[1])


def reversed_error(W, lam, ok=None):
    """For T too long for a dense inverse: norm_error between banded and banded run on the time-
    reversed chains (A reversed is the same kind of matrix, eliminated from the other end: a second,
    independent fp64 evaluation of the same blocks)."""
    a0, a1 = banded(W, lam, ok)
    b0, b1 = banded(W[::-1], lam, ok)
    b0 = b0[::-1]
    c1 = np.full_like(b1, np.nan)
    c1[:-1] = b1[::-1][1:].transpose(0, 1, 3, 2)     # Σ_{t,t+1} = (Σ_{t+1,t})ᵀ
    return norm_error(b0, c1, a0, a1)


# ------------------------------------------------------------------ the smoother cases
COV_FLOOR = 0.01
# (T, P, chunk, λ, use cov, use valid).  Chunk 4: no separator; a 1-frame separator; a 2-frame
# separator; a last chunk of 1 interior frame; several chunks.  Then longer chunks across λ (chunk 32
# with λ >= 1e2 is where an unsymmetrised recursion breaks down), without cov (sigma0 = 0.5), without
# valid.  T > 20 has a 9-frame gap in chain 0.
SMOOTH_CASES = ([(T, 3, 4, 1.0, True, True) for T in (2, 3, 4, 5, 6, 7, 11, 12, 13, 23, 64, 257)]
                + [(T, 3, chunk, lam, True, True) for T, chunk in ((64, 5), (64, 32), (300, 32))
                   for lam in (1e-2, 1.0, 1e2, 1e4)]
                + [(64, 3, 4, 1.0, False, True), (64, 3, 4, 1.0, True, False)])
LONG_CASE = (4099, 2, 0, 1.0, True, True)
SIGMA0 = 0.5
GAP = 9


def case_id(c):
    return f"T{c[0]}-P{c[1]}-chunk{c[2]}-lam{c[3]:g}" + ("" if c[4] else "-nocov") + ("" if c[5] else "-novalid")


@functools.lru_cache(maxsize=None)
def smooth_case(c):
    """The inputs of case c (traj_smooth_ref.make_case; chain 1 keeps its first two frames clean
    whatever the knock-outs hit, so that every case has a chain that does not fail) and its
    reference: dict(xyz, cov or None, valid or None, kw, W, ok, diag, cross)."""
    T, P, chunk, lam, use_cov, use_valid = c
    m = ts.make_case(T, P, seed=T, long_gap=GAP if T > 20 else None)
    m["valid"][:2, 1] = 1
    m["xyz"][:2, 1] = m["truth"][:2, 1].astype(np.float32)
    m["cov"][:2, 1] = np.eye(3, dtype=np.float32)
    cov, valid = (m["cov"] if use_cov else None), (m["valid"] if use_valid else None)
    W, _, obs = ts.weights(m["xyz"], cov, valid, SIGMA0, COV_FLOOR)
    ok = obs.sum(0) >= 2
    diag, cross = banded(W, lam, ok) if T > 1000 else dense_chains(W, lam, ok)
    kw = dict(lambda_smooth=lam, sigma0=SIGMA0, cov_floor=COV_FLOOR, chunk=chunk)
    return {"xyz": m["xyz"], "cov": cov, "valid": valid, "kw": kw, "W": W, "ok": ok, "observed": obs, "diag": diag,
            "cross": cross}
