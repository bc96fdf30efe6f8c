"""CPU: the trajectory fit's fp64 numpy restatement (tests/traj_fit_ref.py, written from the text in
include/mvpose.h) checked on its own, the scene the fit was designed for, the decision margins of
the cases the GPU tests compare, and the argument checks of the three C entry points."""
import ctypes

import numpy as np
import pytest

import traj_fit_cases as tc
import traj_fit_ref as tf
import tri_refine_ref as tr
from mvpose import synthetic as syn


def small_chain(hub, weights=tr.W_CONF, lam=0.7, T=6, seed=4):
    rng = np.random.default_rng(seed)
    cams = syn.make_rig(3, seed=3)
    truth = syn.make_poses(T, seed=seed, jitter=1.0)[:, :1]
    kpts = syn.make_kpts_2d(truth, cams, seed=seed + 1, noise_px=2.0)
    kpts[2, 0, 0, 1] = np.nan            # a frame seen by views 0 and 2
    kpts[3, 0, 0, 1] = kpts[3, 0, 0, 2] = np.nan   # by view 0 alone
    kpts[4, 0, 0, :] = np.nan            # by none
    used, z, W = tf.views(kpts, [0, 1, 2], None, weights, None, 0.0, 1.0)
    X = truth[:, 0] + rng.normal(0.0, 1.0, (T, 3))
    return tf.Chain(cams, [0, 1, 2], used[:, 0], z[:, 0], W[:, 0], hub, lam), X


@pytest.mark.parametrize("hub", [0.0, 1.5])
def test_gradient_matches_central_differences(hub):
    """G = g̃ + λ·D₂ᵀD₂·X is the gradient of the chain's cost, Huber on and off."""
    ch, X = small_chain(hub)
    _, G = ch.linearise(X)
    num = np.zeros_like(G)
    h = 1e-4
    for k in range(G.size):
        e = np.zeros(G.size)
        e[k] = h
        num[k] = (ch.cost(X + e.reshape(X.shape))[0] - ch.cost(X - e.reshape(X.shape))[0]) / (2 * h)
    err = np.abs(G - num).max() / np.abs(G).max()
    print(f"hub {hub}: gradient rel err {err:.3g}")
    assert err < 1e-7


@pytest.mark.parametrize("hub", [0.0, 1.5])
def test_gauss_newton_blocks_match_central_differences(hub):
    """H̃_t = Σ_used Jᵀ·W̃·J with J from central differences of the forward model; A's off-diagonal
    blocks are λ·D₂ᵀD₂'s."""
    ch, X = small_chain(hub)
    A, _ = ch.linearise(X)
    T = X.shape[0]
    h = 1e-4
    for t in range(T):
        H = np.zeros((3, 3))
        for i, col in enumerate(ch.cam_idx):
            if not ch.used[t, i]:
                continue
            J = np.stack([(syn.project(X[t] + h * e, ch.cams[col]) - syn.project(X[t] - h * e, ch.cams[col])) / (2 * h)
                          for e in np.eye(3)], 1)
            r = syn.project(X[t], ch.cams[col]) - ch.z[t, i]
            s = np.sqrt(r @ ch.W[t, i] @ r)
            om = 1.0 if not (hub > 0 and s > hub) else hub / s
            H += J.T @ (om * ch.W[t, i]) @ J
        blk = A[3 * t:3 * t + 3, 3 * t:3 * t + 3] - ch.lam * ch.K3[3 * t:3 * t + 3, 3 * t:3 * t + 3]
        assert np.abs(blk - H).max() <= 1e-7 * max(np.abs(H).max(), 1.0), t
    off = A - ch.lam * ch.K3
    for t in range(T):
        off[3 * t:3 * t + 3, 3 * t:3 * t + 3] = 0.0
    assert np.abs(off).max() == 0.0
    assert np.array_equal(ch.used.sum(1), [3, 3, 2, 1, 0, 3])


def test_system_is_the_chain_linearisation():
    """tf.system (all chains at once, the _system entry point's layout) against tf.Chain."""
    c = tc.case(6)
    H6, g, nviews, cost = tc.reference_system(6)
    used, z, W = tf.views(c["kpts"], c["cam_idx"], c["kw"]["mask_bits"], c["kw"]["weights"], None, tc.MIN_CONF, 1.0)
    p = 3
    ch = tf.Chain(c["cams"], c["cam_idx"], used[:, p], z[:, p], W[:, p], c["kw"]["huber_delta"], 1.0)
    X = c["xyz0"][:, p].astype(np.float64)
    A, G = ch.linearise(X)
    T = X.shape[0]
    for t in range(T):
        blk = A[3 * t:3 * t + 3, 3 * t:3 * t + 3] - ch.K3[3 * t:3 * t + 3, 3 * t:3 * t + 3]
        assert np.allclose(blk[np.triu_indices(3)], H6[t, p], rtol=1e-12, atol=0)
    assert np.allclose(G - ch.K3 @ X.ravel(), g[:, p].ravel(), rtol=1e-12, atol=1e-9)
    assert np.isclose(cost[p].sum(), ch.cost(X)[0], rtol=1e-12)
    assert np.array_equal(nviews[:, p], used[:, p].sum(1))


def test_gap_scene_single_view_frames_count():
    """make_rig(2), 120 frames, camera 1 blind for frames 50..59: the smoother fills the gap from
    its ends; the fit also uses what camera 0 still sees there."""
    g = tc.gap_scene()
    seed_xyz, fit_xyz, fit = tc.gap_reference()
    a, b = tc.gap_rms(seed_xyz, g["truth"]), tc.gap_rms(fit_xyz, g["truth"])
    print(f"gap RMS: seed {a:.3f} cm, fit {b:.3f} cm, factor {a / b:.3f}; status {[hex(s) for s in fit['status']]}")
    assert (fit["status"] & 0xC0 == 0).all()
    assert np.array_equal(fit["nviews"][tc.GAP[0]:tc.GAP[1]], np.ones((10, 3), np.uint8))
    assert a / b >= tc.GAP_FACTOR
    # outside the gap the fit stays where the two-view data put it
    out = np.r_[0:tc.GAP[0] - 5, tc.GAP[1] + 5:120]
    sel = list(tc.GAP_JOINTS)
    assert np.abs(fit_xyz[out][:, sel] - seed_xyz[out][:, sel]).max() < 3.0


@pytest.mark.parametrize("i", range(len(tc.CASES)), ids=[tc.case_id(kw) for kw in tc.CASES])
def test_decision_margins_of_the_gpu_cases(i):
    """Every accept and convergence comparison of the restatement's run has a relative margin above
    1e-6, so that fp64 rounding cannot flip it on the device."""
    r = tc.reference_fit(i)
    m = min(r["margins"]) if r["margins"] else np.inf
    print(f"{tc.case_id(tc.CASES[i])}: {len(r['margins'])} comparisons, smallest margin {m:.3g}; "
          f"status {sorted(set(hex(s) for s in r['status']))}")
    assert m > 1e-6


def test_cases_reach_their_paths():
    """The patterns the GPU cases are there for do occur in them."""
    st = [tc.reference_fit(i)["status"] for i in range(len(tc.CASES))]
    nv = [tc.reference_fit(i)["nviews"] for i in range(len(tc.CASES))]
    assert st[0].tolist() == [tf.INVALID]                              # T = 1
    assert st[1][2] == tf.INVALID and (st[1][:2] & 0xC0 == 0).all()    # starved
    assert st[3][3] == tf.INVALID                                      # NaN seed frame
    assert st[5][1] == tf.INVALID                                      # behind its camera
    assert [st[7][p] for p in (20, 33, 64)] == [tf.INVALID] * 3
    assert (nv[6][4:9, 2] == 0).all() and (nv[7][3:8, 7] == 0).all()   # blind stretches
    for n1 in (nv[7][15:25, 0], nv[8][100:110, 5]):                   # single-view stretches (a confidence below
        assert (n1 <= 1).all() and (n1 == 1).sum() >= 5                # min_conf or a random drop can take view 0 too)
    for i in (3, 6, 8):
        assert (nv[i] < tc.CASES[i]["nv"]).mean() > 0.2                # random drops
    valid = np.concatenate([s[s != tf.INVALID] for s in st[:9]])
    assert (valid & 0x40 == 0).all() and (valid & 63).max() <= tc.MAX_ITER
    assert all(tc.reference_fit(i)["rejected"].sum() == 0 for i in range(9))      # the issue's nine accept every trial
    # the rough seeds: rejected trials followed by accepted ones, with and without the Huber loss;
    # convergence after rejections; out of trials (0x40 with a trial count) at 12 and at 3
    rough, huber, short = (tc.reference_fit(i) for i in (9, 10, 11))
    assert rough["rejected"].tolist() == [4, 0, 7, 4, 0] and st[9].tolist() == [0x09, 0x80, 0x4C, 0x4C, 0x05]
    assert huber["rejected"].tolist() == [0, 0, 0, 5, 0] and st[10].tolist() == [0x06, 0x80, 0x05, 0x4C, 0x80]
    assert short["rejected"].tolist() == [0, 0, 0, 1, 0] and st[11].tolist() == [0x43, 0x80, 0x43, 0x43, 0x80]
    for r in (rough, huber, short):                                               # and every one of them moved
        ok = r["status"] != tf.INVALID
        assert (r["cost"][ok, 1] < r["cost"][ok, 0]).all()


# ------------------------------------------------------------------ the C entry points' argument checks
GOOD = dict(T=10, P=17, V=2, n_cams=2, nv=2, weights=1, gauss=None, min_conf=0.0, cov_floor=1.0, hub=0.0, lam=1.0,
            max_iter=10, tol=1e-6, chunk=0, ws_bytes=1 << 40)
BAD = [
    (dict(T=0), "T=0"), (dict(P=0), "P=0"), (dict(T=65536, P=32768), "2^31"),
    (dict(nv=1), "n_cam_idx=1"), (dict(nv=9, n_cams=8, V=9), "n_cam_idx=9"),
    (dict(lam=0.0), "lambda_smooth"), (dict(lam=float("inf")), "lambda_smooth"), (dict(lam=float("nan")), "lambda_smooth"),
    (dict(tol=0.0), "tol"), (dict(tol=float("nan")), "tol"), (dict(cov_floor=-1.0), "cov_floor"),
    (dict(cov_floor=float("nan")), "cov_floor"), (dict(min_conf=float("nan")), "min_conf"),
    (dict(hub=float("nan")), "huber_delta"), (dict(max_iter=64), "max_iter"), (dict(max_iter=-1), "max_iter"),
    (dict(chunk=3), "chunk"), (dict(weights=3), "weights"), (dict(weights=2), "gauss"), (dict(ws_bytes=16), "workspace_bytes"),
]
SYSTEM_KEYS = {"T", "P", "V", "n_cams", "nv", "weights", "min_conf", "cov_floor", "hub"}


def call_fit(a):
    from mvpose import _lib
    ci = (ctypes.c_int * 9)(*range(9))
    return _lib.lib.mvp_trajectory_fit(None, a["T"], a["P"], a["V"], None, a["n_cams"], ci, a["nv"], None, None,
                                       a["weights"], a["gauss"], a["min_conf"], a["cov_floor"], a["hub"], a["lam"],
                                       a["max_iter"], a["tol"], a["chunk"], None, a["ws_bytes"], None, None, None, None,
                                       None, None)


def call_system(a):
    from mvpose import _lib
    ci = (ctypes.c_int * 9)(*range(9))
    return _lib.lib.mvp_trajectory_fit_system(None, a["T"], a["P"], a["V"], None, a["n_cams"], ci, a["nv"], None, None,
                                              a["weights"], a["gauss"], a["min_conf"], a["cov_floor"], a["hub"], None,
                                              None, None, None, None)


@pytest.mark.parametrize("bad,word", BAD, ids=[f"{'-'.join(f'{k}={v}' for k, v in b.items())}" for b, _ in BAD])
def test_argument_errors(bad, word):
    """MVP_ERR_ARG naming the argument, before any device work (every pointer here is NULL)."""
    from mvpose import _lib
    a = dict(GOOD, **bad)
    assert call_fit(a) == -1
    assert word in _lib.last_error(), _lib.last_error()
    if set(bad) <= SYSTEM_KEYS:
        assert call_system(a) == -1
        assert word in _lib.last_error(), _lib.last_error()


def test_good_arguments_reach_the_pointer_check_and_the_plan():
    from mvpose import _lib
    assert call_fit(GOOD) == -1 and "null device pointer" in _lib.last_error()
    assert call_system(GOOD) == -1 and "null device pointer" in _lib.last_error()
    used, n_chunks, nbytes = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int64(0)
    rc = _lib.lib.mvp_trajectory_fit_plan(100, 17, 0, ctypes.byref(used), ctypes.byref(n_chunks), ctypes.byref(nbytes))
    s_used, s_chunks, s_bytes = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int64(0)
    _lib.lib.mvp_trajectory_smooth_plan(100, 17, 0, ctypes.byref(s_used), ctypes.byref(s_chunks), ctypes.byref(s_bytes))
    assert rc == 0 and (used.value, n_chunks.value) == (s_used.value, s_chunks.value)
    # the solver's workspace, two fp64 states, H, g, the cost terms
    assert nbytes.value >= s_bytes.value + 100 * 17 * 8 * (6 + 9 + 2)
    assert _lib.lib.mvp_trajectory_fit_plan(0, 17, 0, None, None, None) == -1
    assert _lib.lib.mvp_trajectory_fit_plan(100, 17, 5000, None, None, None) == -1
