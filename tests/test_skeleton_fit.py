"""CPU: the skeleton fit's fp64 numpy restatement (tests/skel_fit_ref.py, written from the text in
include/mvpose.h) checked on its own, the arm scene the fit was designed for, the decision margins
and paths of the cases the GPU tests compare, people.estimate_bone_lengths, and the argument checks
of the three C entry points."""
import ctypes

import numpy as np
import pytest
import torch

import skel_fit_cases as sc
import skel_fit_ref as sk
import traj_fit_ref as tf
import tri_refine_ref as tr
from mvpose import people, synthetic as syn


def small_group(hub, beta=3.0, lam=0.7, T=5, J=4, seed=4):
    """Four joints over five frames on three cameras, with a frame seen by two views, by one and by
    none, an invalid chain (joint 3), a dead length, and a state in which segment (0, 1) is shorter
    than its length and segment (2, 1) longer."""
    rng = np.random.default_rng(seed)
    cams = syn.make_rig(3, seed=3)
    truth = syn.make_poses(T, seed=seed, jitter=1.0)[:, :J]
    kpts = syn.make_kpts_2d(truth, cams, seed=seed + 1, noise_px=2.0)
    kpts[2, 0, 0, 1] = np.nan
    kpts[3, 1, 0, 1] = kpts[3, 1, 0, 2] = np.nan
    kpts[4, 2, 0, :] = np.nan
    used, z, W = tf.views(kpts, [0, 1, 2], None, tr.W_CONF, None, 0.0, 1.0)
    chains = [tf.Chain(cams, [0, 1, 2], used[:, j], z[:, j], W[:, j], hub, lam) if j < 3 else None for j in range(J)]
    X = truth + rng.normal(0.0, 1.0, truth.shape)
    pairs = [(0, 1), (2, 1), (0, 2), (2, 3), (1, 3)]
    r = [np.linalg.norm(X[:, b] - X[:, a], axis=-1) for a, b in pairs]
    L = np.array([r[0].max() + 2.0, r[1].min() - 2.0, np.nan, r[3].mean(), r[4].mean()])
    return sk.Group(chains, pairs, L, beta), X


@pytest.mark.parametrize("hub", [0.0, 1.5])
def test_gradient_matches_central_differences(hub):
    """The group's G is the gradient of f_g, Huber on and off, with a segment shorter than its length
    and one longer in the state."""
    gr, X = small_group(hub)
    T, J, _ = X.shape
    assert gr.live.tolist() == [True, True, False, False, False] and gr.valid == [0, 1, 2]
    r = gr.cost(X)[3]
    assert (r[:, 0] < gr.L[0]).all() and (r[:, 1] > gr.L[1]).all()
    _, G = gr.dense(X)
    num = np.zeros_like(G)
    h = 1e-4
    for j in gr.valid:
        for k in range(3 * T):
            E = np.zeros((T, J, 3))
            E[k // 3, j, k % 3] = h
            num[3 * T * j + k] = (gr.cost(X + E)[0] - gr.cost(X - E)[0]) / (2 * h)
    err = np.abs(G - num).max() / np.abs(G).max()
    print(f"hub {hub}: gradient rel err {err:.3g}")
    assert err < 1e-7
    assert (G[3 * T * 3:] == 0).all()                     # the invalid chain has no unknowns


def test_curvature_blocks_are_the_stated_formula():
    """A chain's frame block is the trajectory fit's plus 2β·[n nᵀ + max(0, 1 − L/r)·(I − n nᵀ)] per
    live segment at the joint; the chain-to-chain blocks are exactly zero."""
    gr, X = small_group(1.5)
    T, J, _ = X.shape
    M, _ = gr.dense(X)
    shrunk = 0
    for j in gr.valid:
        A0, _ = gr.chains[j].linearise(X[:, j])
        Aj = M[3 * T * j:3 * T * (j + 1), 3 * T * j:3 * T * (j + 1)]
        extra = Aj - A0
        for t in range(T):
            want = np.zeros((3, 3))
            for s, (a, b) in enumerate(gr.pairs):
                if not gr.live[s] or j not in (a, b):
                    continue
                d = X[t, b] - X[t, a]
                r = np.linalg.norm(d)
                n = d / r
                w = max(0.0, 1.0 - gr.L[s] / r)
                shrunk += w == 0.0
                want += 2 * gr.beta * (np.outer(n, n) + w * (np.eye(3) - np.outer(n, n)))
            blk = extra[3 * t:3 * t + 3, 3 * t:3 * t + 3]
            assert np.abs(blk - want).max() <= 1e-12 * max(np.abs(Aj).max(), 1.0), (j, t)
            extra[3 * t:3 * t + 3, 3 * t:3 * t + 3] = 0.0
        assert np.abs(extra).max() <= 1e-12 * np.abs(Aj).max()      # the bones touch the frame blocks only
    assert shrunk > 0                                     # the clamp at r < L was reached
    for j in range(J):
        M[3 * T * j:3 * T * (j + 1), 3 * T * j:3 * T * (j + 1)] = 0.0
    assert np.abs(M).max() == 0.0


def test_r_zero_costs_half_beta_L2_and_has_no_derivatives():
    X = np.zeros((2, 2, 3))
    X[1, 1] = (3.0, 0.0, 4.0)
    half, g, H, r = sk.bone_terms(X, [(0, 1)], np.array([2.0]), np.array([True]), 3.0)
    assert r[:, 0].tolist() == [0.0, 5.0] and half == 0.5 * 4.0 + 0.5 * 9.0
    assert (g[0] == 0).all() and (H[0] == 0).all()
    assert np.allclose(g[1, 1], 3.0 * 3.0 * np.array([0.6, 0.0, 0.8])) and np.allclose(g[1, 0], -g[1, 1])


def test_system_is_the_group_linearisation():
    """sk.system (the _system entry point's layout, every live length live) against sk.Group."""
    i = 2
    c = sc.case(i)
    H6, g, nviews, cost = sc.reference_system(i)
    used, z, W = tf.views(c["kpts"], c["cam_idx"], c["kw"]["mask_bits"], c["kw"]["weights"], c["gauss"], sc.MIN_CONF, 1.0)
    J = c["J"]
    chains = [tf.Chain(c["cams"], c["cam_idx"], used[:, p], z[:, p], W[:, p], c["kw"]["huber_delta"], 1.0)
              for p in range(J)]
    gr = sk.Group(chains, c["pairs"], c["lengths"][0].astype(np.float64), c["beta"])
    X = c["xyz0"].astype(np.float64)
    T = X.shape[0]
    for j, (A, G) in gr.linearise(X).items():
        K3 = chains[j].K3
        for t in range(T):
            blk = A[3 * t:3 * t + 3, 3 * t:3 * t + 3] - K3[3 * t:3 * t + 3, 3 * t:3 * t + 3]
            assert np.allclose(blk[np.triu_indices(3)], H6[t, j], rtol=1e-12, atol=0)
        assert np.allclose(G - K3 @ X[:, j].ravel(), g[:, j].ravel(), rtol=1e-12, atol=1e-9)
    f, fb, _, _ = gr.cost(X)
    assert np.isclose(cost[0, 0] + cost[0, 1] + c["beta"] * cost[0, 2], f, rtol=1e-12)
    assert np.isclose(c["beta"] * cost[0, 2], fb, rtol=1e-12)


def test_arm_scene_a_known_bone_pins_the_lost_joint():
    """make_rig(2), 120 frames, camera 1 without the left elbow and wrist for frames 40..79, all 17
    joints fitted with the 12 segments at their true lengths: λ = 0.25, β = 1, tol 1e-4, 60 trials."""
    a = sc.arm_scene()
    seed_xyz, fit = sc.arm_reference()
    _, plain = sc.arm_reference(0.0)
    s, f, p = (sc.arm_rms(x, a["truth"]) for x in (seed_xyz, fit["xyz"], plain["xyz"]))
    print(f"gap RMS over joints {sc.ARM_JOINTS}: blind fill {s:.3f} cm, fit with bones {f:.3f} cm (factor {s / f:.3f}), "
          f"fit without bones {p:.3f} cm; status {[hex(v) for v in fit['group_status']]}, rejected {fit['rejected']}")
    assert (fit["group_status"] & 0xC0 == 0).all() and (fit["chain_status"] == 0).all()
    assert (fit["nviews"][sc.ARM_GAP[0]:sc.ARM_GAP[1]][:, list(sc.ARM_JOINTS)] == 1).all()
    assert s / f >= sc.ARM_FACTOR
    assert p > s                                          # without bones the fit is worse than the blind fill here
    out = np.r_[0:sc.ARM_GAP[0] - 5, sc.ARM_GAP[1] + 5:120]
    assert np.abs(fit["xyz"][out] - seed_xyz[out]).max() < 3.0


IDS = [sc.case_id(kw) for kw in sc.CASES]


@pytest.mark.parametrize("i", range(len(sc.CASES)), ids=IDS)
def test_decision_margins_of_the_gpu_cases(i):
    """Every accept and convergence comparison of the restatement's run has a relative margin of at
    least 1e-6, so that fp64 rounding cannot flip it on the device; every live segment the run met
    has r == 0 exactly or r > 1e-6·L, so that rounding cannot move it across the r == 0 rule."""
    r = sc.reference_fit(i)
    m = min(r["margins"]) if r["margins"] else np.inf
    rs = np.concatenate([x.ravel() for x in r["r_seen"]]) if r["r_seen"] else np.zeros(0)
    print(f"{IDS[i]}: {len(r['margins'])} comparisons, smallest margin {m:.3g}; {rs.size} segment lengths, "
          f"{int((rs == 0).sum())} zero, smallest other r / L {rs[rs != 0].min() if (rs != 0).any() else np.nan:.3g}; "
          f"status {[hex(s) for s in r['group_status']]}")
    assert m >= 1e-6
    assert np.isfinite(rs).all() and ((rs == 0) | (rs > 1e-6)).all()


def test_cases_reach_their_paths():
    """The patterns the GPU cases are there for do occur in them."""
    fits = [sc.reference_fit(i) for i in range(len(sc.CASES))]
    gs = [f["group_status"] for f in fits]
    cs = [f["chain_status"] for f in fits]
    assert gs[0].tolist() == [sk.INVALID]                                         # T = 1: an all-invalid group
    assert gs[3][2] == sk.INVALID and (cs[3][8:] == sk.INVALID).all()             # every seed NaN
    assert np.isnan(fits[3]["cost"][2]).all() and np.isnan(fits[3]["bone"][:, 2]).all()
    # an invalid chain inside a valid group: the chain is returned, its segments are dead, the rest is fitted
    assert cs[3][6] == sk.INVALID and gs[3][1] & 0xC0 == 0
    assert cs[4][3] == sk.INVALID and cs[4][33] == sk.INVALID and (gs[4] & 0xC0 == 0).all()
    dead = [s for s, (a, b) in enumerate(sc.PAIRS4) if 2 in (a, b)]
    assert np.isnan(fits[3]["bone"][:, 1][:, dead]).all() and np.isfinite(np.delete(fits[3]["bone"][:, 1], dead, 1)).all()
    # dead lengths
    assert np.isnan(fits[2]["bone"][:, 0, [3, 8]]).all() and np.isnan(fits[4]["bone"][:, 1, [0, 5]]).all()
    assert np.isfinite(np.delete(fits[2]["bone"][:, 0], [3, 8], 1)).all()
    # r == 0 exactly, at the seed and nowhere after it
    for i in (1, 2):
        assert sum(int((r == 0).sum()) for r in fits[i]["r_seen"]) == 1
    # the cases with a gentle seed accept every trial and converge
    for i in range(1, 7):
        ok = gs[i] != sk.INVALID
        assert (gs[i][ok] & 0x40 == 0).all() and fits[i]["rejected"].sum() == 0
    # the rough seeds: group 0 rejects 3 trials and then converges at its 12th, group 2 runs out of its 12;
    # "short" is stopped after 3
    rough, short = fits[7], fits[8]
    assert rough["rejected"].tolist() == [3, 0, 0] and gs[7].tolist() == [0x0C, 0x06, 0x4C]
    assert gs[8].tolist() == [0x43, 0x43, 0x43]
    for r in (rough, short):
        assert (r["cost"][:, 1] < r["cost"][:, 0]).all()
    # every weight mode, masks, Huber, 2 and 3 views, G in {1, 3}, J in {1, 4, 17}, T in {1, 2, 7, 40, 130}
    assert {kw["weights"] for kw in sc.CASES} == {tr.W_UNIT, tr.W_CONF, tr.W_GAUSS}
    assert {kw["T"] for kw in sc.CASES} == {1, 2, 7, 40, 130} and {kw["J"] for kw in sc.CASES} == {1, 4, 17}


def test_j1_is_the_trajectory_fit():
    """With one joint per group the restatement is traj_fit_ref's, number for number."""
    c = sc.case(sc.J1_CASE)
    r = sc.reference_fit(sc.J1_CASE)
    t = tf.fit(c["kpts"], c["cams"], c["cam_idx"], c["xyz0"], lambda_smooth=c["lam"], max_iter=c["max_iter"], tol=sc.TOL,
               **c["kw"])
    assert np.array_equal(r["group_status"], t["status"])
    assert np.array_equal(r["xyz"].view(np.uint32), t["xyz"].view(np.uint32))
    assert np.array_equal(r["cost"][:, :2], t["cost"], equal_nan=True)


# ------------------------------------------------------------------ people.estimate_bone_lengths
def test_estimate_bone_lengths_is_the_median_over_the_usable_frames():
    """Rigid people (every frame the same offsets, moved about) but for one joint, some frames NaN: the
    per-person median over the frames where both ends are finite (and valid), NaN below min_frames."""
    rng = np.random.default_rng(0)
    T, G, J = 30, 2, 5
    # whole numbers: every difference and every sum of squares is exact in float32, so the distances
    # do not depend on the order of a norm's additions
    shape = rng.integers(-40, 41, (G, J, 3))
    xyz = (shape[None] + rng.integers(-100, 101, (T, G, 1, 3))).astype(np.float32)
    pairs = [(0, 1), (1, 2), (3, 4), (4, 0)]
    xyz[:, 0, 2] += rng.integers(-3, 4, (T, 3)).astype(np.float32)   # person 0's joint 2 is not rigid: a true median
    xyz[5:12, 0, 1, 0] = np.nan                           # 7 frames of person 0's joint 1
    xyz[3:27, 1, 3] = np.nan                              # person 1's joint 3: 6 frames left
    valid = np.ones((T, G, J), bool)
    valid[8:, 0, 4] = False                               # person 0's joint 4: 8 valid frames
    x = torch.tensor(xyz)
    got = people.estimate_bone_lengths(x, pairs, valid=torch.tensor(valid), min_frames=10).numpy()
    assert got.shape == (G, len(pairs)) and got.dtype == np.float32
    d = np.linalg.norm(xyz[:, :, [b for _, b in pairs]] - xyz[:, :, [a for a, _ in pairs]], axis=-1)   # (T, G, n_seg)
    ok = np.isfinite(d)
    ok[8:, 0, 2] = ok[8:, 0, 3] = False
    for g in range(G):
        for s in range(len(pairs)):
            v = np.sort(d[ok[:, g, s], g, s])
            want = v[(len(v) - 1) // 2] if len(v) >= 10 else np.nan      # torch's median: the lower middle
            assert (np.isnan(want) and np.isnan(got[g, s])) or got[g, s] == want, (g, s)
    assert np.isnan(got[1, 2]) and np.isfinite(got[0, :2]).all() and np.isnan(got[0, 2:]).all()
    # one person, (T, J, 3), no valid mask
    one = people.estimate_bone_lengths(x[:, 0], pairs).numpy()
    assert one.shape == (len(pairs),)
    assert one[0] == got[0, 0] and one[1] == got[0, 1]    # the mask took frames from joint 4's segments only
    assert np.isfinite(one[2:]).all()


# ------------------------------------------------------------------ the C entry points' argument checks
GOOD = dict(T=10, P=34, V=2, n_cams=2, nv=2, weights=1, gauss=None, min_conf=0.0, cov_floor=1.0, hub=0.0, lam=1.0,
            J=17, seg=[], seg_len=None, beta=1.0, max_iter=10, tol=1e-6, chunk=0, ws_bytes=1 << 40)
LEN = ctypes.c_void_p(256)      # a non-NULL lengths pointer: the argument checks never read it
BAD = [
    (dict(T=0), "T=0"), (dict(P=0), "P=0"), (dict(T=65536, P=32768, J=1), "2^31"),
    (dict(nv=1), "n_cam_idx=1"), (dict(nv=9, n_cams=8, V=9), "n_cam_idx=9"),
    (dict(lam=0.0), "lambda_smooth"), (dict(lam=float("inf")), "lambda_smooth"), (dict(lam=float("nan")), "lambda_smooth"),
    (dict(tol=0.0), "tol"), (dict(tol=float("nan")), "tol"), (dict(cov_floor=-1.0), "cov_floor"),
    (dict(cov_floor=float("nan")), "cov_floor"), (dict(min_conf=float("nan")), "min_conf"),
    (dict(hub=float("nan")), "huber_delta"), (dict(max_iter=64), "max_iter"), (dict(max_iter=-1), "max_iter"),
    (dict(chunk=3), "chunk"), (dict(weights=3), "weights"), (dict(weights=2), "gauss"), (dict(ws_bytes=16), "workspace_bytes"),
    (dict(J=0), "J=0"), (dict(J=256, P=512), "J=256"), (dict(J=16), "multiple of J"),
    (dict(beta=-1.0), "lambda_bone"), (dict(beta=float("nan")), "lambda_bone"), (dict(beta=float("inf")), "lambda_bone"),
    (dict(seg=[(0, 1)]), "seg_len_dev"), (dict(seg=[(0, 17)], seg_len=LEN), "seg_host[0]"),
    (dict(seg=[(-1, 2)], seg_len=LEN), "seg_host[0]"), (dict(seg=[(0, 1), (3, 3)], seg_len=LEN), "seg_host[1]"),
    (dict(seg=[(0, 1), (2, 3), (1, 0)], seg_len=LEN), "seg_host[2] repeats"),
    (dict(seg=[(k, k + 1) for k in range(16)] * 5, seg_len=LEN), "n_seg=80"),
]
SYSTEM_KEYS = {"T", "P", "V", "n_cams", "nv", "weights", "min_conf", "cov_floor", "hub", "J", "seg", "seg_len", "beta"}
PLAN_KEYS = {"T", "P", "J", "chunk"}


def seg_args(a):
    flat = [v for pair in a["seg"] for v in pair]
    return (ctypes.c_int * max(len(flat), 1))(*flat), len(a["seg"])


def call_fit(a):
    from mvpose import _lib
    ci = (ctypes.c_int * 9)(*range(9))
    seg, n_seg = seg_args(a)
    return _lib.lib.mvp_skeleton_fit(None, a["T"], a["P"], a["V"], None, a["n_cams"], ci, a["nv"], None, None,
                                     a["weights"], a["gauss"], a["min_conf"], a["cov_floor"], a["hub"], a["lam"], a["J"],
                                     seg, n_seg, a["seg_len"], a["beta"], a["max_iter"], a["tol"], a["chunk"], None,
                                     a["ws_bytes"], None, None, None, None, None, None, None, None)


def call_system(a):
    from mvpose import _lib
    ci = (ctypes.c_int * 9)(*range(9))
    seg, n_seg = seg_args(a)
    return _lib.lib.mvp_skeleton_fit_system(None, a["T"], a["P"], a["V"], None, a["n_cams"], ci, a["nv"], None, None,
                                            a["weights"], a["gauss"], a["min_conf"], a["cov_floor"], a["hub"], a["J"], seg,
                                            n_seg, a["seg_len"], a["beta"], None, None, None, None, None)


def call_plan(a):
    from mvpose import _lib
    return _lib.lib.mvp_skeleton_fit_plan(a["T"], a["P"], a["J"], a["chunk"], None, None, None)


def bad_id(b):
    return "-".join(f"{k}={len(v) if k == 'seg' else 'ptr' if k == 'seg_len' else v}" for k, v in b.items())


@pytest.mark.parametrize("bad,word", BAD, ids=[bad_id(b) + f"-{n}" for n, (b, _) in enumerate(BAD)])
def test_argument_errors(bad, word):
    """MVP_ERR_ARG naming the argument, before any device work (every device pointer here is NULL or
    never read)."""
    from mvpose import _lib
    a = dict(GOOD, **bad)
    assert call_fit(a) == -1
    assert word in _lib.last_error(), _lib.last_error()
    if set(bad) <= SYSTEM_KEYS:
        assert call_system(a) == -1
        assert word in _lib.last_error(), _lib.last_error()
    if set(bad) <= PLAN_KEYS:
        assert call_plan(a) == -1
        assert word in _lib.last_error(), _lib.last_error()


def test_good_arguments_reach_the_pointer_check_and_the_plan():
    from mvpose import _lib
    assert call_fit(GOOD) == -1 and "null device pointer" in _lib.last_error()
    assert call_system(GOOD) == -1 and "null device pointer" in _lib.last_error()
    twelve = dict(GOOD, seg=sc.PAIRS17, seg_len=LEN)
    assert call_fit(twelve) == -1 and "null device pointer" in _lib.last_error()
    assert call_system(twelve) == -1 and "null device pointer" in _lib.last_error()
    used, n_chunks, nbytes = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int64(0)
    rc = _lib.lib.mvp_skeleton_fit_plan(100, 34, 17, 0, ctypes.byref(used), ctypes.byref(n_chunks), ctypes.byref(nbytes))
    f_used, f_chunks, f_bytes = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int64(0)
    _lib.lib.mvp_trajectory_fit_plan(100, 34, 0, ctypes.byref(f_used), ctypes.byref(f_chunks), ctypes.byref(f_bytes))
    assert rc == 0 and (used.value, n_chunks.value) == (f_used.value, f_chunks.value)
    # the trajectory fit's workspace, a third cost term per frame and the groups' state
    assert nbytes.value >= f_bytes.value + 100 * 34 * 8
