"""CPU: the fp64 numpy restatement of the trajectory fit with sub-frame camera offsets
(tests/traj_fit_lag_ref.py, written from the text in include/mvpose.h) checked on its own, the scene
the offsets were built for, the decision margins of the cases the GPU tests compare, and the
argument checks of the three C entry points."""
import ctypes

import numpy as np
import pytest

import traj_fit_cases as tc
import traj_fit_lag_cases as lc
import traj_fit_lag_ref as tl
import traj_fit_ref as tf
import tri_refine_ref as tr
from mvpose import synthetic as syn

FRACS = {"zero": (0.0, 0.0, 0.0), "0.4": (0.4, 0.4, 0.4), "mixed": (0.0, 0.4, 0.75)}


def small_chain(hub, frac, weights=tr.W_CONF, lam=0.7, T=6, seed=4):
    """test_trajectory_fit.py's chain (frames seen by 3, 3, 2, 1, 0, 3 views) with offsets."""
    rng = np.random.default_rng(seed)
    cams = syn.make_rig(3, seed=3)
    truth = syn.make_poses(T, seed=seed, jitter=1.0)[:, :1]
    kpts = syn.make_kpts_2d(truth, cams, seed=seed + 1, noise_px=2.0)
    kpts[2, 0, 0, 1] = np.nan
    kpts[3, 0, 0, 1] = kpts[3, 0, 0, 2] = np.nan
    kpts[4, 0, 0, :] = np.nan
    used, z, W = tf.views(kpts, [0, 1, 2], None, weights, None, 0.0, 1.0)
    X = truth[:, 0] + rng.normal(0.0, 1.0, (T, 3))
    return tl.Chain(cams, [0, 1, 2], used[:, 0], z[:, 0], W[:, 0], hub, lam, frac), X


def central(f, x, h=1e-4):
    g = np.zeros(x.size)
    for k in range(x.size):
        e = np.zeros(x.size)
        e[k] = h
        g[k] = (f(x + e) - f(x - e)) / (2 * h)
    return g


@pytest.mark.parametrize("name", list(FRACS))
@pytest.mark.parametrize("hub", [0.0, 1.5])
def test_gradient_matches_central_differences(hub, name):
    """G = g̃ + λ·D₂ᵀD₂·X is the gradient of the chain's cost."""
    ch, X = small_chain(hub, FRACS[name])
    _, G = ch.linearise(X)
    num = central(lambda x: ch.cost(x.reshape(X.shape))[0], X.ravel())
    err = np.abs(G - num).max() / np.abs(G).max()
    print(f"hub {hub} frac {name}: gradient rel err {err:.3g}")
    assert err < 1e-7


@pytest.mark.parametrize("name", list(FRACS))
@pytest.mark.parametrize("hub", [0.0, 1.5])
def test_blocks_match_central_differences(hub, name):
    """H̃_t and C_t against Σ over the observations of (∂Y/∂X_t)ᵀ Jᵀ W̃ J (∂Y/∂X_s), with J from
    central differences of the forward model at Y; nothing else lies off the diagonal but λ·D₂ᵀD₂."""
    ch, X = small_chain(hub, FRACS[name])
    a = ch.a
    A, _ = ch.linearise(X)
    T = X.shape[0]
    h = 1e-4
    want = np.zeros((3 * T, 3 * T))
    for t in range(T):
        for i, col in enumerate(ch.cam_idx):
            if not ch.used[t, i]:
                continue
            Y = X[t] if a[i] == 0 else (1 - a[i]) * X[t] + a[i] * X[t + 1]
            J = np.stack([(syn.project(Y + h * e, ch.cams[col]) - syn.project(Y - h * e, ch.cams[col])) / (2 * h)
                          for e in np.eye(3)], 1)
            r = syn.project(Y, ch.cams[col]) - ch.z[t, i]
            s = np.sqrt(r @ ch.W[t, i] @ r)
            om = 1.0 if not (hub > 0 and s > hub) else hub / s
            Hi = J.T @ (om * ch.W[t, i]) @ J
            w = {t: 1 - a[i]}
            if a[i] > 0:
                w[t + 1] = a[i]
            for t1, w1 in w.items():
                for t2, w2 in w.items():
                    want[3 * t1:3 * t1 + 3, 3 * t2:3 * t2 + 3] += w1 * w2 * Hi
    got = A - ch.lam * ch.K3
    assert np.abs(got - want).max() <= 1e-7 * np.abs(want).max()
    assert np.abs(got - got.T).max() <= 1e-12 * np.abs(got).max()
    if name != "zero":
        assert np.abs(got[0:3, 3:6]).max() > 0                        # the pair's block is there
    assert np.array_equal(ch.used.sum(1), [3, 3, 2, 1, 0, 3 if name == "zero" else 1 if name == "mixed" else 0])


@pytest.mark.parametrize("name", list(FRACS))
@pytest.mark.parametrize("hub", [0.0, 1.5])
def test_offset_derivative_matches_central_differences(hub, name):
    """ga[i] is the derivative of the chain's cost with respect to a_i at fixed X.  At a_i = 0 the
    central difference would leave [0, 1): a one-sided third-order difference stands in, and the
    last frame, which a view loses when its offset becomes positive, is taken out by hand.  Bound
    1e-7 relative for every view."""
    ch, X = small_chain(hub, FRACS[name])
    ga = ch.dlag(X)[:, 0]
    h = 1e-4

    def cost_at(i, ai):
        a = ch.a.copy()
        a[i] = ai
        used = ch.used.copy()
        if ch.a[i] == 0:
            used[-1, i] = False        # compare like with like
        return tl.Chain(ch.cams, ch.cam_idx, used, ch.z, ch.W, ch.hub, ch.lam, a).cost(X)[0]
    for i in range(3):
        if ch.a[i] == 0:
            num = (-11 * cost_at(i, 0.0) + 18 * cost_at(i, h) - 9 * cost_at(i, 2 * h) + 2 * cost_at(i, 3 * h)) / (6 * h)
        else:
            num = (cost_at(i, ch.a[i] + h) - cost_at(i, ch.a[i] - h)) / (2 * h)
        err = abs(ga[i] - num) / np.abs(ga).max()
        print(f"hub {hub} frac {name} view {i}: ga {ga[i]:.6g} numeric {num:.6g} rel err {err:.3g}")
        assert err < 1e-7


def test_ha_is_the_gauss_newton_curvature():
    ch, X = small_chain(0.0, FRACS["mixed"])
    _, _, H, g, _ = ch.terms(X)
    D = X[1:] - X[:-1]
    for i in range(3):
        want = sum(D[t] @ H[t, i] @ D[t] for t in range(5) if ch.used[t, i])
        assert np.isclose(ch.dlag(X)[i, 1], want, rtol=1e-12)
    assert (ch.dlag(X)[:, 1] > 0).all()


@pytest.mark.parametrize("i", [3, 6, 7, 9])
def test_zero_offsets_equal_the_plain_restatement_bit_for_bit(i):
    """With every a_i = 0 the system and the fit are traj_fit_ref's, on its own cases."""
    c = tc.case(i)
    zero = np.zeros(len(c["cam_idx"]))
    H0, g0, nv0, cost0 = tc.reference_system(i)
    H, C, g, nv, cost, _ = tl.system(c["kpts"], c["cams"], c["cam_idx"], zero, c["xyz0"], **c["kw"])
    assert np.array_equal(H, H0, equal_nan=True) and np.array_equal(g, g0, equal_nan=True)
    assert np.array_equal(nv, nv0) and np.array_equal(cost, cost0, equal_nan=True) and not C.any()
    r0 = tc.reference_fit(i)
    r = tl.fit(c["kpts"], c["cams"], c["cam_idx"], zero, c["xyz0"], lambda_smooth=c["lam"], max_iter=c["max_iter"],
               tol=tc.TOL, **c["kw"])
    for k in ("X", "xyz", "resid", "nviews", "cost", "status", "rejected"):
        assert np.array_equal(r[k], r0[k], equal_nan=True), k
    assert r["margins"] == r0["margins"]


def test_system_is_the_chain_linearisation():
    """tl.system (all chains at once, the _system entry point's layout) against tl.Chain."""
    i, p = 7, 3
    c = lc.case(i)
    H6, C6, g, nviews, cost, dlag = lc.reference_system(i)
    used, z, W = tf.views(c["kpts"], c["cam_idx"], c["kw"]["mask_bits"], c["kw"]["weights"], None, lc.MIN_CONF, 1.0)
    ch = tl.Chain(c["cams"], c["cam_idx"], used[:, p], z[:, p], W[:, p], c["kw"]["huber_delta"], 1.0, c["frac"])
    X = c["xyz0"][:, p].astype(np.float64)
    A, G = ch.linearise(X)
    B = A - ch.K3
    iu = np.triu_indices(3)
    for t in range(X.shape[0]):
        assert np.allclose(B[3 * t:3 * t + 3, 3 * t:3 * t + 3][iu], H6[t, p], rtol=1e-12, atol=0)
        if t + 1 < X.shape[0]:
            assert np.allclose(B[3 * t:3 * t + 3, 3 * t + 3:3 * t + 6][iu], C6[t, p], rtol=1e-12, atol=0)
    assert not C6[-1].any()
    assert np.allclose(G - ch.K3 @ X.ravel(), g[:, p].ravel(), rtol=1e-12, atol=1e-9)
    assert np.isclose(cost[p].sum(), ch.cost(X)[0], rtol=1e-12)
    assert np.array_equal(nviews[:, p], ch.used.sum(1))
    assert np.allclose(dlag[p], ch.dlag(X), rtol=1e-12)


def test_accuracy_scene():
    """make_rig(3, seed=3), four joints on 40 x 30 cm ellipses at 1 Hz, views 1 and 2 planted 0.4 and
    0.75 of a frame late, 1 px noise.  The fit that takes the views of a frame for one instant is
    several times further off than the fit with the planted offsets, and the offset search of
    sync.refine_frame_offsets, run on the restatement from (0.3, 0.3), finds them."""
    rms0, rms1, s, info = lc.scene_reference()
    print(f"RMS error: zero offsets {rms0:.3f} cm, planted offsets {rms1:.3f} cm, ratio {rms0 / rms1:.2f}; recovered "
          f"{s[1]:.4f}, {s[2]:.4f} (planted {lc.SCENE_FRAC[1:]}) in {len(info['step'])} rounds, steps {info['step']}, "
          f"costs {info['cost']}")
    assert abs(rms0 - lc.SCENE_RMS_ZERO) < 0.02 and abs(rms1 - lc.SCENE_RMS_TRUE) < 0.01
    assert np.abs(s[1:] - lc.SCENE_RECOVERED).max() < 2e-3 and s[0] == 0
    # the asked-for properties, on the restatement itself
    assert rms0 / rms1 >= 0.5 * lc.SCENE_RMS_ZERO / lc.SCENE_RMS_TRUE
    dev = np.abs(np.array(lc.SCENE_RECOVERED) - lc.SCENE_FRAC[1:])
    assert (np.abs(s[1:] - lc.SCENE_FRAC[1:]) <= 2 * dev).all()
    assert info["cost"][-1] < info["cost"][0]


@pytest.mark.parametrize("i", range(len(lc.CASES)), ids=[lc.case_id(kw) for kw in lc.CASES])
def test_decision_margins_of_the_gpu_cases(i):
    """Every accept and convergence comparison of the restatement's run has a relative margin above
    1e-6, so that fp64 rounding cannot flip it on the device."""
    r = lc.reference_fit(i)
    m = min(r["margins"]) if r["margins"] else np.inf
    print(f"{lc.case_id(lc.CASES[i])}: {len(r['margins'])} comparisons, smallest margin {m:.3g}; "
          f"status {sorted(set(hex(s) for s in r['status']))}")
    assert m > 1e-6


def test_cases_reach_their_paths():
    """The patterns the GPU cases are there for do occur in them."""
    st = [lc.reference_fit(i)["status"] for i in range(len(lc.CASES))]
    nv = [lc.reference_fit(i)["nviews"] for i in range(len(lc.CASES))]
    assert st[0].tolist() == [tl.INVALID]                               # T = 1
    assert st[1][2] == tl.INVALID and (st[1][:2] & 0xC0 == 0).all()     # T = 2: two views without an offset; starved
    assert (nv[1][1] <= 2).all() and (nv[2][2] <= 1).all()              # the last frame loses the views with an offset
    assert st[3][3] == tl.INVALID                                       # NaN seed frame
    assert st[5][1] == tl.INVALID                                       # behind its camera at its Y
    c = lc.case(5)
    assert np.isfinite(c["xyz0"][:, 1]).all()
    assert [st[8][p] for p in (20, 33, 64)] == [tl.INVALID] * 3
    assert (nv[7][4:9, 2] == 0).all() and (nv[8][3:8, 7] == 0).all()    # blind stretches
    assert (nv[8][15:25, 0] <= 1).all() and (nv[8][15:25, 0] == 1).sum() >= 5          # single-view stretch
    for i in (3, 7, 9):
        assert (nv[i] < lc.CASES[i]["nv"]).mean() > 0.2                 # random drops
    valid = np.concatenate([s[s != tl.INVALID] for s in st[:lc.ROUGH]])
    assert (valid & 0x40 == 0).all() and (valid & 63).max() <= lc.MAX_ITER
    rough = lc.reference_fit(lc.ROUGH)
    assert rough["rejected"].tolist() == [5, 0, 0, 0, 3] and st[lc.ROUGH].tolist() == [0x0B, 0x80, 0x04, 0x06, 0x4C]
    ok = rough["status"] != tl.INVALID
    assert (rough["cost"][ok, 1] < rough["cost"][ok, 0]).all()


def test_rough_case_is_well_conditioned():
    """The rough-seed case can be compared to a float32 ulp only if the restatement itself is
    reproducible there: lambda changed by 1e-13 of itself must move no coordinate by more than
    1e-10 cm (half a float32 ulp of 300 cm is 1.5e-5 cm), and no cost may be astronomic."""
    c, r = lc.case(lc.ROUGH), lc.reference_fit(lc.ROUGH)
    worst = 0.0
    for eps in (1e-13, -1e-13):
        r2 = tl.fit(c["kpts"], c["cams"], c["cam_idx"], c["frac"], c["xyz0"], lambda_smooth=c["lam"] * (1 + eps),
                    max_iter=c["max_iter"], tol=lc.TOL, **c["kw"])
        assert np.array_equal(r2["status"], r["status"])
        worst = max(worst, float(np.abs(r2["X"] - r["X"]).max()))
    print(f"largest move of a coordinate under lambda·(1 ± 1e-13): {worst:.3g} cm; largest cost {np.nanmax(r['cost']):.3g}")
    assert worst <= 1e-10 and np.nanmax(r["cost"]) < 1e9


def test_python_fronts_refuse_what_they_cannot_do():
    """Host checks that come before any device work: with_cov together with frame_offsets, and a
    frac that does not hold one offset per listed view."""
    from mvpose import ops, refine
    k, x0 = np.zeros((4, 2, 3, 3), np.float32), np.zeros((4, 2, 3), np.float32)
    params = syn.reference_camera_params(syn.make_rig(3, seed=3))
    with pytest.raises(ValueError, match="with_cov"):
        refine.fit_trajectory(k, params, x0, frame_offsets=(0.0, 0.4, 0.75), return_info=True, with_cov=True)
    args = tuple(range(15))
    with pytest.raises(ValueError, match="one offset per listed view"):
        ops._lag_args(args, (0.0, 0.4), 3)
    out = ops._lag_args(args, (0.0, 0.4, 0.75), 3)
    assert out[:8] == args[:8] and out[9:] == args[8:] and list(out[8]) == [0.0, 0.4, 0.75]


def test_refine_frame_offsets_checks_its_shapes():
    from mvpose import sync
    params = syn.reference_camera_params(syn.make_rig(3, seed=3))
    with pytest.raises(ValueError, match="one column per camera"):
        sync.refine_frame_offsets(np.zeros((4, 2, 3, 2), np.float32), params, np.zeros((4, 2, 3)), (0.0, 0.1, 0.2))
    with pytest.raises(ValueError, match="one offset per camera"):
        sync.refine_frame_offsets(np.zeros((4, 2, 3, 3), np.float32), params, np.zeros((4, 2, 3)), (0.0, 0.1))


def test_split_frame_offsets():
    from mvpose import sync
    n, a = sync.split_frame_offsets([0.0, 2.4, -0.25, -3.0, 5.0 - 1e-17])
    assert n.tolist() == [0, 2, -1, -3, 5] and np.allclose(a, [0.0, 0.4, 0.75, 0.0, 0.0])
    assert n.dtype == np.int64 and ((a >= 0) & (a < 1)).all()
    with pytest.raises(ValueError):
        sync.split_frame_offsets([0.0, np.nan])


# ------------------------------------------------------------------ the C entry points' argument checks
GOOD = dict(T=10, P=17, V=3, n_cams=3, nv=3, frac=(0.0, 0.4, 0.75), weights=1, gauss=None, min_conf=0.0, cov_floor=1.0,
            hub=0.0, lam=1.0, max_iter=10, tol=1e-6, chunk=0, ws_bytes=1 << 40)
BAD = [
    (dict(T=0), "T=0"), (dict(P=0), "P=0"), (dict(T=65536, P=32768), "2^31"),
    (dict(nv=1), "n_cam_idx=1"), (dict(nv=9, n_cams=8, V=9), "n_cam_idx=9"),
    (dict(frac=None), "frac"), (dict(frac=(0.0, 1.0, 0.5)), "frac"), (dict(frac=(0.0, 0.5, -1e-9)), "frac"),
    (dict(frac=(float("nan"), 0.0, 0.0)), "frac"), (dict(frac=(0.0, float("inf"), 0.0)), "frac"),
    (dict(frac=(0.0, 0.0, -float("inf"))), "frac"),
    (dict(lam=0.0), "lambda_smooth"), (dict(lam=float("inf")), "lambda_smooth"), (dict(lam=float("nan")), "lambda_smooth"),
    (dict(tol=0.0), "tol"), (dict(tol=float("nan")), "tol"), (dict(cov_floor=-1.0), "cov_floor"),
    (dict(cov_floor=float("nan")), "cov_floor"), (dict(min_conf=float("nan")), "min_conf"),
    (dict(hub=float("nan")), "huber_delta"), (dict(max_iter=64), "max_iter"), (dict(max_iter=-1), "max_iter"),
    (dict(chunk=3), "chunk"), (dict(weights=3), "weights"), (dict(weights=2), "gauss"), (dict(ws_bytes=16), "workspace_bytes"),
]
SYSTEM_KEYS = {"T", "P", "V", "n_cams", "nv", "frac", "weights", "min_conf", "cov_floor", "hub"}


def frac_arg(a):
    return None if a["frac"] is None else (ctypes.c_double * 9)(*(list(a["frac"]) + [0.0] * (9 - len(a["frac"]))))


def call_fit(a):
    from mvpose import _lib
    ci = (ctypes.c_int * 9)(*range(9))
    return _lib.lib.mvp_trajectory_fit_lag(None, a["T"], a["P"], a["V"], None, a["n_cams"], ci, a["nv"], frac_arg(a), None,
                                           None, a["weights"], a["gauss"], a["min_conf"], a["cov_floor"], a["hub"],
                                           a["lam"], a["max_iter"], a["tol"], a["chunk"], None, a["ws_bytes"], None, None,
                                           None, None, None, None, None)


def call_system(a):
    from mvpose import _lib
    ci = (ctypes.c_int * 9)(*range(9))
    return _lib.lib.mvp_trajectory_fit_lag_system(None, a["T"], a["P"], a["V"], None, a["n_cams"], ci, a["nv"],
                                                  frac_arg(a), None, None, a["weights"], a["gauss"], a["min_conf"],
                                                  a["cov_floor"], a["hub"], None, None, None, None, None, None, None)


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
    rc = _lib.lib.mvp_trajectory_fit_lag_plan(100, 17, 0, ctypes.byref(used), ctypes.byref(n_chunks), ctypes.byref(nbytes))
    f_used, f_chunks, f_bytes = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int64(0)
    _lib.lib.mvp_trajectory_fit_plan(100, 17, 0, ctypes.byref(f_used), ctypes.byref(f_chunks), ctypes.byref(f_bytes))
    assert rc == 0 and (used.value, n_chunks.value) == (f_used.value, f_chunks.value)
    # the plain fit's workspace, the blocks between neighbouring frames, the offset derivative's tile sums
    assert nbytes.value >= f_bytes.value + 100 * 17 * 8 * 6 + 17 * 8 * 2 * 8
    assert _lib.lib.mvp_trajectory_fit_lag_plan(0, 17, 0, None, None, None) == -1
    assert _lib.lib.mvp_trajectory_fit_lag_plan(100, 17, 5000, None, None, None) == -1
