"""CPU: the numpy reference of the trajectory covariances (tests/traj_cov_ref.py) agrees with
itself on every case the GPU file uses, the conditions the GPU fit test relies on hold in the
reference, and the C-ABI argument and plan checks of mvp_trajectory_smooth_cov(_plan) and
mvp_trajectory_fit_cov(_plan) reject bad values before any device work (every device pointer is
NULL here, in the manner of test_trajectory_smooth.py)."""
import ctypes

import numpy as np
import pytest

import traj_cov_ref as cr
import traj_fit_ref as tf
import traj_smooth_ref as ts

SMOOTH, SMOOTH_PLAN = "mvp_trajectory_smooth_cov", "mvp_trajectory_smooth_cov_plan"
FIT, FIT_PLAN = "mvp_trajectory_fit_cov", "mvp_trajectory_fit_cov_plan"


# ------------------------------------------------------------------ the reference
@pytest.mark.parametrize("T", [2, 3, 7, 64])
def test_banded_equals_dense(T):
    c = ts.make_case(T, 4, seed=T, long_gap=9)
    c["valid"][:2, 1] = 1          # chain 1 keeps two clean frames whatever the knock-outs hit
    c["xyz"][:2, 1] = c["truth"][:2, 1].astype(np.float32)
    c["cov"][:2, 1] = np.eye(3, dtype=np.float32)
    W, _, obs = ts.weights(c["xyz"], c["cov"], c["valid"], 1.0, 0.01)
    ok = obs.sum(0) >= 2
    assert ok.any()
    for lam in (1e-2, 1.0, 1e4):
        d0, d1 = cr.dense_chains(W, lam, ok)
        b0, b1 = cr.banded(W, lam, ok)
        err = cr.norm_error(b0, b1, d0, d1)
        print(f"T={T} lam={lam}: banded vs dense {err:.3g}")
        assert err <= 1e-9
        assert np.isnan(d1[-1]).all() and np.isfinite(d1[:-1][:, ok]).all()
        # Σ_tt is symmetric positive definite, and |Σij| <= sqrt(Σii Σjj) also across the two frames
        assert np.allclose(d0[:, ok], d0[:, ok].swapaxes(-1, -2), rtol=0.0, atol=1e-12 * np.abs(d0[:, ok]).max())
        assert (np.linalg.eigvalsh(d0[:, ok]) > 0).all()
        s = np.sqrt(np.einsum("tpii->tpi", d0[:, ok]))
        assert (np.abs(d1[:-1][:, ok]) <= s[:-1, :, :, None] * s[1:, :, None, :] * (1 + 1e-12)).all()


@pytest.mark.parametrize("c", cr.SMOOTH_CASES, ids=cr.case_id)
def test_self_error_of_the_gpu_cases(c):
    """Two fp64 evaluations of the same inverse agree to 1e-9 normalised on every smoother case of
    the GPU file: the condition under which its 2^-23 bound means what it says.  (Measured: at most
    2.8e-12, at λ = 1e4.)"""
    s = cr.smooth_case(c)
    assert s["ok"].any()
    worst = max(cr.self_error(s["W"][:, p], c[3]) for p in range(c[1]) if s["ok"][p])
    print(f"{cr.case_id(c)}: self error {worst:.3g}")
    assert worst <= 1e-9


def test_self_error_of_the_long_case():
    """T = 4099 is too long for a dense inverse: banded against banded on the reversed chains."""
    s = cr.smooth_case(cr.LONG_CASE)
    assert s["ok"].all()
    err = cr.reversed_error(s["W"], cr.LONG_CASE[3], s["ok"])
    print(f"{cr.case_id(cr.LONG_CASE)}: forward vs reversed {err:.3g}")
    assert err <= 1e-9


@pytest.mark.parametrize("weights", ["conf", "heatmap"])
def test_fit_scene_conditions_hold_in_the_reference(weights):
    """What test_trajectory_cov_gpu.py asserts of the device over the single-view stretch holds, with
    room, for dense() on the numpy linearisation: the largest axis of Σ_tt within 5° of camera 0's
    ray through the joint in every frame of the stretch; its eigenvalue above every two-view frame's
    in every frame of the stretch, and above 10x in the frames at least FIT_EDGE frames from a
    two-view frame.  (Nearer to one, the prior ties the depth to that frame's: the first and last
    frame of the stretch reach about 4x, the ones next to them about 12x; from FIT_EDGE frames in, 21x
    to 58x.)"""
    import traj_cov_cases as cc
    sc = cc.fit_scene()
    w = {"conf": cc.tr.W_CONF, "heatmap": cc.tr.W_GAUSS}[weights]
    gauss = sc["gauss"] if weights == "heatmap" else None
    e = cc.FIT_EDGE
    for hub in cc.FIT_HUBERS:
        r = tf.fit(sc["kpts"], sc["cams"], [0, 1], sc["xyz0"], weights=w, gauss=gauss, lambda_smooth=cc.FIT_LAMBDA,
                   max_iter=30, tol=1e-6, huber_delta=hub, min_conf=0.0, cov_floor=1.0)
        assert (r["status"] & 0xC0 == 0).all()
        H, _, nviews, _ = tf.system(sc["kpts"], sc["cams"], [0, 1], r["xyz"], weights=w, gauss=gauss, huber_delta=hub)
        assert (nviews[cc.FIT_GAP[0]:cc.FIT_GAP[1], list(cc.FIT_LOST)] == 1).all()
        for p in cc.FIT_LOST:
            diag, _ = cr.dense(cr.full6(H[:, p]), cc.FIT_LAMBDA)
            angle, ratio = cc.stretch_figures(diag, r["xyz"][:, p], sc["cams"][0])
            print(f"{weights} huber {hub} joint {p}: angle <= {angle.max():.2f} deg, ratio {ratio.min():.1f} (edges) "
                  f"{ratio[e:-e].min():.1f} (inside) .. {ratio.max():.1f}")
            assert angle.max() <= 5.0 / 2          # with room: the device is held to 5
            assert ratio.min() > 1.0 * 2 and ratio[e:-e].min() > 10.0 * 1.1


# ------------------------------------------------------------------ the C-ABI argument checks
def _plan(fn, T, P, chunk):
    from mvpose import _lib
    used, n, b = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int64(-1)
    rc = getattr(_lib.lib, fn)(T, P, chunk, ctypes.byref(used), ctypes.byref(n), ctypes.byref(b))
    return rc, _lib.last_error(), used.value, n.value, b.value


def _smooth(T=10, P=3, lam=1.0, sigma0=1.0, cov_floor=0.0, chunk=0, ws_bytes=1 << 40, xyz=None, ws=None, out=None):
    from mvpose import _lib
    rc = _lib.lib.mvp_trajectory_smooth_cov(xyz, None, None, T, P, lam, sigma0, cov_floor, chunk, ws, ws_bytes, out,
                                            None, None, None)
    return rc, _lib.last_error()


def _fit(T=10, P=3, V=2, n_cams=2, nv=2, weights=1, min_conf=0.0, cov_floor=1.0, hub=0.0, lam=1.0, chunk=0,
         ws_bytes=1 << 40, ptr=None, out=None):
    from mvpose import _lib
    ci = (ctypes.c_int * 9)(*range(9))
    rc = _lib.lib.mvp_trajectory_fit_cov(ptr, T, P, V, ptr, n_cams, ci, nv, ptr, None, weights, None, min_conf,
                                         cov_floor, hub, lam, chunk, ptr, ws_bytes, out, None, None, None)
    return rc, _lib.last_error()


@pytest.mark.parametrize("kw,msg", [
    (dict(T=0), "T=0 "), (dict(T=-3), "T=-3 "), (dict(P=0), "P=0 "),
    (dict(lam=0.0), "lambda_smooth=0 "), (dict(lam=-2.0), "lambda_smooth=-2 "),
    (dict(lam=float("nan")), "lambda_smooth=nan "), (dict(lam=float("inf")), "lambda_smooth=inf "),
    (dict(sigma0=0.0), "sigma0=0 "), (dict(sigma0=float("nan")), "sigma0=nan "),
    (dict(cov_floor=-1.0), "cov_floor=-1 "), (dict(cov_floor=float("nan")), "cov_floor=nan "),
    (dict(chunk=3), "chunk=3 "), (dict(chunk=-1), "chunk=-1 "), (dict(chunk=4097), "chunk=4097 "),
    (dict(ws_bytes=16), "workspace_bytes=16 "),
])
def test_smooth_cov_argument_checks(kw, msg):
    rc, err = _smooth(**kw)
    assert rc == -1
    assert err.startswith(SMOOTH + ": "), err
    assert msg in err, err


@pytest.mark.parametrize("kw,msg", [
    (dict(T=0), "T=0"), (dict(P=0), "P=0"), (dict(T=65536, P=32768), "2^31"), (dict(nv=1), "n_cam_idx=1"),
    (dict(nv=9, n_cams=8, V=9), "n_cam_idx=9"), (dict(lam=0.0), "lambda_smooth"), (dict(lam=float("inf")), "lambda_smooth"),
    (dict(lam=float("nan")), "lambda_smooth"), (dict(cov_floor=-1.0), "cov_floor"), (dict(cov_floor=float("nan")), "cov_floor"),
    (dict(min_conf=float("nan")), "min_conf"), (dict(hub=float("nan")), "huber_delta"), (dict(chunk=3), "chunk"),
    (dict(chunk=5000), "chunk"), (dict(weights=3), "weights"), (dict(weights=2), "gauss"),
    (dict(ws_bytes=16), "workspace_bytes=16 "),
])
def test_fit_cov_argument_checks(kw, msg):
    rc, err = _fit(**kw)
    assert rc == -1
    assert err.startswith(FIT + ": "), err
    assert msg in err, err


def test_null_pointers():
    """out_cov is required; nothing is dereferenced (the check comes before any launch)."""
    buf = ctypes.c_void_p(4096)
    rc, err = _smooth()
    assert rc == -1 and err == SMOOTH + ": null device pointer", err
    rc, err = _smooth(xyz=buf, ws=buf, out=None)
    assert rc == -1 and err == SMOOTH + ": null device pointer", err
    rc, err = _fit()
    assert rc == -1 and err == FIT + ": null device pointer", err
    rc, err = _fit(ptr=buf, out=None)
    assert rc == -1 and err == FIT + ": null device pointer", err


@pytest.mark.parametrize("fn", [SMOOTH_PLAN, FIT_PLAN])
@pytest.mark.parametrize("kw,msg", [(dict(T=0, P=3, chunk=0), "T=0 "), (dict(T=5, P=0, chunk=0), "P=0 "),
                                    (dict(T=5, P=3, chunk=2), "chunk=2 "), (dict(T=5, P=3, chunk=5000), "chunk=5000 ")])
def test_plan_argument_checks(fn, kw, msg):
    rc, err, *_ = _plan(fn, **kw)
    assert rc == -1 and err.startswith(fn + ": ") and msg in err, err


@pytest.mark.parametrize("T,P,chunk", [(1, 1, 0), (5, 3, 4), (6, 3, 4), (7, 3, 4), (300, 17, 32), (4099, 17, 0)])
def test_plans_are_consistent(T, P, chunk):
    """The chunking is the solver's; the workspace is the mirrored call's plus 6 doubles per eliminated
    frame and lane (the pivots) and 57 per separator and chain (the reduced system's Σ); one byte
    less is refused, the exact size passes on to the pointer check."""
    for plan, base, call, fn in ((SMOOTH_PLAN, "mvp_trajectory_smooth_plan", _smooth, SMOOTH),
                                 (FIT_PLAN, "mvp_trajectory_fit_plan", _fit, FIT)):
        rc, err, used, n, nbytes = _plan(plan, T, P, chunk)
        rc0, _, used0, n0, nbytes0 = _plan(base, T, P, chunk)
        assert rc == 0 and rc0 == 0, err
        assert (used, n) == (used0, n0) and n == -(-T // (used + 2))
        n_seps = (T - used - 1) // (used + 2) + 1 if T > used else 0
        lanes64 = -(-(P * n) // 64) * 64
        extra = 6 * 8 * min(T, used) * lanes64 + 57 * 8 * n_seps * P
        assert nbytes0 + extra <= nbytes <= nbytes0 + extra + 2 * 256      # two arrays, each rounded up to 256 bytes
        rc, err = call(T=T, P=P, chunk=chunk, ws_bytes=nbytes - 1)
        assert rc == -1 and f"workspace_bytes={nbytes - 1} " in err, err
        rc, err = call(T=T, P=P, chunk=chunk, ws_bytes=nbytes)
        assert rc == -1 and err == fn + ": null device pointer", err


def test_the_solver_plans_are_unchanged():
    """The byte counts mvp_trajectory_smooth_plan and mvp_trajectory_fit_plan reported before the
    covariance calls existed (the pivots live in the new calls' workspace only)."""
    assert _plan("mvp_trajectory_smooth_plan", 300, 17, 32)[2:] == (32, 9, 2130944)
    assert _plan("mvp_trajectory_smooth_plan", 4099, 17, 0)[2:] == (80, 50, 23479296)
    assert _plan("mvp_trajectory_fit_plan", 300, 17, 32)[2:] == (32, 9, 2826752)
    assert _plan("mvp_trajectory_fit_plan", 4099, 17, 0)[2:] == (80, 50, 32962304)
