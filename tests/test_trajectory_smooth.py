"""CPU: the numpy restatement of mvp_trajectory_smooth agrees with itself and with the
contract's consequences, and the C-ABI argument checks of mvp_trajectory_smooth /
mvp_trajectory_smooth_plan reject bad values before any device work (every device pointer is NULL
here, in the manner of test_triangulate_args.py)."""
import ctypes

import numpy as np
import pytest

import traj_smooth_ref as ref
from test_cli import REF_FLAGS, _dests

FN = "mvp_trajectory_smooth"
PLAN = "mvp_trajectory_smooth_plan"


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("T", [2, 3, 7, 64])
def test_banded_equals_dense(T):
    c = ref.make_case(T, 4, seed=T, long_gap=9)
    c["valid"][:2, 1] = 1          # chain 1 keeps two clean frames whatever the knock-outs hit
    c["xyz"][:2, 1] = c["truth"][:2, 1].astype(np.float32)
    c["cov"][:2, 1] = np.eye(3, dtype=np.float32)
    for lam in (1e-2, 1.0, 1e2):
        a = ref.solve_dense(c["xyz"], c["cov"], c["valid"], lambda_smooth=lam, cov_floor=0.01)
        b = ref.solve_banded(c["xyz"], c["cov"], c["valid"], lambda_smooth=lam, cov_floor=0.01)
        assert np.array_equal(a.status, b.status) and np.array_equal(a.observed, b.observed)
        assert (a.status == 0).any()
        ok = a.status == 0
        err = np.abs(a.x64[:, ok] - b.x64[:, ok]).max()
        print(f"T={T} lam={lam}: banded vs dense {err:.3g}")
        assert err <= 1e-8
        np.testing.assert_allclose(a.resid, b.resid, rtol=1e-7, atol=1e-9, equal_nan=True)
        assert np.array_equal(a.xyz[:, ~ok].view(np.uint32), c["xyz"][:, ~ok].view(np.uint32))


@pytest.mark.parametrize("lam", [1e-2, 1.0, 1e4])
@pytest.mark.parametrize("solver", [ref.solve_dense, ref.solve_banded])
def test_affine_data_are_returned(lam, solver):
    T, P = 48, 3
    t = np.arange(T, dtype=np.float64)[:, None, None]
    slope = np.array([[0.5, -0.25, 2.0], [1.0, 0.125, -0.75], [0.0, 3.0, 0.375]])      # dyadic
    off = np.array([[3.0, -7.0, 100.0], [0.0, 12.0, -5.0], [40.0, 1.0, 2.0]])            # integer
    xyz = (off + slope * t).astype(np.float32)
    assert np.array_equal(xyz.astype(np.float64), off + slope * t)
    cov = ref.make_case(T, P, seed=1, knock=0.0)["cov"]
    valid = np.ones((T, P), np.uint8)
    valid[5:17, 0] = 0
    valid[:4, 1] = 0
    valid[-6:, 2] = 0
    r = solver(xyz, cov, valid, lambda_smooth=lam)
    assert (r.status == 0).all()
    err = np.abs(r.x64 - (off + slope * t)).max()
    print(f"lam={lam}: affine error {err:.3g}")
    assert err <= 1e-8
    assert np.nanmax(r.resid) <= 1e-12


@pytest.mark.parametrize("solver", [ref.solve_dense, ref.solve_banded])
def test_two_observed_frames_give_their_line(solver):
    T = 40
    rng = np.random.default_rng(3)
    xyz = rng.normal(size=(T, 1, 3)).astype(np.float32) * 50
    valid = np.zeros((T, 1), np.uint8)
    valid[11], valid[29] = 1, 1
    r = solver(xyz, None, valid, lambda_smooth=1.0, sigma0=0.5)
    assert r.status[0] == 0
    a, b = xyz[11, 0].astype(np.float64), xyz[29, 0].astype(np.float64)
    line = a + (np.arange(T)[:, None] - 11) / 18.0 * (b - a)
    err = np.abs(r.x64[:, 0] - line).max()
    print(f"two frames: line error {err:.3g}")
    assert err <= 1e-8


@pytest.mark.parametrize("solver", [ref.solve_dense, ref.solve_banded])
def test_chains_with_0_and_1_observed_frames_fail(solver):
    c = ref.make_case(20, 3, seed=5)
    c["valid"][:, 0] = 0
    c["valid"][:, 1] = 0
    c["valid"][7, 1] = 1
    c["xyz"][7, 1] = 1.0
    c["cov"][7, 1] = np.eye(3, dtype=np.float32)
    r = solver(c["xyz"], c["cov"], c["valid"])
    assert list(r.status) == [0x80, 0x80, 0]
    assert np.isnan(r.resid[:, :2]).all()
    assert np.array_equal(r.xyz[:, :2].view(np.uint32), c["xyz"][:, :2].view(np.uint32))
    assert np.isfinite(r.xyz[:, 2]).all()


def test_gap_mask_and_huber_loop():
    obs = np.ones((12, 2), bool)
    obs[:3, 0] = False
    obs[5:7, 0] = False
    obs[9:, 1] = False
    m = ref.gap_mask(obs, 2)
    assert m[:3, 0].all() and not m[3:, 0].any() and m[9:, 1].all() and not m[:9, 1].any()
    # the loop down-weights a displaced frame
    T = 60
    t = np.arange(T)
    xyz = np.stack([0.1 * t, np.zeros(T), np.ones(T)], -1)[:, None, :].astype(np.float32)
    xyz[30, 0] += 30
    plain, _ = ref.smooth_trajectory(xyz, sigma0=0.5, lambda_smooth=10.0)
    robust, res = ref.smooth_trajectory(xyz, sigma0=0.5, lambda_smooth=10.0, robust_k=3.0)
    truth = xyz.copy()
    truth[30, 0] -= 30
    assert np.abs(robust - truth).max() < 0.25 * np.abs(plain - truth).max()
    assert res.resid[30, 0] > 100


# ------------------------------------------------------------------ the C-ABI argument checks
def _plan(T, P, chunk):
    from mvpose import _lib
    used, n, b = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int64(-1)
    rc = _lib.lib.mvp_trajectory_smooth_plan(T, P, chunk, ctypes.byref(used), ctypes.byref(n), ctypes.byref(b))
    return rc, _lib.last_error(), used.value, n.value, b.value


def _call(T=10, P=3, lam=1.0, sigma0=1.0, cov_floor=0.0, chunk=0, ws_bytes=1 << 40, xyz=None, ws=None, out=None):
    from mvpose import _lib
    rc = _lib.lib.mvp_trajectory_smooth(xyz, None, None, T, P, lam, sigma0, cov_floor, chunk, ws, ws_bytes, out, None,
                                        None, None, None)
    return rc, _lib.last_error()


@pytest.mark.parametrize("kw,msg", [
    (dict(T=0), "T=0 "),
    (dict(T=-3), "T=-3 "),
    (dict(P=0), "P=0 "),
    (dict(lam=0.0), "lambda_smooth=0 "),
    (dict(lam=-2.0), "lambda_smooth=-2 "),
    (dict(lam=float("nan")), "lambda_smooth=nan "),
    (dict(lam=float("inf")), "lambda_smooth=inf "),
    (dict(sigma0=0.0), "sigma0=0 "),
    (dict(sigma0=float("nan")), "sigma0=nan "),
    (dict(sigma0=float("inf")), "sigma0=inf "),
    (dict(cov_floor=-1.0), "cov_floor=-1 "),
    (dict(cov_floor=float("nan")), "cov_floor=nan "),
    (dict(chunk=3), "chunk=3 "),
    (dict(chunk=-1), "chunk=-1 "),
    (dict(chunk=4097), "chunk=4097 "),
    (dict(ws_bytes=16), "workspace_bytes=16 "),
])
def test_argument_checks(kw, msg):
    rc, err = _call(**kw)
    assert rc == -1
    assert err.startswith(FN + ": "), err
    assert msg in err, err


def test_null_and_aliased_pointers():
    rc, err = _call()
    assert rc == -1 and err == FN + ": null device pointer", err
    buf = ctypes.c_void_p(4096)     # never dereferenced: the alias check comes before any launch
    rc, err = _call(xyz=buf, ws=ctypes.c_void_p(8192), out=buf)
    assert rc == -1 and err.startswith(FN + ": ") and "out_xyz must not alias xyz" in err, err


@pytest.mark.parametrize("kw,msg", [(dict(T=0, P=3, chunk=0), "T=0 "), (dict(T=5, P=0, chunk=0), "P=0 "),
                                    (dict(T=5, P=3, chunk=2), "chunk=2 "), (dict(T=5, P=3, chunk=5000), "chunk=5000 ")])
def test_plan_argument_checks(kw, msg):
    rc, err, *_ = _plan(**kw)
    assert rc == -1 and err.startswith(PLAN + ": ") and msg in err, err


@pytest.mark.parametrize("T,P,chunk", [(1, 1, 0), (5, 3, 4), (6, 3, 4), (7, 3, 4), (300, 17, 32), (4099, 17, 0),
                                       (100000, 17, 0), (100000, 17, 4096)])
def test_plan_is_consistent(T, P, chunk):
    rc, err, used, n, nbytes = _plan(T, P, chunk)
    assert rc == 0, err
    assert 4 <= used <= 4096 and (chunk == 0 or used == chunk)
    assert n == -(-T // (used + 2))          # chunks of `used` interior frames + a 2-frame separator
    assert nbytes > 0
    # the factor alone: 39 doubles per eliminated frame and lane
    assert nbytes >= 39 * 8 * min(T, used) * n * P
    rc, err = _call(T=T, P=P, chunk=chunk, ws_bytes=nbytes - 1)
    assert rc == -1 and f"workspace_bytes={nbytes - 1} " in err, err
    rc, err = _call(T=T, P=P, chunk=chunk, ws_bytes=nbytes)
    assert rc == -1 and err == FN + ": null device pointer", err


def test_refinement_parser_extensions():
    from mvpose import cli
    assert _dests(cli.pose_refinement_parser()) == REF_FLAGS
    assert _dests(cli.pose_refinement_parser(extensions=True)) == REF_FLAGS + ["kpts_3d_cov", "kpts_3d_refine_status"]
