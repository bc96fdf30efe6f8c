"""GPU: mvp_trajectory_smooth (csrc/smooth.hip) against the fp64 numpy restatement
tests/traj_smooth_ref.py, through mvpose.ops.trajectory_smooth and its fronts.

Inputs (traj_smooth_ref.make_case): ground truth (100 + 50 sin(t/9), 200 + 30 cos(t/13),
900 + 0.2 t) plus a per-chain offset, noise from a random rotation with per-axis σ in [0.05, 2],
the true covariances rounded to float32 and symmetrised, 20 % of the frames knocked out (NaN xyz,
NaN covariance, a covariance with a negative eigenvalue, valid = 0), one gap longer than a whole
chunk; |coordinates| < 1024.

Bounds.  Both sides solve the same fp64 system from the same float32 inputs.  xyz within 1e-4 world
units: partitioned and dense fp64 solutions agree to ~1e-7, so the two float32 roundings differ by
at most one ulp, 6.1e-5 below 1024.  resid within rtol 1e-4 + atol 1e-5: a 1e-7 shift in X moves a
residual of order 10 by about 1e-5 at the smallest σ.  Measured on an MI355X: every float32 xyz
equal to the restatement's in every case, resid relative error <= 6e-8."""
import functools
import os

import numpy as np
import pytest
import torch
import yaml

import traj_smooth_ref as ref

pytestmark = pytest.mark.gpu
XYZ_ATOL = 1e-4
RESID_RTOL, RESID_ATOL = 1e-4, 1e-5


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mvpose import ops as _ops
    return _ops


def _dev(ops, c, use_cov=True, use_valid=True, **kw):
    xyz = torch.tensor(c["xyz"], device="cuda")
    cov = torch.tensor(c["cov"], device="cuda") if use_cov else None
    valid = torch.tensor(c["valid"], device="cuda") if use_valid else None
    out = ops.trajectory_smooth(xyz, cov, valid, **kw)
    torch.cuda.synchronize()
    return [o.cpu().numpy() if o is not None else None for o in out]


def _check(c, dev, r, what):
    xyz, resid, observed, status = dev
    assert np.array_equal(status, r.status), (what, status, r.status)
    assert np.array_equal(observed, r.observed), what
    ok = r.status == 0
    if ok.any():
        err = np.abs(xyz[:, ok].astype(np.float64) - r.xyz[:, ok].astype(np.float64)).max()
        print(f"{what}: max |xyz - ref| = {err:.3g}")
        assert err <= XYZ_ATOL, what
    assert np.array_equal(xyz[:, ~ok].view(np.uint32), c["xyz"][:, ~ok].view(np.uint32)), what
    fin = np.isfinite(r.resid)
    if fin.any():
        print(f"{what}: max resid rel err = {np.max(np.abs(resid[fin] - r.resid[fin]) / (np.abs(r.resid[fin]) + 0.1)):.3g}")
    np.testing.assert_allclose(resid, r.resid, rtol=RESID_RTOL, atol=RESID_ATOL, equal_nan=True, err_msg=what)


@functools.lru_cache(maxsize=None)
def _case(T, P, seed, long_gap):
    return ref.make_case(T, P, seed=seed, long_gap=long_gap)


@functools.lru_cache(maxsize=None)
def _dense300(lam):
    c = _case(300, 3, 11, 40)
    return ref.solve_dense(c["xyz"], c["cov"], c["valid"], lambda_smooth=lam)


# ------------------------------------------------------------------ layouts
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 6, 7, 11, 12, 13, 64, 257])
def test_tail_layouts_chunk4(ops, T):
    """chunk = 4: no separator, a 1-frame separator, last chunks of 0, 1 and 2 interior frames."""
    c = _case(T, 3, 100 + T, 7)
    r = ref.solve_dense(c["xyz"], c["cov"], c["valid"])
    _check(c, _dev(ops, c, chunk=4), r, f"T={T} chunk=4")
    if T >= 5:   # the same layouts with every frame observed (no failed chain at tiny T)
        full = ref.make_case(T, 3, seed=200 + T, knock=0.0)
        r = ref.solve_dense(full["xyz"], full["cov"], full["valid"])
        assert (r.status == 0).all()
        _check(full, _dev(ops, full, chunk=4), r, f"T={T} chunk=4 all observed")


@pytest.mark.parametrize("chunk", [5, 32])
@pytest.mark.parametrize("lam", [1e-2, 1.0, 1e2, 1e4])
def test_chunks_and_lambdas(ops, chunk, lam):
    c = _case(300, 3, 11, 40)     # the 40-frame gap is longer than either chunk
    _check(c, _dev(ops, c, chunk=chunk, lambda_smooth=lam), _dense300(lam), f"T=300 chunk={chunk} lam={lam}")


def test_automatic_chunk(ops):
    T, P = 4099, 17
    used, n_chunks, nbytes = ops.trajectory_smooth_plan(T, P, 0)
    assert n_chunks > 1 and 4 <= used <= 4096 and nbytes > 0
    c = _case(T, P, 12, used + 5)
    r = ref.solve_banded(c["xyz"], c["cov"], c["valid"])
    assert (r.status == 0).all()
    _check(c, _dev(ops, c, chunk=0), r, f"T={T} automatic chunk {used}")


def test_long_reduced_system(ops):
    T, P = 8192, 2
    c = _case(T, P, 13, 25)
    r = ref.solve_banded(c["xyz"], c["cov"], c["valid"])
    assert (r.status == 0).all()
    _check(c, _dev(ops, c, chunk=16), r, f"T={T} chunk=16")


# ------------------------------------------------------------------ failure and passthrough
@pytest.fixture(scope="module")
def failing():
    c = {k: v.copy() for k, v in ref.make_case(64, 5, seed=14, long_gap=9).items()}
    c["valid"][:, 1] = 0                       # 0 observed frames
    c["valid"][:, 3] = 0                       # 1 observed frame
    c["valid"][20, 3] = 1
    c["xyz"][20, 3] = (1.0, 2.0, 3.0)
    c["cov"][20, 3] = np.eye(3, dtype=np.float32)
    c["xyz"][5, 1] = np.nan                    # NaNs pass through as they came
    return c, ref.solve_dense(c["xyz"], c["cov"], c["valid"])


def test_failed_chains_pass_through(ops, failing):
    c, r = failing
    assert list(r.status) == [0, 0x80, 0, 0x80, 0]
    dev = _dev(ops, c, chunk=4)
    _check(c, dev, r, "failing chains")
    assert np.isnan(dev[1][:, [1, 3]]).all()
    assert np.array_equal(dev[0][:, [1, 3]].view(np.uint32), c["xyz"][:, [1, 3]].view(np.uint32))
    # the other chains are those of a call without the failing ones
    keep = [0, 2, 4]
    sub = {k: np.ascontiguousarray(v[:, keep]) for k, v in c.items()}
    alone = _dev(ops, sub, chunk=4)
    assert np.array_equal(alone[0].view(np.uint32), dev[0][:, keep].view(np.uint32))


def test_knocked_out_coordinates_are_never_used(ops, failing):
    c, r = failing
    out_frames = ~r.observed & np.isfinite(c["xyz"]).all(-1)
    assert out_frames.sum() > 20
    moved = {k: v.copy() for k, v in c.items()}
    moved["xyz"][out_frames] += np.float32(777.0)
    a, b = _dev(ops, c, chunk=4), _dev(ops, moved, chunk=4)
    ok = r.status == 0
    assert np.array_equal(a[0][:, ok].view(np.uint32), b[0][:, ok].view(np.uint32))
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


def test_sigma0_and_cov_floor(ops):
    c = _case(64, 3, 15, 9)
    r = ref.solve_dense(c["xyz"], None, c["valid"], sigma0=0.7, lambda_smooth=3.0)
    _check(c, _dev(ops, c, use_cov=False, sigma0=0.7, lambda_smooth=3.0, chunk=5), r, "cov=None sigma0=0.7")
    r = ref.solve_dense(c["xyz"], None, None, sigma0=2.0)
    _check(c, _dev(ops, c, use_cov=False, use_valid=False, sigma0=2.0, chunk=4), r, "cov=None valid=None")
    r = ref.solve_dense(c["xyz"], c["cov"], c["valid"], cov_floor=0.5)
    _check(c, _dev(ops, c, cov_floor=0.5, chunk=7), r, "cov_floor=0.5")
    cov6 = dict(c, cov=ref._cov6(c["cov"]))
    _check(c, _dev(ops, cov6, cov_floor=0.5, chunk=7), r, "cov (T, P, 6)")


def test_optional_outputs(ops):
    c = _case(64, 3, 15, 9)
    full = _dev(ops, c, chunk=6)
    bare = _dev(ops, c, chunk=6, want_resid=False, want_observed=False, want_status=False)
    assert bare[1] is None and bare[2] is None and bare[3] is None
    assert np.array_equal(full[0].view(np.uint32), bare[0].view(np.uint32))


# ------------------------------------------------------------------ fronts
def test_smooth_trajectory_front(ops):
    from mvpose import refine
    c = _case(64, 3, 15, 9)
    status = np.where(c["valid"] != 0, 3, 0x83).astype(np.uint8)     # refine status: bit 0x80 = failed
    want, res = ref.smooth_trajectory(c["xyz"], c["cov"], status, lambda_smooth=2.0, solver=ref.solve_dense)
    got, info = refine.smooth_trajectory(c["xyz"], c["cov"], status, lambda_smooth=2.0, return_info=True)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == c["xyz"].shape
    assert set(info) == {"resid", "observed", "status"} and all(isinstance(v, np.ndarray) for v in info.values())
    _check(c, (got, info["resid"], info["observed"], info["status"]), res, "smooth_trajectory numpy")
    t_dev = refine.smooth_trajectory(torch.tensor(c["xyz"], device="cuda"), torch.tensor(c["cov"], device="cuda"),
                                     torch.tensor(status, device="cuda"), lambda_smooth=2.0)
    assert isinstance(t_dev, torch.Tensor) and t_dev.is_cuda
    assert np.array_equal(t_dev.cpu().numpy().view(np.uint32), got.view(np.uint32))
    t_cpu = refine.smooth_trajectory(torch.tensor(c["xyz"]), torch.tensor(c["cov"]), torch.tensor(status),
                                     lambda_smooth=2.0)
    assert isinstance(t_cpu, torch.Tensor) and t_cpu.device.type == "cpu"
    # max_gap: the reference's mask, NaN exactly there
    want_gap, res = ref.smooth_trajectory(c["xyz"], c["cov"], status, lambda_smooth=2.0, max_gap=2,
                                          solver=ref.solve_dense)
    got_gap = refine.smooth_trajectory(c["xyz"], c["cov"], status, lambda_smooth=2.0, max_gap=2)
    mask = ref.gap_mask(res.observed, 2)
    assert mask.any() and not mask.all()
    assert np.array_equal(np.isnan(got_gap).all(-1), mask) and np.array_equal(np.isnan(want_gap).all(-1), mask)
    assert np.array_equal(got_gap[~mask].view(np.uint32), got[~mask].view(np.uint32))


def test_huber_reweighting(ops):
    from mvpose import refine
    T, P, sigma = 240, 3, 0.5
    rng = np.random.default_rng(21)
    truth = ref.make_case(T, P, seed=21, knock=0.0)["truth"]
    xyz = (truth + sigma * rng.normal(size=truth.shape)).astype(np.float32)
    hit = rng.uniform(size=(T, P)) < 0.05
    xyz[hit] += (30.0 * rng.choice([-1.0, 1.0], size=(int(hit.sum()), 3))).astype(np.float32)
    kw = dict(lambda_smooth=10.0, sigma0=sigma)
    plain = refine.smooth_trajectory(xyz, **kw)
    got, info = refine.smooth_trajectory(xyz, robust_k=3.0, robust_iters=3, return_info=True, **kw)
    want, res = ref.smooth_trajectory(xyz, robust_k=3.0, robust_iters=3, solver=ref.solve_dense, **kw)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64)).max()
    rms = lambda a: float(np.sqrt(np.mean((a - truth) ** 2)))
    print(f"huber: device vs reference loop {err:.3g}; rms robust {rms(got):.3g} plain {rms(plain):.3g} "
          f"ratio {rms(got) / rms(plain):.3g}")
    assert err <= XYZ_ATOL
    np.testing.assert_allclose(info["resid"], res.resid, rtol=RESID_RTOL, atol=RESID_ATOL, equal_nan=True)
    assert rms(got) < 0.25 * rms(plain)


def test_command_line(ops, tmp_path):
    from mvpose import cli, refine
    c = _case(64, 17, 16, 9)
    status = np.where(c["valid"] != 0, 2, 0x82).astype(np.uint8)
    run = tmp_path / "run"
    run.mkdir()
    paths = {k: str(run / (k + ".npy")) for k in ("kpts_3d", "kpts_3d_cov", "kpts_3d_refine_status")}
    np.save(paths["kpts_3d"], c["xyz"])
    np.save(paths["kpts_3d_cov"], c["cov"])
    np.save(paths["kpts_3d_refine_status"], status)
    with open(run / "recording_log.yaml", "w") as f:
        yaml.dump(paths, f)
    params = tmp_path / "params.yaml"
    params.write_text(yaml.dump({"smooth": {"lambda_smooth": 5.0, "max_gap": 20}}))
    cli.pose_refinement_main(["--run_path", str(run), "--refinement_params_yaml", str(params)])
    assert sorted(os.listdir(run)) == sorted(["kpts_3d.npy", "kpts_3d_cov.npy", "kpts_3d_refine_status.npy",
                                              "recording_log.yaml", "kpts_3d_linear_interpolation.npy"])
    out = cli.pose_refinement_main(["--run_path", str(run), "--refinement_types", "smooth",
                                    "--refinement_params_yaml", str(params)])
    want, info = refine.smooth_trajectory(c["xyz"], c["cov"], status, lambda_smooth=5.0, max_gap=20, return_info=True)
    got = np.load(out["smooth"])
    assert out["smooth"] == str(run / "kpts_3d_smooth.npy")
    assert got.dtype == np.float32 and got.shape == (64, 17, 3)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    resid = np.load(run / "kpts_3d_smooth_resid.npy")
    assert resid.shape == (64, 17) and np.array_equal(resid.view(np.uint32), info["resid"].view(np.uint32))
    # without a covariance file the smoother runs with sigma0
    os.remove(paths["kpts_3d_cov"])
    out = cli.pose_refinement_main(["--run_path", str(run), "--refinement_types", "smooth",
                                    "--refinement_params_yaml", str(params)])
    want = refine.smooth_trajectory(c["xyz"], None, status, lambda_smooth=5.0, max_gap=20)
    assert np.array_equal(np.load(out["smooth"]).view(np.uint32), want.view(np.uint32))
    with pytest.raises(ValueError, match="smooth"):
        cli.pose_refinement_main(["--run_path", str(run), "--refinement_types", "nonsense"])
