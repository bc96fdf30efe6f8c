"""GPU: mvp_trajectory_smooth_cov and mvp_trajectory_fit_cov (the covariance sweeps of
csrc/smooth_solver.h) against the fp64 numpy reference tests/traj_cov_ref.py, through mvpose.ops
and the fronts in mvpose.refine and mvpose.cli.

Bound on every float32 output entry: |dev − ref| <= 2^-23 · sqrt(ref_ii · ref_jj), ref_ii and ref_jj
the diagonal entries of the two frames' own blocks.  |Σij| <= sqrt(Σii Σjj); rounding to float32
costs at most 2^-24 of that; and the device's fp64 value differs from the reference's by far less
than 1e-9 of it (tests/test_trajectory_cov.py holds two fp64 evaluations of the reference to that on
every case used here), which moves a rounding by at most one more half-ulp.  Each test prints its
largest error as a multiple of the bound.

Measured on an MI355X, largest error as a multiple of the bound (0.5 is one float32 rounding of an
entry as large as sqrt(Σii Σjj)): the smoother's cases 0.178 (T = 2) to 0.498 (T = 300, chunk 32,
λ = 1e4), T = 4099 0.496, T = 2 against cov + cov_floor·I 0.480; the fit's cases 0.459 to 0.485;
chunk 4 against chunk 32 at T = 257: every float32 equal.  Over the fit's single-view stretch: angle
to the ray at most 1.05°, eigenvalue ratio 3.7 at the stretch's edges, 21.1 to 58.5 inside."""
import functools
import os

import numpy as np
import pytest
import torch
import yaml

import traj_cov_cases as cc
import traj_cov_ref as cr
import traj_smooth_ref as ts
from mvpose import ops, refine, synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def ratio(cov6, cross, diag0, cross0):
    """The largest error of the device's (cov (T, P, 6), cross (T, P, 3, 3)) as a multiple of the bound."""
    return cr.norm_error(cr.full6(cov6), cross, diag0, cross0) / cr.BOUND


@functools.lru_cache(maxsize=None)
def dev_smooth(c, chunk=None):
    s = cr.smooth_case(c)
    t = lambda a: None if a is None else torch.tensor(a, device=DEV)
    kw = dict(s["kw"], chunk=s["kw"]["chunk"] if chunk is None else chunk)
    cov, cross, status = ops.trajectory_smooth_cov(t(s["xyz"]), t(s["cov"]), t(s["valid"]), **kw)
    return cov.cpu().numpy(), cross.cpu().numpy(), status.cpu().numpy()


def check_smooth(c):
    s = cr.smooth_case(c)
    cov, cross, status = dev_smooth(c)
    assert np.array_equal(status, np.where(s["ok"], 0, 0x80))
    r = ratio(cov, cross, s["diag"], s["cross"])
    print(f"{cr.case_id(c)}: {int(s['ok'].sum())} chains, largest error {r:.3f} x bound")
    assert r <= 1.0
    return r


# ------------------------------------------------------------------ the smoother against the reference
@pytest.mark.parametrize("c", cr.SMOOTH_CASES, ids=cr.case_id)
def test_smooth_cov_matches_reference(c):
    check_smooth(c)


def test_smooth_cov_long_recording():
    """T = 4099 with the automatic chunk (80: 50 chunks, a reduced system of 49 separators), against
    the banded reference."""
    assert ops.trajectory_smooth_cov_plan(4099, 2, 0)[:2] == (80, 50)
    check_smooth(cr.LONG_CASE)


# ------------------------------------------------------------------ exact properties
def test_two_observed_frames_return_their_covariances():
    """T = 2: no prior row exists, A = blockdiag(W), so Σ_tt = cov_t + cov_floor·I and Σ_01 = 0."""
    m = ts.make_case(2, 3, seed=1, knock=0.0)
    floor = 0.25
    cov, cross, status = [o.cpu().numpy() for o in ops.trajectory_smooth_cov(
        torch.tensor(m["xyz"], device=DEV), torch.tensor(m["cov"], device=DEV), None, lambda_smooth=3.0,
        cov_floor=floor, chunk=4)]
    assert (status == 0).all()
    want = m["cov"].astype(np.float64) + floor * np.eye(3)
    zero = np.zeros((2, 3, 3, 3))
    zero[1] = np.nan
    r = ratio(cov, cross, want, zero)
    print(f"T=2: largest error {r:.3f} x bound")
    assert r <= 1.0
    assert np.array_equal(cross[0], np.zeros((3, 3, 3), np.float32)) and np.isnan(cross[1]).all()


def test_translation_leaves_the_covariance_bit_identical():
    c = cr.SMOOTH_CASES[10]          # T = 64, chunk 4
    s = cr.smooth_case(c)
    moved = (s["xyz"] + np.array([1000.0, -500.0, 250.0], np.float32)).astype(np.float32)
    cov, cross, status = [o.cpu().numpy() for o in ops.trajectory_smooth_cov(
        torch.tensor(moved, device=DEV), torch.tensor(s["cov"], device=DEV), torch.tensor(s["valid"], device=DEV),
        **s["kw"])]
    a = dev_smooth(c)
    assert np.array_equal(cov.view(np.uint32), a[0].view(np.uint32))
    assert np.array_equal(cross.view(np.uint32), a[1].view(np.uint32)) and np.array_equal(status, a[2])


def test_chunk_4_and_32_agree():
    c = cr.SMOOTH_CASES[11]          # T = 257
    s = cr.smooth_case(c)
    a, b = dev_smooth(c, 4), dev_smooth(c, 32)
    assert np.array_equal(a[2], b[2])
    # each within the bound of the reference; against each other, in the same normalisation, twice that
    r = cr.norm_error(cr.full6(a[0]), a[1], cr.full6(b[0]).astype(np.float64), b[1].astype(np.float64)) / cr.BOUND
    print(f"chunk 4 vs 32: {r:.3f} x bound")
    assert ratio(a[0], a[1], s["diag"], s["cross"]) <= 1.0 and ratio(b[0], b[1], s["diag"], s["cross"]) <= 1.0
    assert r <= 1.0


def test_uncertainty_grows_into_a_gap():
    """Chain 0's 9 unobserved frames: the trace of Σ_tt rises monotonically to the middle frame from
    both ends, and every gap frame exceeds both observed frames at the gap's edges."""
    c = cr.SMOOTH_CASES[10]
    s = cr.smooth_case(c)
    obs = s["observed"][:, 0]
    runs = [(t, t + cr.GAP) for t in range(len(obs) - cr.GAP) if not obs[t:t + cr.GAP].any()]
    a, b = runs[0]
    while a > 0 and not obs[a - 1]:
        a -= 1
    while b < len(obs) and not obs[b]:
        b += 1
    cov = dev_smooth(c)[0]
    trace = (cov[:, 0, 0] + cov[:, 0, 3] + cov[:, 0, 5]).astype(np.float64)
    mid = a + int(np.argmax(trace[a:b]))
    print(f"gap {a}..{b - 1}: trace {trace[a - 1]:.3g} | {trace[a]:.3g} .. {trace[mid]:.3g} .. {trace[b - 1]:.3g} | {trace[b]:.3g}")
    assert b - a >= cr.GAP and a >= 1 and b < len(obs)
    assert (np.diff(trace[a:mid + 1]) > 0).all() and (np.diff(trace[mid:b]) < 0).all()
    assert abs(mid - (a + b - 1) / 2) <= 1
    assert trace[a:b].min() > max(trace[a - 1], trace[b])


# ------------------------------------------------------------------ failed chains
def test_failed_chains_are_nan_and_leave_the_others_alone():
    m = {k: v.copy() for k, v in ts.make_case(64, 5, seed=14, long_gap=9).items()}
    m["valid"][:, 1] = 0                       # 0 observed frames
    m["valid"][:, 3] = 0                       # 1 observed frame
    m["valid"][20, 3] = 1
    m["xyz"][20, 3] = (1.0, 2.0, 3.0)
    m["cov"][20, 3] = np.eye(3, dtype=np.float32)

    def run(sel):
        t = lambda a: torch.tensor(np.ascontiguousarray(a[:, sel]), device=DEV)
        return [o.cpu().numpy() for o in ops.trajectory_smooth_cov(t(m["xyz"]), t(m["cov"]), t(m["valid"]), chunk=4)]
    cov, cross, status = run([0, 1, 2, 3, 4])
    assert list(status) == [0, 0x80, 0, 0x80, 0]
    assert np.isnan(cov[:, [1, 3]]).all() and np.isnan(cross[:, [1, 3]]).all()
    assert np.isfinite(cov[:, [0, 2, 4]]).all() and np.isfinite(cross[:-1, [0, 2, 4]]).all()
    alone = run([0, 2, 4])
    assert np.array_equal(alone[0].view(np.uint32), cov[:, [0, 2, 4]].view(np.uint32))
    assert np.array_equal(alone[1].view(np.uint32), cross[:, [0, 2, 4]].view(np.uint32))


# ------------------------------------------------------------------ the fit
def fit_args(weights, xyz):
    sc = cc.fit_scene()
    cams = torch.tensor(ops.pack_cameras(syn.reference_camera_params(sc["cams"])), device=DEV)
    gauss = torch.tensor(sc["gauss"], device=DEV) if weights == "heatmap" else None
    return (torch.tensor(sc["kpts"], device=DEV), cams, [0, 1], torch.tensor(xyz, device=DEV)), dict(
        weights=weights, gauss=gauss, min_conf=0.0, cov_floor=1.0)


@functools.lru_cache(maxsize=None)
def dev_fit(weights, hub):
    """ops.trajectory_fit's result on the scene: the state the covariance is taken at."""
    args, kw = fit_args(weights, cc.fit_scene()["xyz0"])
    out = ops.trajectory_fit(*args, huber_delta=hub, lambda_smooth=cc.FIT_LAMBDA, max_iter=30, tol=1e-6, **kw)
    assert (out[4].cpu().numpy() & 0xC0 == 0).all()
    return out[0].cpu().numpy()


@pytest.mark.parametrize("chunk", [4, 0])
@pytest.mark.parametrize("hub", cc.FIT_HUBERS)
@pytest.mark.parametrize("weights", ["conf", "heatmap"])
def test_fit_cov_matches_reference(weights, hub, chunk):
    """The reference is dense() on the device's own H̃ (ops.trajectory_fit_system at the same state,
    which other tests pin to the numpy restatement).  Over the single-view stretch the largest axis
    of Σ_tt lies within 5° of camera 0's ray through the joint and is larger than in every two-view
    frame, more than 10x in the frames at least FIT_EDGE frames from a two-view frame (conditions the
    reference meets with room under both weights: tests/test_trajectory_cov.py)."""
    sc = cc.fit_scene()
    state = dev_fit(weights, hub)
    args, kw = fit_args(weights, state)
    H, _, nviews, _ = [o.cpu().numpy() for o in ops.trajectory_fit_system(*args, huber_delta=hub, **kw)]
    cov, cross, status = [o.cpu().numpy() for o in ops.trajectory_fit_cov(
        *args, huber_delta=hub, lambda_smooth=cc.FIT_LAMBDA, chunk=chunk, **kw)]
    assert (status == 0).all()
    assert (nviews[cc.FIT_GAP[0]:cc.FIT_GAP[1], list(cc.FIT_LOST)] == 1).all()
    diag0, cross0 = cr.dense_chains(cr.full6(H), cc.FIT_LAMBDA)
    r = ratio(cov, cross, diag0, cross0)
    print(f"{weights} huber {hub} chunk {chunk}: largest error {r:.3f} x bound")
    assert r <= 1.0
    e = cc.FIT_EDGE
    for p in cc.FIT_LOST:
        angle, big = cc.stretch_figures(cr.full6(cov[:, p]), state[:, p], sc["cams"][0])
        print(f"  joint {p}: angle <= {angle.max():.2f} deg, eigenvalue ratio {big.min():.1f} (edges) {big[e:-e].min():.1f} "
              f"(inside) .. {big.max():.1f}")
        assert angle.max() <= 5.0
        assert big.min() > 1.0 and big[e:-e].min() > 10.0


def test_fit_cov_invalid_chains():
    """A state frame that is not finite, and one behind a used camera: NaN and 0x80 for that chain,
    the other chains as before to the bit."""
    sc = cc.fit_scene()
    state = dev_fit("conf", 0.0).copy()
    args, kw = fit_args("conf", state)
    good = [o.cpu().numpy() for o in ops.trajectory_fit_cov(*args, lambda_smooth=cc.FIT_LAMBDA, chunk=4, **kw)]
    state[7, 0, 1] = np.nan
    c0 = sc["cams"][0]
    state[30, 3] = (c0["R"].T @ (np.array([0.0, 0.0, -400.0]) - c0["T"].reshape(3))).astype(np.float32)
    args, kw = fit_args("conf", state)
    cov, cross, status = [o.cpu().numpy() for o in ops.trajectory_fit_cov(*args, lambda_smooth=cc.FIT_LAMBDA, chunk=4, **kw)]
    assert list(status) == [0x80, 0, 0, 0x80]
    assert np.isnan(cov[:, [0, 3]]).all() and np.isnan(cross[:, [0, 3]]).all()
    assert np.array_equal(cov[:, [1, 2]].view(np.uint32), good[0][:, [1, 2]].view(np.uint32))
    assert np.array_equal(cross[:, [1, 2]].view(np.uint32), good[1][:, [1, 2]].view(np.uint32))


# ------------------------------------------------------------------ fronts
def _front_case():
    m = ts.make_case(64, 3, seed=15, long_gap=9)
    return m, np.where(m["valid"] != 0, 3, 0x83).astype(np.uint8)     # refine status: bit 0x80 = failed


def test_smooth_trajectory_with_cov():
    m, status = _front_case()
    plain, info0 = refine.smooth_trajectory(m["xyz"], m["cov"], status, lambda_smooth=2.0, return_info=True)
    got, info = refine.smooth_trajectory(m["xyz"], m["cov"], status, lambda_smooth=2.0, return_info=True, with_cov=True)
    assert set(info0) == {"resid", "observed", "status"} and set(info) == set(info0) | {"cov", "cov_next"}
    assert np.array_equal(got.view(np.uint32), plain.view(np.uint32))
    for k in ("cov", "cov_next"):
        assert isinstance(info[k], np.ndarray) and info[k].dtype == np.float32 and info[k].shape == (64, 3, 3, 3)
    t = lambda a: torch.tensor(a, device=DEV)
    cov, cross, _ = ops.trajectory_smooth_cov(t(m["xyz"]), t(m["cov"]), t((status & 0x80) == 0), lambda_smooth=2.0)
    assert np.array_equal(info["cov"].view(np.uint32), cr.full6(cov.cpu().numpy()).view(np.uint32))
    assert np.array_equal(info["cov_next"].view(np.uint32), cross.cpu().numpy().view(np.uint32))
    assert np.isnan(info["cov_next"][-1]).all() and np.isfinite(info["cov"]).all()
    # without return_info nothing changes; tensors stay tensors, at home
    assert np.array_equal(refine.smooth_trajectory(m["xyz"], m["cov"], status, lambda_smooth=2.0, with_cov=True)
                          .view(np.uint32), plain.view(np.uint32))
    for home in ("cuda:0", "cpu"):
        _, ti = refine.smooth_trajectory(torch.tensor(m["xyz"], device=home), torch.tensor(m["cov"], device=home),
                                         torch.tensor(status, device=home), lambda_smooth=2.0, return_info=True,
                                         with_cov=True)
        assert isinstance(ti["cov"], torch.Tensor) and ti["cov"].device.type == home[:4].rstrip(":")
        assert np.array_equal(ti["cov"].cpu().numpy().view(np.uint32), info["cov"].view(np.uint32))
        assert np.array_equal(ti["cov_next"].cpu().numpy().view(np.uint32), info["cov_next"].view(np.uint32))
    # max_gap: NaN covariance exactly where the points are NaN; cov_next also where the next frame is
    got_gap, gi = refine.smooth_trajectory(m["xyz"], m["cov"], status, lambda_smooth=2.0, max_gap=2, return_info=True,
                                           with_cov=True)
    mask = np.isnan(got_gap).all(-1)
    assert mask.any() and not mask.all()
    assert np.array_equal(np.isnan(gi["cov"]).all((-1, -2)), mask) and np.array_equal(np.isnan(gi["cov"]).any((-1, -2)), mask)
    pair = mask | np.concatenate([mask[1:], np.ones_like(mask[:1])])
    assert np.array_equal(np.isnan(gi["cov_next"]).all((-1, -2)), pair)
    assert np.array_equal(gi["cov"][~mask].view(np.uint32), info["cov"][~mask].view(np.uint32))


def test_smooth_trajectory_with_cov_and_robust_k():
    """With robust_k the covariance is that of the final reweighted solve: ops.trajectory_smooth_cov
    on the covariance the loop scaled last (the reference loop's, formed in float32 as the device's)."""
    m, status = _front_case()
    m["xyz"][30, 1] += np.float32(25.0)           # a frame the loop down-weights
    kw = dict(lambda_smooth=2.0, cov_floor=0.01, robust_k=3.0, robust_iters=2)
    _, info = refine.smooth_trajectory(m["xyz"], m["cov"], status, return_info=True, with_cov=True, **kw)
    # the loop again by hand, through ops
    t = lambda a: torch.tensor(a, device=DEV)
    x, valid = t(m["xyz"]), t((status & 0x80) == 0)
    diag = t(np.array([1, 0, 0, 1, 0, 1], np.float32))
    base = t(ts._cov6(m["cov"]).astype(np.float32)) + torch.tensor(0.01, dtype=torch.float32, device=DEV) * diag
    scale = torch.ones((64, 3), dtype=torch.float32, device=DEV)
    k = torch.tensor(3.0, dtype=torch.float32, device=DEV)
    resid = ops.trajectory_smooth(x, base, valid, lambda_smooth=2.0)[1]
    for _ in range(2):
        d = torch.sqrt(resid * scale)
        scale = torch.where(d > k, d / k, torch.ones_like(d))
        last = (base * scale.unsqueeze(-1)).contiguous()
        resid = ops.trajectory_smooth(x, last, valid, lambda_smooth=2.0)[1]
    assert float(scale.max()) > 1.5
    cov, cross, _ = ops.trajectory_smooth_cov(x, last, valid, lambda_smooth=2.0)
    assert np.array_equal(info["cov"].view(np.uint32), cr.full6(cov.cpu().numpy()).view(np.uint32))
    assert np.array_equal(info["cov_next"].view(np.uint32), cross.cpu().numpy().view(np.uint32))


def test_fit_trajectory_with_cov_folds_people():
    """(T, Np, J, 3, V) in: "cov" and "cov_next" come back (T, Np, J, 3, 3), the numbers of the chains."""
    sc = cc.fit_scene()
    params = syn.reference_camera_params(sc["cams"])
    k5 = sc["kpts"].reshape(cc.FIT_T, 2, 2, 3, 2)
    s5 = sc["xyz0"].reshape(cc.FIT_T, 2, 2, 3)
    kw = dict(camera_indices=[0, 1], weights="conf", lambda_smooth=cc.FIT_LAMBDA, return_info=True)
    plain, info0 = refine.fit_trajectory(k5, params, s5, **kw)
    out, info = refine.fit_trajectory(k5, params, s5, with_cov=True, **kw)
    assert set(info) == set(info0) | {"cov", "cov_next"} and np.array_equal(out.view(np.uint32), plain.view(np.uint32))
    assert info["cov"].shape == info["cov_next"].shape == (cc.FIT_T, 2, 2, 3, 3) and info["cov"].dtype == np.float32
    args, akw = fit_args("conf", out.reshape(cc.FIT_T, 4, 3))
    cov, cross, _ = ops.trajectory_fit_cov(*args, lambda_smooth=cc.FIT_LAMBDA, **akw)
    assert np.array_equal(info["cov"].reshape(cc.FIT_T, 4, 3, 3).view(np.uint32), cr.full6(cov.cpu().numpy()).view(np.uint32))
    assert np.array_equal(info["cov_next"].reshape(cc.FIT_T, 4, 3, 3).view(np.uint32), cross.cpu().numpy().view(np.uint32))


def test_command_line_writes_the_covariance_on_request(tmp_path):
    from mvpose import cli
    m = ts.make_case(64, 17, seed=16, long_gap=9)
    status = np.where(m["valid"] != 0, 2, 0x82).astype(np.uint8)
    run = tmp_path / "run"
    run.mkdir()
    paths = {k: str(run / (k + ".npy")) for k in ("kpts_3d", "kpts_3d_cov", "kpts_3d_refine_status")}
    np.save(paths["kpts_3d"], m["xyz"])
    np.save(paths["kpts_3d_cov"], m["cov"])
    np.save(paths["kpts_3d_refine_status"], status)
    with open(run / "recording_log.yaml", "w") as f:
        yaml.dump(paths, f)
    params = tmp_path / "params.yaml"
    params.write_text(yaml.dump({"smooth": {"lambda_smooth": 5.0}}))
    cli.pose_refinement_main(["--run_path", str(run), "--refinement_types", "smooth", "--refinement_params_yaml", str(params)])
    assert "kpts_3d_smooth.npy" in os.listdir(run) and "kpts_3d_smooth_cov.npy" not in os.listdir(run)
    params.write_text(yaml.dump({"smooth": {"lambda_smooth": 5.0, "with_cov": True}}))
    cli.pose_refinement_main(["--run_path", str(run), "--refinement_types", "smooth", "--refinement_params_yaml", str(params)])
    got = np.load(run / "kpts_3d_smooth_cov.npy")
    _, info = refine.smooth_trajectory(m["xyz"], m["cov"], status, lambda_smooth=5.0, return_info=True, with_cov=True)
    assert got.dtype == np.float32 and got.shape == (64, 17, 3, 3)
    assert np.array_equal(got.view(np.uint32), info["cov"].view(np.uint32))
