"""GPU: mvp_trajectory_fit_system and mvp_trajectory_fit against the fp64 numpy restatement
(tests/traj_fit_ref.py, written from the text in include/mvpose.h) on the shapes and patterns of
tests/traj_fit_cases.py, and refine.fit_trajectory on the scene it was built for."""
import functools

import numpy as np
import pytest
import torch

import traj_fit_cases as tc
import traj_fit_ref as tf
import tri_refine_ref as tr
from mvpose import ops, refine, synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WNAME = {tr.W_UNIT: "unit", tr.W_CONF: "conf", tr.W_GAUSS: "heatmap"}
IDS = [tc.case_id(kw) for kw in tc.CASES]


def dev_cams(cams):
    return torch.tensor(ops.pack_cameras(syn.reference_camera_params(cams)), device=DEV)


def dev_args(c):
    nv = len(c["cam_idx"])
    mask = None
    if c["mask"] is not None:
        mask = torch.tensor(((c["mask"][..., None] >> np.arange(nv)) & 1).astype(bool), device=DEV)
    gauss = torch.tensor(c["gauss"], device=DEV) if c["gauss"] is not None else None
    kw = dict(weights=WNAME[c["kw"]["weights"]], gauss=gauss, mask=mask, min_conf=c["kw"]["min_conf"],
              cov_floor=c["kw"]["cov_floor"], huber_delta=c["kw"]["huber_delta"])
    return (torch.tensor(c["kpts"], device=DEV), dev_cams(c["cams"]), c["cam_idx"], torch.tensor(c["xyz0"], device=DEV)), kw


@functools.lru_cache(maxsize=None)
def gpu_fit(i, chunk=None):
    c = tc.case(i)
    args, kw = dev_args(c)
    out = ops.trajectory_fit(*args, lambda_smooth=c["lam"], max_iter=c["max_iter"], tol=tc.TOL,
                             chunk=c["chunk"] if chunk is None else chunk, **kw)
    return [o.cpu().numpy() for o in out]


def ulps(a, b):
    """Distance in float32 steps between two float32 arrays (finite values)."""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia), np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


@pytest.mark.parametrize("i", range(len(tc.CASES)), ids=IDS)
def test_system_matches_restatement(i):
    """nviews equal; H̃ and g̃ within 1e-9 of the frame block's largest magnitude (sums of like-signed
    or O(1)-conditioned terms); the two costs per chain within rtol 1e-9."""
    c = tc.case(i)
    H0, g0, nv0, cost0 = tc.reference_system(i)
    args, kw = dev_args(c)
    H, g, nviews, cost = [o.cpu().numpy() for o in ops.trajectory_fit_system(*args, **kw)]
    assert np.array_equal(nviews, nv0)
    assert np.array_equal(np.isnan(H), np.isnan(H0)) and np.array_equal(np.isnan(g), np.isnan(g0))
    with np.errstate(all="ignore"):
        sH = np.abs(H0).max(-1, keepdims=True)
        sg = np.abs(g0).max(-1, keepdims=True)
        dH = np.nanmax(np.where(sH > 0, np.abs(H - H0) / sH, np.abs(H - H0)), initial=0.0)
        dg = np.nanmax(np.where(sg > 0, np.abs(g - g0) / sg, np.abs(g - g0)), initial=0.0)
        fin = np.isfinite(cost0)
        dc = np.max(np.abs(cost - cost0)[fin] / np.maximum(np.abs(cost0[fin]), 1e-300), initial=0.0)
    print(f"{IDS[i]}: rel diff H {dH:.3g} g {dg:.3g} cost {dc:.3g}; chains with a non-finite cost {int((~fin).any(1).sum())}")
    assert np.array_equal(cost[~fin], cost0[~fin], equal_nan=True)
    assert dH <= 1e-9 and dg <= 1e-9 and dc <= 1e-9


@pytest.mark.parametrize("i", range(len(tc.CASES)), ids=IDS)
def test_fit_matches_restatement(i):
    """Status and trial count equal; out_xyz within one float32 ulp of the restatement's rounded
    result (the fp64 states differ by about 1e-9 and may straddle a rounding boundary); the costs
    within rtol 1e-9; invalid chains return their seed's bits, NaN resid and cost.  The last three
    cases reject trials (a state kept, its linearisation reused with a larger mu) and run out of
    trials, which only equal states and costs after those trials can show."""
    c = tc.case(i)
    r = tc.reference_fit(i)
    xyz, resid, nviews, cost, status = gpu_fit(i)
    assert np.array_equal(status, r["status"]), (status, r["status"])
    assert np.array_equal(nviews, r["nviews"])
    bad = status == tf.INVALID
    assert np.array_equal(xyz[:, bad].view(np.uint32), c["xyz0"][:, bad].view(np.uint32))
    assert np.isnan(resid[:, bad]).all() and np.isnan(cost[bad]).all()
    ok = ~bad
    if ok.any():
        u = ulps(xyz[:, ok], r["xyz"][:, ok])
        dX = np.abs(xyz[:, ok].astype(np.float64) - r["X"][:, ok]).max() / np.abs(r["X"][:, ok]).max()
        dc = (np.abs(cost[ok] - r["cost"][ok]) / np.abs(r["cost"][ok])).max()
        seen = nviews[:, ok] > 0
        rr = r["resid"][:, ok]
        dr = (np.abs(resid[:, ok][seen] - rr[seen]) / np.maximum(np.abs(rr[seen]), 1e-3)).max() if seen.any() else 0.0
        print(f"{IDS[i]}: {int(ok.sum())} chains, trials {sorted(set(int(s) & 63 for s in status[ok]))}; coordinates "
              f"that differ {(u > 0).mean():.3%}, largest {int(u.max())} ulp; |xyz - X_ref| / |X| {dX:.3g}; cost {dc:.3g}; "
              f"resid {dr:.3g}")
        assert u.max() <= 1
        assert dc <= 1e-9
        assert np.array_equal(np.isnan(resid[:, ok]), ~seen)
        assert dr <= 1e-5          # float32 outputs of an fp64 sum: 2^-24 and the state's 1e-9


@pytest.mark.parametrize("i", [3, 7, 8, 9], ids=[IDS[k] for k in (3, 7, 8, 9)])
def test_two_calls_are_bit_equal(i):
    c = tc.case(i)
    args, kw = dev_args(c)
    again = ops.trajectory_fit(*args, lambda_smooth=c["lam"], max_iter=c["max_iter"], tol=tc.TOL, chunk=c["chunk"],
                               **kw)
    for a, b in zip(gpu_fit(i), again):
        assert np.array_equal(a.view(np.uint8), b.cpu().numpy().view(np.uint8))


@pytest.mark.parametrize("i", [6, 7, 8], ids=[IDS[k] for k in (6, 7, 8)])
def test_chunk_4_and_automatic_agree(i):
    """The result does not depend on the chunk length beyond fp64 rounding (automatic: 5, 8, 18)."""
    a, b = gpu_fit(i, 4), gpu_fit(i, 0)
    assert ops.trajectory_fit_plan(tc.CASES[i]["T"], tc.CASES[i]["P"], 0)[0] != 4
    assert np.array_equal(a[4], b[4])
    ok = a[4] != tf.INVALID
    assert ulps(a[0][:, ok], b[0][:, ok]).max() <= 1


def test_max_iter_0_returns_the_seed_with_its_cost():
    c = tc.case(3)
    args, kw = dev_args(c)
    xyz, resid, nviews, cost, status = [o.cpu().numpy() for o in
                                        ops.trajectory_fit(*args, lambda_smooth=c["lam"], max_iter=0, chunk=4, **kw)]
    _, _, _, cost0 = tc.reference_system(3)
    ok = tc.reference_fit(3)["status"] != tf.INVALID
    assert (status[ok] == 0x40).all() and (status[~ok] == 0x80).all()
    assert np.array_equal(xyz.view(np.uint32), c["xyz0"].view(np.uint32))
    f0 = cost0[:, 0] + c["lam"] * cost0[:, 1]
    assert np.allclose(cost[ok, 0], f0[ok], rtol=1e-9) and np.array_equal(cost[ok, 0], cost[ok, 1])


def test_gap_scene_on_the_device():
    """The scene of test_trajectory_fit.py through the public path: the two-view frames' points,
    smooth_trajectory's gap-filled seed from them, refine.fit_trajectory on all 17 joints.  The gap
    RMS must be below the seed's by half the factor the restatement reaches."""
    g = tc.gap_scene()
    params = syn.reference_camera_params(g["cams"])
    tri = torch.tensor(g["tri"], device=DEV)
    seed = refine.smooth_trajectory(tri, lambda_smooth=tc.GAP_LAMBDA, sigma0=1.0)
    fit, info = refine.fit_trajectory(torch.tensor(g["kpts"], device=DEV), params, seed, camera_indices=[0, 1],
                                      weights="conf", lambda_smooth=tc.GAP_LAMBDA, return_info=True)
    a, b = tc.gap_rms(seed.cpu().numpy(), g["truth"]), tc.gap_rms(fit.cpu().numpy(), g["truth"])
    print(f"gap RMS: seed {a:.3f} cm, fit {b:.3f} cm, factor {a / b:.3f} (restatement: {tc.GAP_FACTOR})")
    assert (info["status"].cpu().numpy() & 0xC0 == 0).all()
    assert (info["nviews"][tc.GAP[0]:tc.GAP[1]] == 1).all()
    assert a / b >= tc.GAP_FACTOR / 2


def test_people_are_folded_to_chains():
    """(T, Np, J, 3, V) is Np·J independent chains: the same numbers as one person at a time."""
    c = tc.case(7)                           # 65 chains: read them as 5 people of 13 joints
    T = c["kpts"].shape[0]
    params = syn.reference_camera_params(c["cams"])
    k5 = torch.tensor(c["kpts"].reshape(T, 5, 13, 3, 2), device=DEV)
    s5 = torch.tensor(c["xyz0"].reshape(T, 5, 13, 3), device=DEV)
    kw = dict(camera_indices=c["cam_idx"], weights="conf", lambda_smooth=2.0, huber_px=2.0, min_conf=tc.MIN_CONF)
    all5 = refine.fit_trajectory(k5, params, s5, **kw)
    one = refine.fit_trajectory(k5[:, 2].contiguous(), params, s5[:, 2].contiguous(), **kw)
    assert all5.shape == (T, 5, 13, 3)
    assert torch.equal(all5[:, 2].view(torch.int32), one.view(torch.int32))


def test_people_trajectories_gathers_the_2d_inputs_on_request():
    """with_2d=True adds kpts_2d / heatmaps_2d / tri_inliers per person, gathered like kpts_3d; the
    default returns what it returned before."""
    from mvpose.pipeline import MultiViewPipeline
    T, G, J, V = 6, 2, 17, 2
    rng = np.random.default_rng(0)
    xyz = np.stack([syn.make_poses(T, seed=1, jitter=0.0), syn.make_poses(T, seed=2, jitter=0.0) + 200.0], 1)
    xyz[3:] = xyz[3:, ::-1]                                  # the groups swap places at frame 3
    out = {"kpts_3d": torch.tensor(xyz, dtype=torch.float32, device=DEV),
           "kpts_2d": torch.tensor(rng.uniform(0, 1000, (T, G, J, 3, V)), dtype=torch.float32, device=DEV),
           "heatmaps_2d": torch.tensor(rng.uniform(0, 10, (T, G, V, J, 6)), device=DEV),
           "tri_inliers": torch.tensor(rng.uniform(size=(T, G, J, V)) < 0.7, device=DEV)}
    plain = MultiViewPipeline.people_trajectories(out, max_gap=0)
    full = MultiViewPipeline.people_trajectories(out, max_gap=0, with_2d=True)
    assert sorted(plain) == ["kpts_3d_person", "person_present", "person_track"]
    assert sorted(full) == sorted(list(plain) + ["kpts_2d_person", "heatmaps_2d_person", "tri_inliers_person"])
    for k in plain:
        assert torch.equal(plain[k], full[k])
    for name in ("kpts_2d", "heatmaps_2d", "tri_inliers"):
        got = full[name + "_person"]
        assert got.shape == out[name].shape
        assert torch.equal(got[:3], out[name][:3]) and torch.equal(got[3:], out[name][3:].flip(1))
