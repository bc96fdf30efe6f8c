"""GPU: mvp_trajectory_fit_lag_system and mvp_trajectory_fit_lag against the fp64 numpy restatement
(tests/traj_fit_lag_ref.py, written from the text in include/mvpose.h) on the shapes and patterns of
tests/traj_fit_lag_cases.py; the call with every offset zero against mvp_trajectory_fit; and
refine.fit_trajectory(frame_offsets=...) and sync.refine_frame_offsets on the scene they were built
for."""
import functools

import numpy as np
import pytest
import torch

import traj_fit_cases as tc
import traj_fit_lag_cases as lc
import traj_fit_lag_ref as tl
import tri_refine_ref as tr
from mvpose import ops, refine, sync, synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WNAME = {tr.W_UNIT: "unit", tr.W_CONF: "conf", tr.W_GAUSS: "heatmap"}
IDS = [lc.case_id(kw) for kw in lc.CASES]


def dev_cams(cams):
    return torch.tensor(ops.pack_cameras(syn.reference_camera_params(cams)), device=DEV)


def dev_args(c):
    """(kpts, cams, cam_idx, xyz0), keywords: a case's inputs on the device (frac is the caller's)."""
    nv = len(c["cam_idx"])
    mask = None
    if c["mask"] is not None:
        mask = torch.tensor(((c["mask"][..., None] >> np.arange(nv)) & 1).astype(bool), device=DEV)
    gauss = torch.tensor(c["gauss"], device=DEV) if c["gauss"] is not None else None
    kw = dict(weights=WNAME[c["kw"]["weights"]], gauss=gauss, mask=mask, min_conf=c["kw"]["min_conf"],
              cov_floor=c["kw"]["cov_floor"], huber_delta=c["kw"]["huber_delta"])
    return (torch.tensor(c["kpts"], device=DEV), dev_cams(c["cams"]), c["cam_idx"], torch.tensor(c["xyz0"], device=DEV)), kw


def run_fit(c, frac, chunk):
    (k, cams, idx, x0), kw = dev_args(c)
    return ops.trajectory_fit_lag(k, cams, idx, frac, x0, lambda_smooth=c["lam"], max_iter=c["max_iter"], tol=lc.TOL,
                                  chunk=chunk, **kw)


@functools.lru_cache(maxsize=None)
def gpu_fit(i, chunk=None):
    c = lc.case(i)
    return [o.cpu().numpy() for o in run_fit(c, c["frac"], c["chunk"] if chunk is None else chunk)]


def ulps(a, b):
    """Distance in float32 steps between two float32 arrays (finite values)."""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia), np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


def block_diff(a, a0):
    """The largest difference relative to the frame block's largest magnitude."""
    with np.errstate(all="ignore"):
        s = np.abs(a0).max(-1, keepdims=True)
        return np.nanmax(np.where(s > 0, np.abs(a - a0) / s, np.abs(a - a0)), initial=0.0)


@pytest.mark.parametrize("i", range(len(lc.CASES)), ids=IDS)
def test_system_matches_restatement(i):
    """nviews equal; H̃, C and g̃ within 1e-9 of the frame block's largest magnitude; the two costs per
    chain and every entry of the offset derivative within rtol 1e-9."""
    c = lc.case(i)
    H0, C0, g0, nv0, cost0, dl0 = lc.reference_system(i)
    (k, cams, idx, x0), kw = dev_args(c)
    H, C, g, nviews, cost, dl = [o.cpu().numpy() for o in ops.trajectory_fit_lag_system(k, cams, idx, c["frac"], x0, **kw)]
    assert np.array_equal(nviews, nv0)
    for a, a0 in ((H, H0), (C, C0), (g, g0), (dl, dl0)):
        assert np.array_equal(np.isnan(a), np.isnan(a0))
    assert not C[-1].any()
    dH, dC, dg = block_diff(H, H0), block_diff(C, C0), block_diff(g, g0)
    with np.errstate(all="ignore"):
        fin = np.isfinite(cost0)
        dc = np.max(np.abs(cost - cost0)[fin] / np.maximum(np.abs(cost0[fin]), 1e-300), initial=0.0)
        dd = np.nanmax(np.where(dl0 != 0, np.abs(dl - dl0) / np.abs(dl0), np.abs(dl - dl0)), initial=0.0)
    print(f"{IDS[i]}: rel diff H {dH:.3g} C {dC:.3g} g {dg:.3g} cost {dc:.3g} dlag {dd:.3g}; chains with a non-finite "
          f"cost {int((~fin).any(1).sum())}")
    assert np.array_equal(cost[~fin], cost0[~fin], equal_nan=True)
    assert dH <= 1e-9 and dC <= 1e-9 and dg <= 1e-9 and dc <= 1e-9 and dd <= 1e-9


@pytest.mark.parametrize("i", range(len(lc.CASES)), ids=IDS)
def test_fit_matches_restatement(i):
    """Status and trial count equal; out_xyz within one float32 ulp of the restatement's rounded
    result; the costs within rtol 1e-9; invalid chains return their seed's bits, NaN resid, cost and
    dlag.  The last case rejects trials and runs out of them, asserted as every other."""
    c = lc.case(i)
    r = lc.reference_fit(i)
    xyz, resid, nviews, cost, status, dlag = gpu_fit(i)
    assert np.array_equal(status, r["status"]), (status, r["status"])
    assert np.array_equal(nviews, r["nviews"])
    bad = status == tl.INVALID
    assert np.array_equal(xyz[:, bad].view(np.uint32), c["xyz0"][:, bad].view(np.uint32))
    assert np.isnan(resid[:, bad]).all() and np.isnan(cost[bad]).all() and np.isnan(dlag[bad]).all()
    ok = ~bad
    if ok.any():
        u = ulps(xyz[:, ok], r["xyz"][:, ok])
        dX = np.abs(xyz[:, ok].astype(np.float64) - r["X"][:, ok]).max() / np.abs(r["X"][:, ok]).max()
        dc = (np.abs(cost[ok] - r["cost"][ok]) / np.abs(r["cost"][ok])).max()
        seen = nviews[:, ok] > 0
        rr = r["resid"][:, ok]
        dr = (np.abs(resid[:, ok][seen] - rr[seen]) / np.maximum(np.abs(rr[seen]), 1e-3)).max() if seen.any() else 0.0
        # The fp64 states may differ by 1e-9 of |X| = 300 cm, i.e. 3e-7 cm, and both sums depend on
        # them through X_{t+1} − X_t, about 1 cm here: ha (like-signed terms) moves by up to 1e-6 of
        # itself; ga, which nearly cancels at a fitted state, by up to 1e-6 of ha (ga / ha is a step in
        # frames).
        d0, d1 = dlag[ok], r["dlag"][ok]
        dha = (np.abs(d0[..., 1] - d1[..., 1]) / np.maximum(np.abs(d1[..., 1]), 1e-300))[d1[..., 1] > 0].max(initial=0.0)
        dga = (np.abs(d0[..., 0] - d1[..., 0]) / np.maximum(d1[..., 1], 1e-300))[d1[..., 1] > 0].max(initial=0.0)
        print(f"{IDS[i]}: {int(ok.sum())} chains, trials {sorted(set(int(s) & 63 for s in status[ok]))}; coordinates "
              f"that differ {(u > 0).mean():.3%}, largest {int(u.max())} ulp; |xyz - X_ref| / |X| {dX:.3g}; cost {dc:.3g}; "
              f"resid {dr:.3g}; ha {dha:.3g}; ga / ha {dga:.3g}")
        if u.max() > 1:
            for p in np.flatnonzero(ok):
                print(f"  chain {p}: status {status[p]:#x}, cost seed / final {cost[p].tolist()} (restatement "
                      f"{r['cost'][p].tolist()}, rejected {int(r['rejected'][p])}), largest "
                      f"{int(ulps(xyz[:, p], r['xyz'][:, p]).max())} ulp")
        assert u.max() <= 1
        assert dc <= 1e-9
        assert np.array_equal(np.isnan(resid[:, ok]), ~seen)
        assert dr <= 1e-5          # float32 outputs of an fp64 sum: 2^-24 and the state's 1e-9
        assert dha <= 1e-6 and dga <= 1e-6
        assert np.array_equal(d0[..., 1] == 0, d1[..., 1] == 0)


@pytest.mark.parametrize("i", [3, 7, 8, 9], ids=[IDS[k] for k in (3, 7, 8, 9)])
def test_all_offsets_zero_is_the_plain_fit(i):
    """traj_fit_cases' inputs with frac = 0 against ops.trajectory_fit: status, trials and nviews
    equal, out_xyz within one float32 ulp."""
    c = tc.case(i)
    (k, cams, idx, x0), kw = dev_args(c)
    plain = ops.trajectory_fit(k, cams, idx, x0, lambda_smooth=c["lam"], max_iter=c["max_iter"], tol=tc.TOL,
                               chunk=c["chunk"], **kw)
    lag = ops.trajectory_fit_lag(k, cams, idx, np.zeros(len(idx)), x0, lambda_smooth=c["lam"], max_iter=c["max_iter"],
                                 tol=tc.TOL, chunk=c["chunk"], **kw)
    xa, _, na, _, sa = [o.cpu().numpy() for o in plain]
    xb, _, nb, _, sb, _ = [o.cpu().numpy() for o in lag]
    assert np.array_equal(sa, sb) and np.array_equal(na, nb)
    ok = sa != tl.INVALID
    assert np.array_equal(xa[:, ~ok].view(np.uint32), xb[:, ~ok].view(np.uint32))
    u = ulps(xa[:, ok], xb[:, ok])
    print(f"{tc.case_id(tc.CASES[i])}: coordinates that differ {(u > 0).mean():.3%}, largest {int(u.max())} ulp")
    assert u.max() <= 1


@pytest.mark.parametrize("i", [4, 8, 9, lc.ROUGH], ids=[IDS[k] for k in (4, 8, 9, lc.ROUGH)])
def test_two_calls_are_bit_equal(i):
    """The second call on a side stream."""
    c = lc.case(i)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        again = run_fit(c, c["frac"], c["chunk"])
    side.synchronize()
    for a, b in zip(gpu_fit(i), again):
        assert np.array_equal(a.view(np.uint8), b.cpu().numpy().view(np.uint8))


@pytest.mark.parametrize("i", [7, 8, 9], ids=[IDS[k] for k in (7, 8, 9)])
def test_chunk_4_and_automatic_agree(i):
    """The result does not depend on the chunk length beyond fp64 rounding (automatic: 5, 8, 18)."""
    a, b = gpu_fit(i, 4), gpu_fit(i, 0)
    assert ops.trajectory_fit_lag_plan(lc.CASES[i]["T"], lc.CASES[i]["P"], 0)[0] != 4
    assert np.array_equal(a[4], b[4])
    ok = a[4] != tl.INVALID
    assert ulps(a[0][:, ok], b[0][:, ok]).max() <= 1


def test_accuracy_scene_on_the_device():
    """The scene of test_trajectory_fit_lag.py through the public path: refine.fit_trajectory with
    no offsets and with the planted ones, and sync.refine_frame_offsets from (0.3, 0.3).  The error
    ratio must reach half the restatement's, the recovered offsets lie within twice the restatement's
    own deviation from the planted ones."""
    sc = lc.scene()
    params = syn.reference_camera_params(sc["cams"])
    kw = dict(weights="conf", lambda_smooth=lc.SCENE_LAMBDA)
    k = torch.tensor(sc["kpts"], device=DEV)
    x0 = torch.tensor(sc["seed"], device=DEV)
    plain = refine.fit_trajectory(k, params, x0, **kw)
    lag, info = refine.fit_trajectory(k, params, x0, frame_offsets=lc.SCENE_FRAC, return_info=True, **kw)
    a, b = lc.scene_rms(plain.cpu().numpy(), sc["truth"]), lc.scene_rms(lag.cpu().numpy(), sc["truth"])
    s, sinfo = sync.refine_frame_offsets(sc["kpts"], params, sc["seed"], (0.0,) + lc.SCENE_START, **kw)
    print(f"RMS error: zero offsets {a:.3f} cm, planted offsets {b:.3f} cm, ratio {a / b:.2f} (restatement "
          f"{lc.SCENE_RMS_ZERO / lc.SCENE_RMS_TRUE:.2f}); recovered {s[1]:.4f}, {s[2]:.4f} (restatement "
          f"{lc.SCENE_RECOVERED}) in {len(sinfo['step'])} rounds, {sinfo['fits']} fits, costs {sinfo['cost']}")
    assert (info["status"].cpu().numpy() & 0xC0 == 0).all()
    assert tuple(info["dlag"].shape) == (lc.SCENE_JOINTS, 3, 2)
    assert a / b >= 0.5 * lc.SCENE_RMS_ZERO / lc.SCENE_RMS_TRUE
    dev = np.abs(np.array(lc.SCENE_RECOVERED) - lc.SCENE_FRAC[1:])
    assert s[0] == 0 and (np.abs(s[1:] - lc.SCENE_FRAC[1:]) <= 2 * dev).all()
    assert sinfo["cost"][-1] < sinfo["cost"][0] and len(sinfo["cost"]) == len(sinfo["step"]) + 1
