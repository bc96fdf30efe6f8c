"""GPU: mvp_bundle_adjust_system and mvp_bundle_adjust against the fp64 numpy restatement
(tests/ba_ref.py, written from the text in include/mvpose.h), the calls' edge cases, and
calib.refine_extrinsics on the rig it has to repair."""
import functools

import numpy as np
import pytest
import torch

import ba_cases
import ba_ref
import tri_refine_ref as tr
from mvpose import _lib, calib, ops, synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WNAME = {tr.W_UNIT: "unit", tr.W_CONF: "conf", tr.W_GAUSS: "heatmap"}


def dev_cams(cams):
    return torch.tensor(ops.pack_cameras(syn.reference_camera_params(cams)), device=DEV)


def unpack_mask(bits, nv):
    return torch.tensor(((bits[:, None] >> np.arange(nv)) & 1).astype(bool), device=DEV)


@pytest.mark.parametrize("kw", ba_cases.SYSTEM_CASES, ids=ba_cases.case_id)
def test_system_matches_restatement(kw):
    """S, b and the cost to relative 1e-9 of the largest entry of S (of |b|); counts equal."""
    case = ba_cases.system_case(**ba_cases.case_args(kw))
    lam, hub, sigma = kw.get("lam", 0.0), kw.get("hub", 0.0), kw.get("sigma", 0.0)
    S0, b0, f0, n_act, n_used, _ = ba_cases.reference_system(case, lam, hub, sigma)
    nv = len(case["cam_idx"])
    kp = torch.tensor(case["kpts"], device=DEV)
    gauss = torch.tensor(case["gauss"], device=DEV) if case["gauss"] is not None else None
    if gauss is not None:
        kp = kp.reshape(case["shape"] + kp.shape[1:])
    xyz = torch.tensor(case["xyz"], device=DEV).reshape(tuple(kp.shape[:-2]) + (3,))
    mask = unpack_mask(case["mask"], nv).reshape(tuple(kp.shape[:-2]) + (nv,)) if case["mask"] is not None else None
    S, b, f, counts = ops.bundle_adjust_system(
        kp, dev_cams(case["cams"]), case["cam_idx"], case["free"], xyz, lam=lam, weights=WNAME[case["weights"]],
        gauss=gauss, mask=mask, min_conf=case["min_conf"], huber_delta=hub, trans_prior_sigma=sigma)
    S, b, f, counts = S.cpu().numpy(), b.cpu().numpy(), float(f.cpu()), counts.cpu().numpy()
    dS = np.abs(S - S0).max() / np.abs(S0).max()
    db = np.abs(b - b0).max() / max(np.abs(b0).max(), 1e-300)
    df = abs(f - f0) / max(abs(f0), 1e-300)
    print(f"{ba_cases.case_id(kw)}: active {n_act} used {n_used} rel diff S {dS:.3g} b {db:.3g} cost {df:.3g}")
    assert counts.tolist() == [n_act, n_used]
    assert np.array_equal(S, S.T)
    assert dS <= 1e-9 and db <= 1e-9 and df <= 1e-9


@functools.lru_cache(maxsize=None)
def gpu_run(name):
    rc = ba_cases.recovery()
    kw = dict(ba_cases.RUNS[name])
    cam_idx, free, w = kw.pop("cam_idx"), kw.pop("free"), WNAME[kw.pop("weights")]
    cams = dev_cams(rc["cams"])
    out = ops.bundle_adjust(torch.tensor(rc["kpts"], device=DEV), cams, cam_idx, free,
                            torch.tensor(rc["xyz0"], device=DEV), weights=w, **kw)
    return cams.cpu().numpy(), free, [t.cpu().numpy() for t in out]


@pytest.mark.parametrize("name", sorted(ba_cases.RUNS))
def test_bundle_adjust_matches_restatement(name):
    ref = ba_cases.reference_run(name)
    cams_in, free, (cams, xyz, pstat, cov, info) = gpu_run(name)
    worst_R = worst_T = 0.0
    for v in range(4):
        R, T = cams[v, 14:23].reshape(3, 3), cams[v, 23:26]
        worst_R = max(worst_R, np.abs(R - ref["cams"][v]["R"]).max())
        worst_T = max(worst_T, np.abs(T - ref["cams"][v]["T"].reshape(3)).max())
        c = ref["cams"][v]
        np.testing.assert_allclose(cams[v], ops.pack_camera(c["K"], R, T, c["dist"]), rtol=1e-15, atol=1e-9)
        if v not in free:
            assert np.array_equal(cams[v], cams_in[v])
    dX = np.abs(xyz.astype(np.float64) - ref["X"])[ref["active"]].max()
    dcov = np.abs(cov - ref["cov"]).max() / np.abs(ref["cov"]).max()
    print(f"{name}: |dR| {worst_R:.3g} |dT| {worst_T:.3g} |dX| {dX:.3g} cov rel {dcov:.3g} info {info.tolist()}")
    assert worst_R <= 1e-7 and worst_T <= 1e-7
    assert dX <= 1e-4
    assert info[2:5].tolist() == ref["info"][2:5].tolist()
    assert info[6:8].tolist() == ref["info"][6:8].tolist()
    np.testing.assert_allclose(info[:2], ref["info"][:2], rtol=1e-9)
    assert info[5] == ref["info"][5]
    assert np.array_equal(pstat, ref["point_status"])
    assert np.array_equal(cov, cov.T) or np.allclose(cov, cov.T, rtol=1e-9, atol=0)
    assert dcov <= 1e-6


def test_rejected_trials_follow_the_restatement():
    """Seeds 150 cm off and cameras 10 degrees off: the run rejects trials (lambda goes up and down)
    and leaves seeds behind a camera out.  The state this far from a minimum amplifies rounding by
    a factor nobody has bounded, so what is compared is what the margins (>= 0.8 here, asserted on
    the CPU) protect: every decision (trials, accepted trials, status, the final lambda), the
    counts and the point status.  The cost and camera differences are printed."""
    r, ref = ba_cases.rough(), ba_cases.rough_reference_run()
    kw = dict(r["kw"])
    w = WNAME[kw.pop("weights")]
    cams, xyz, pstat, cov, info = ops.bundle_adjust(torch.tensor(r["kpts"], device=DEV), dev_cams(r["cams"]), [0, 1, 2, 3],
                                                    [2, 3], torch.tensor(r["xyz0"], device=DEV), weights=w, **kw)
    info, cams = info.cpu().numpy(), cams.cpu().numpy()
    dT = max(np.abs(cams[v, 23:26] - ref["cams"][v]["T"].reshape(3)).max() for v in (2, 3))
    print(f"rough: info {info.tolist()} rel cost diff {abs(info[1] - ref['info'][1]) / ref['info'][1]:.3g} |dT| {dT:.3g}")
    assert info[2:8].tolist() == ref["info"][2:8].tolist()
    assert 0 < info[3] < info[2]
    assert np.array_equal(pstat.cpu().numpy(), ref["point_status"])
    assert np.isfinite(info[:2]).all() and info[1] < info[0]


def dirty_run(max_iter=30, **over):
    """A run with inactive points: one used view, a seed that is not finite, a seed behind camera 0."""
    case = ba_cases.system_case(4, [2, 3], 170, dirty=True)
    nv = 4
    args = dict(weights="unit", mask=unpack_mask(case["mask"], nv), min_conf=case["min_conf"], max_iter=max_iter, tol=1e-6)
    args.update(over)
    kp, xyz = torch.tensor(case["kpts"], device=DEV), torch.tensor(case["xyz"], device=DEV)
    cams = dev_cams(case["cams"])
    return case, cams, ops.bundle_adjust(kp, cams, case["cam_idx"], case["free"], xyz, **args)


def test_inactive_points_return_their_seed_bits():
    case, cams, (oc, xyz, pstat, cov, info) = dirty_run()
    used, _, _ = tr.views(case["kpts"], case["cam_idx"], case["mask"], tr.W_UNIT, None, case["min_conf"], 1.0)
    act = ba_ref.active_points(case["xyz"], case["cams"], case["cam_idx"], used)
    assert (~act).sum() >= 3
    ps = pstat.cpu().numpy()
    assert np.array_equal(ps, np.where(act, 0, 0x80).astype(np.uint8))
    out = xyz.cpu().numpy()
    assert np.array_equal(out[~act].view(np.uint32), case["xyz"][~act].view(np.uint32))
    assert np.isfinite(out[act]).all() and int(info[6]) == act.sum()
    assert np.array_equal(oc.cpu().numpy()[:2], cams.cpu().numpy()[:2])


def test_max_iter_zero_returns_the_seed_state():
    case, cams, (oc, xyz, pstat, cov, info) = dirty_run(max_iter=0)
    info = info.cpu().numpy()
    assert info[2] == 0 and info[3] == 0 and info[4] == 1 and info[0] == info[1] and info[5] == 1e-3
    f0 = ba_cases.reference_system(case, 0.0, 0.0, 0.0)[2]
    assert abs(info[0] - f0) <= 1e-9 * f0
    oc, ci = oc.cpu().numpy(), cams.cpu().numpy()
    assert np.array_equal(oc[:, :26], ci[:, :26])
    np.testing.assert_allclose(oc, ci, rtol=1e-15, atol=1e-9)
    assert np.array_equal(xyz.cpu().numpy().view(np.uint32), case["xyz"].view(np.uint32))


def test_starved_free_view_ends_at_once():
    rc = ba_cases.recovery()
    kp = rc["kpts"][:34].copy()
    kp[2:, 0, 3] = np.nan       # view 3 keeps two observations
    cams = dev_cams(rc["cams"])
    oc, xyz, pstat, cov, info = ops.bundle_adjust(torch.tensor(kp, device=DEV), cams, [0, 1, 2, 3], [2, 3],
                                                  torch.tensor(rc["xyz0"][:34], device=DEV))
    info = info.cpu().numpy()
    assert info[4] == 3 and info[2] == 0
    assert np.array_equal(oc.cpu().numpy()[:, :26], cams.cpu().numpy()[:, :26])
    assert np.array_equal(xyz.cpu().numpy().view(np.uint32), rc["xyz0"][:34].view(np.uint32))


def test_two_runs_are_bit_identical():
    a = dirty_run(huber_delta=1.0)[2]
    b = dirty_run(huber_delta=1.0)[2]
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.uint8) if x.dtype == torch.uint8 else x.contiguous().view(torch.int32 if x.dtype == torch.float32 else torch.int64),
                           y.view(torch.uint8) if y.dtype == torch.uint8 else y.contiguous().view(torch.int32 if y.dtype == torch.float32 else torch.int64))


def test_argument_errors_name_the_argument():
    rc = ba_cases.recovery()
    kp, xyz, cams = torch.tensor(rc["kpts"][:34], device=DEV), torch.tensor(rc["xyz0"][:34], device=DEV), dev_cams(rc["cams"])
    with pytest.raises(_lib.MvposeError, match="free_mask"):
        ops.bundle_adjust(kp, cams, [0, 1, 2, 3], [4], xyz)
    with pytest.raises(_lib.MvposeError, match="fixed"):
        ops.bundle_adjust(kp, cams, [0, 1, 2, 3], [0, 1, 2, 3], xyz)
    with pytest.raises(_lib.MvposeError, match="trans_prior_sigma"):
        ops.bundle_adjust(kp, cams, [0, 1, 2, 3], [2, 3], xyz, trans_prior_sigma=float("nan"))
    with pytest.raises(_lib.MvposeError, match="max_iter"):
        ops.bundle_adjust(kp, cams, [0, 1, 2, 3], [2, 3], xyz, max_iter=64)
    with pytest.raises(_lib.MvposeError, match="lambda"):
        ops.bundle_adjust_system(kp, cams, [0, 1, 2, 3], [2, 3], xyz, lam=float("inf"))
    with pytest.raises(_lib.MvposeError, match="cam_idx"):
        ops.bundle_adjust(kp, cams, [0, 1, 2, 7], [2], xyz)


def mean_reproj(kpts4, params, device=DEV):
    """Mean reprojection error of the robust triangulation over its inlier views (undistorted px)."""
    kp = torch.tensor(kpts4, device=device)
    cams = torch.tensor(ops.pack_cameras(params), device=device)
    _, inl, err = ops.triangulate_robust(kp, cams, list(range(kp.shape[-1])), inlier_px=25.0)
    return float(err[inl].mean().cpu())


def test_refine_extrinsics_repairs_the_rig():
    rc = ba_cases.recovery()
    bad = syn.reference_camera_params(rc["cams"])
    new, info = calib.refine_extrinsics(rc["kpts4"], bad, free=[2, 3], weights="unit")
    e_bad, e_new = mean_reproj(rc["kpts4"], bad), mean_reproj(rc["kpts4"], new)
    e_true = mean_reproj(rc["kpts4"], syn.reference_camera_params(rc["true"]))
    print(f"mean reprojection error: perturbed {e_bad:.4f} adjusted {e_new:.4f} true {e_true:.4f} px; "
          f"rms {info['rms_before']:.4f} -> {info['rms_after']:.4f}; status {info['status_text']}, {info['trials']} trials")
    assert info["status"] == 0 and info["rms_after"] < info["rms_before"]
    assert e_new < e_bad and abs(e_new - e_true) <= 0.05 * e_true
    assert info["points"].shape == rc["kpts4"].shape[:2] + (3,) and info["cam_cov"].shape == (12, 12)
    for k in (0, 1):
        assert new[k][1] is bad[k][1] and new[k][2] is bad[k][2]


def test_refine_extrinsics_takes_people_groups():
    rc = ba_cases.recovery()
    k4 = rc["kpts4"][:40]
    T, J = k4.shape[:2]
    k5 = np.full((T, 2, J, 3, 4), np.nan, np.float32)      # group 1 is padding
    k5[:, 0] = k4
    bad = syn.reference_camera_params(rc["cams"])
    new5, info5 = calib.refine_extrinsics(k5, bad, free=[2, 3], weights="unit")
    new4, info4 = calib.refine_extrinsics(k4, bad, free=[2, 3], weights="unit")
    assert info5["points"].shape == (T, 2, J, 3) and (info5["point_status"][:, 1] == 0x80).all()
    assert info5["active_points"] == info4["active_points"] == T * J
    for k in (2, 3):
        np.testing.assert_allclose(new5[k][1], new4[k][1], rtol=0, atol=1e-9)
        np.testing.assert_allclose(new5[k][2], new4[k][2], rtol=0, atol=1e-7)
