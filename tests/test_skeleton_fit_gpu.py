"""GPU: mvp_skeleton_fit_system and mvp_skeleton_fit against the fp64 numpy restatement
(tests/skel_fit_ref.py, written from the text in include/mvpose.h) on the shapes and patterns of
tests/skel_fit_cases.py, against mvp_trajectory_fit where the two state the same problem,
refine.fit_skeleton on the scene it was built for, and the pose_refinement command line's
skeleton_fit type."""
import functools
import os

import numpy as np
import pytest
import torch
import yaml

import skel_fit_cases as sc
import skel_fit_ref as sk
import tri_refine_ref as tr
from mvpose import cli, ops, refine, synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WNAME = {tr.W_UNIT: "unit", tr.W_CONF: "conf", tr.W_GAUSS: "heatmap"}
IDS = [sc.case_id(kw) for kw in sc.CASES]


def dev_cams(cams):
    return torch.tensor(ops.pack_cameras(syn.reference_camera_params(cams)), device=DEV)


def dev_args(c):
    """The positional arguments of the trajectory fit's calls and the keyword ones both families share."""
    nv = len(c["cam_idx"])
    mask = None
    if c["mask"] is not None:
        mask = torch.tensor(((c["mask"][..., None] >> np.arange(nv)) & 1).astype(bool), device=DEV)
    gauss = torch.tensor(c["gauss"], device=DEV) if c["gauss"] is not None else None
    kw = dict(weights=WNAME[c["kw"]["weights"]], gauss=gauss, mask=mask, min_conf=c["kw"]["min_conf"],
              cov_floor=c["kw"]["cov_floor"], huber_delta=c["kw"]["huber_delta"])
    return (torch.tensor(c["kpts"], device=DEV), dev_cams(c["cams"]), c["cam_idx"], torch.tensor(c["xyz0"], device=DEV)), kw


def skel_args(c):
    return (c["J"], c["pairs"], torch.tensor(c["lengths"], device=DEV))


@functools.lru_cache(maxsize=None)
def gpu_fit(i, chunk=None, max_iter=None):
    c = sc.case(i)
    args, kw = dev_args(c)
    out = ops.skeleton_fit(*args, *skel_args(c), lambda_bone=c["beta"], lambda_smooth=c["lam"],
                           max_iter=c["max_iter"] if max_iter is None else max_iter, tol=sc.TOL,
                           chunk=c["chunk"] if chunk is None else chunk, **kw)
    return [o.cpu().numpy() for o in out]


def ulps(a, b):
    """Distance in float32 steps between two float32 arrays (finite values)."""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia), np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


@pytest.mark.parametrize("i", range(len(sc.CASES)), ids=IDS)
def test_system_matches_restatement(i):
    """nviews equal, NaN patterns equal; H̃ and g̃ (data plus bone terms) within 1e-9 of the frame
    block's largest magnitude; the three costs per group within rtol 1e-9."""
    c = sc.case(i)
    H0, g0, nv0, cost0 = sc.reference_system(i)
    args, kw = dev_args(c)
    H, g, nviews, cost = [o.cpu().numpy() for o in ops.skeleton_fit_system(*args, *skel_args(c), lambda_bone=c["beta"],
                                                                           **kw)]
    assert np.array_equal(nviews, nv0)
    assert np.array_equal(np.isnan(H), np.isnan(H0)) and np.array_equal(np.isnan(g), np.isnan(g0))
    with np.errstate(all="ignore"):
        sH = np.abs(H0).max(-1, keepdims=True)
        sg = np.abs(g0).max(-1, keepdims=True)
        dH = np.nanmax(np.where(sH > 0, np.abs(H - H0) / sH, np.abs(H - H0)), initial=0.0)
        dg = np.nanmax(np.where(sg > 0, np.abs(g - g0) / sg, np.abs(g - g0)), initial=0.0)
        fin = np.isfinite(cost0)
        dc = np.max(np.abs(cost - cost0)[fin] / np.maximum(np.abs(cost0[fin]), 1e-300), initial=0.0)
    print(f"{IDS[i]}: rel diff H {dH:.3g} g {dg:.3g} cost {dc:.3g}; groups with a non-finite cost {int((~fin).any(1).sum())}")
    assert np.array_equal(cost[~fin], cost0[~fin], equal_nan=True)
    assert dH <= 1e-9 and dg <= 1e-9 and dc <= 1e-9


@pytest.mark.parametrize("i", range(len(sc.CASES)), ids=IDS)
def test_fit_matches_restatement(i):
    """Group and chain status and the trial counts equal; out_xyz within one float32 ulp of the
    restatement's rounded result; the four costs within rtol 1e-9; out_bone within 1e-5 of L;
    invalid chains and groups return their seed's bits, NaN resid, NaN cost and NaN bones."""
    c = sc.case(i)
    r = sc.reference_fit(i)
    xyz, resid, nviews, bone, cost, gstatus, cstatus = gpu_fit(i)
    assert np.array_equal(gstatus, r["group_status"]), (gstatus, r["group_status"])
    assert np.array_equal(cstatus, r["chain_status"]), (cstatus, r["chain_status"])
    assert np.array_equal(nviews, r["nviews"])
    bad = cstatus == sk.INVALID
    assert np.array_equal(xyz[:, bad].view(np.uint32), c["xyz0"][:, bad].view(np.uint32))
    assert np.isnan(resid[:, bad]).all()
    gbad = gstatus == sk.INVALID
    assert np.isnan(cost[gbad]).all() and np.isnan(bone[:, gbad]).all()
    assert bad.reshape(-1, c["J"])[gbad].all()
    assert np.array_equal(np.isnan(bone), np.isnan(r["bone"]))
    ok = ~bad
    if ok.any():
        u = ulps(xyz[:, ok], r["xyz"][:, ok])
        dX = np.abs(xyz[:, ok].astype(np.float64) - r["X"][:, ok]).max() / np.abs(r["X"][:, ok]).max()
        with np.errstate(all="ignore"):
            dc = np.nanmax(np.abs(cost[~gbad] - r["cost"][~gbad]) / np.maximum(np.abs(r["cost"][~gbad]), 1e-300))
            L = np.broadcast_to(c["lengths"].astype(np.float64)[None], bone.shape)
            db = np.nanmax(np.abs(bone.astype(np.float64) - r["bone"]) / L, initial=0.0)
        seen = nviews[:, ok] > 0
        rr = r["resid"][:, ok]
        dr = (np.abs(resid[:, ok][seen] - rr[seen]) / np.maximum(np.abs(rr[seen]), 1e-3)).max() if seen.any() else 0.0
        print(f"{IDS[i]}: {int(ok.sum())} chains, trials {[int(s) & 63 for s in gstatus]}; coordinates that differ "
              f"{(u > 0).mean():.3%}, largest {int(u.max())} ulp; |xyz - X_ref| / |X| {dX:.3g}; cost {dc:.3g}; bone {db:.3g}; "
              f"resid {dr:.3g}")
        assert u.max() <= 1
        assert dc <= 1e-9
        assert db <= 1e-5
        assert np.array_equal(np.isnan(resid[:, ok]), ~seen)
        assert dr <= 1e-5          # float32 outputs of an fp64 sum: 2^-24 and the state's 1e-9


def test_one_joint_per_group_is_the_trajectory_fit():
    """J = 1, n_seg = 0 against ops.trajectory_fit on the same inputs: status equal, out_xyz within
    one ulp, cost within rtol 1e-9."""
    i = sc.J1_CASE
    c = sc.case(i)
    args, kw = dev_args(c)
    txyz, tresid, tnviews, tcost, tstatus = [o.cpu().numpy() for o in ops.trajectory_fit(
        *args, lambda_smooth=c["lam"], max_iter=c["max_iter"], tol=sc.TOL, chunk=c["chunk"], **kw)]
    xyz, resid, nviews, bone, cost, gstatus, cstatus = gpu_fit(i)
    assert bone.shape == (c["kpts"].shape[0], 3, 0)
    assert np.array_equal(gstatus, tstatus) and np.array_equal(cstatus, tstatus & 0x80)
    ok = tstatus != sk.INVALID
    assert ok.sum() == 2
    assert ulps(xyz[:, ok], txyz[:, ok]).max() <= 1
    assert np.array_equal(xyz[:, ~ok].view(np.uint32), txyz[:, ~ok].view(np.uint32))
    assert (np.abs(cost[ok, :2] - tcost[ok]) / np.abs(tcost[ok])).max() <= 1e-9
    assert (cost[ok, 2:] == 0).all() and np.isnan(cost[~ok]).all()
    assert np.array_equal(nviews, tnviews) and np.array_equal(np.isnan(resid), np.isnan(tresid))


@pytest.mark.parametrize("i", [2, 4, 7], ids=[IDS[k] for k in (2, 4, 7)])
def test_two_calls_are_bit_equal(i):
    c = sc.case(i)
    args, kw = dev_args(c)
    again = ops.skeleton_fit(*args, *skel_args(c), lambda_bone=c["beta"], lambda_smooth=c["lam"], max_iter=c["max_iter"],
                             tol=sc.TOL, chunk=c["chunk"], **kw)
    for a, b in zip(gpu_fit(i), again):
        assert np.array_equal(a.view(np.uint8), b.cpu().numpy().view(np.uint8))


@pytest.mark.parametrize("i", sc.CHUNK_CASES, ids=[IDS[k] for k in sc.CHUNK_CASES])
def test_chunk_4_and_automatic_agree(i):
    """The result does not depend on the chunk length beyond fp64 rounding."""
    a, b = gpu_fit(i, 4), gpu_fit(i, 0)
    kw = sc.CASES[i]
    assert ops.skeleton_fit_plan(kw["T"], kw["G"] * kw["J"], kw["J"], 0)[0] != 4
    assert np.array_equal(a[5], b[5]) and np.array_equal(a[6], b[6])
    ok = a[6] != sk.INVALID
    assert ulps(a[0][:, ok], b[0][:, ok]).max() <= 1


def test_max_iter_0_returns_the_seed_with_its_cost():
    i = 3
    c = sc.case(i)
    xyz, resid, nviews, bone, cost, gstatus, cstatus = gpu_fit(i, max_iter=0)
    r = sc.reference_fit(i)
    ok = r["group_status"] != sk.INVALID
    assert (gstatus[ok] == 0x40).all() and (gstatus[~ok] == 0x80).all()
    assert np.array_equal(cstatus, r["chain_status"])
    assert np.array_equal(xyz.view(np.uint32), c["xyz0"].view(np.uint32))
    assert np.allclose(cost[ok, 0], r["cost"][ok, 0], rtol=1e-9) and np.allclose(cost[ok, 2], r["cost"][ok, 2], rtol=1e-9)
    assert np.array_equal(cost[ok, 0], cost[ok, 1]) and np.array_equal(cost[ok, 2], cost[ok, 3])
    assert np.isnan(cost[~ok]).all()


def test_arm_scene_on_the_device():
    """The scene of test_skeleton_fit.py through the public path: smooth_trajectory's gap-filled seed
    from the two-view frames' points, refine.fit_skeleton on all 17 joints with the 12 segments.  The
    RMS over the lost joints must be below the blind fill's by half the factor the restatement
    reaches, and the person must converge."""
    a = sc.arm_scene()
    params = syn.reference_camera_params(a["cams"])
    seed = refine.smooth_trajectory(torch.tensor(a["tri"], device=DEV), lambda_smooth=sc.ARM_LAMBDA, sigma0=1.0)
    fit, info = refine.fit_skeleton(torch.tensor(a["kpts"], device=DEV), params, seed,
                                    segments=(a["pairs"], a["lengths"]), lambda_bone=sc.ARM_BETA, camera_indices=[0, 1],
                                    weights="conf", lambda_smooth=sc.ARM_LAMBDA, max_iter=sc.ARM_MAX_ITER, tol=sc.ARM_TOL,
                                    return_info=True)
    s, f = sc.arm_rms(seed.cpu().numpy(), a["truth"]), sc.arm_rms(fit.cpu().numpy(), a["truth"])
    print(f"gap RMS: blind fill {s:.3f} cm, fit with bones {f:.3f} cm, factor {s / f:.3f} (restatement: {sc.ARM_FACTOR}); "
          f"status {int(info['group_status']):#x}")
    assert int(info["group_status"]) & 0xC0 == 0 and (info["chain_status"] == 0).all()
    assert info["bone"].shape == (120, 12) and info["cost"].shape == (4,)
    assert s / f >= sc.ARM_FACTOR / 2


def test_people_are_groups():
    """(T, Np, J, 3, V) is Np people of J joints: the same numbers as one person at a time, with a
    row of lengths per person."""
    c = sc.case(4)
    T, J = c["kpts"].shape[0], c["J"]
    params = syn.reference_camera_params(c["cams"])
    k3 = torch.tensor(c["kpts"].reshape(T, 3, J, 3, 2), device=DEV)
    s3 = torch.tensor(c["xyz0"].reshape(T, 3, J, 3), device=DEV)
    kw = dict(camera_indices=c["cam_idx"], weights="conf", lambda_smooth=c["lam"], min_conf=sc.MIN_CONF, max_iter=12,
              tol=sc.TOL, return_info=True)
    all3, info3 = refine.fit_skeleton(k3, params, s3, segments=(c["pairs"], c["lengths"]), **kw)
    one, info1 = refine.fit_skeleton(k3[:, 1].contiguous(), params, s3[:, 1].contiguous(),
                                     segments=(c["pairs"], c["lengths"][1]), **kw)
    assert all3.shape == (T, 3, J, 3) and info3["bone"].shape == (T, 3, 12) and info3["group_status"].shape == (3,)
    assert torch.equal(all3[:, 1].view(torch.int32), one.view(torch.int32))
    assert torch.equal(info3["bone"][:, 1].view(torch.int32), info1["bone"].view(torch.int32))
    assert int(info3["group_status"][1]) == int(info1["group_status"])


def test_cli_skeleton_fit_type(tmp_path):
    """pose_refinement's skeleton_fit type on a tiny run directory (T = 12): it writes its two files,
    and they equal the direct fit_skeleton call from smooth_trajectory's seed bit for bit."""
    T = 12
    cams = syn.make_rig(2, seed=3)
    truth = syn.make_poses(T, seed=5, jitter=0.5)
    kpts = syn.make_kpts_2d(truth, cams, seed=6, noise_px=1.0)
    kpts[4:9, 7, :2, 1] = np.nan
    k3 = (truth + np.random.default_rng(7).normal(0.0, 1.0, truth.shape)).astype(np.float32)
    k3[4:9, 7] = np.nan
    run = tmp_path / "recordings" / "run"
    ext, intr = tmp_path / "extrinsic_camera_parameters", tmp_path / "intrinsic_camera_parameters"
    run.mkdir(parents=True)
    params = write_camera_folders(cams, ext, intr)
    np.save(run / "kpts_2d.npy", kpts)
    np.save(run / "kpts_3d.npy", k3)
    with open(run / "lengths.yaml", "w") as f:
        yaml.safe_dump({"my_lengths": dict(sc.BODY_LENGTHS)}, f, sort_keys=False)
    with open(run / "params.yaml", "w") as f:
        yaml.safe_dump({"smooth": {"lambda_smooth": 0.5}, "skeleton_fit": {"lambda_bone": 2.0, "lambda_smooth": 0.5,
                                                                           "max_iter": 20}}, f)
    out = cli.pose_refinement_main(["--run_path", str(run), "--refinement_types", "skeleton_fit", "--kpts_2d",
                                    str(run / "kpts_2d.npy"), "--kpts_3d", str(run / "kpts_3d.npy"),
                                    "--extrinsic_params_dir", str(ext), "--intrinsic_params_dir", str(intr),
                                    "--body_part_lengths_yaml", str(run / "lengths.yaml"), "--refinement_params_yaml",
                                    str(run / "params.yaml")])
    assert out["skeleton_fit"] == os.path.join(str(run), "kpts_3d_skeleton_fit.npy")
    got, got_resid = np.load(out["skeleton_fit"]), np.load(run / "kpts_3d_skeleton_fit_resid.npy")
    seed = refine.smooth_trajectory(k3, lambda_smooth=0.5)
    want, info = refine.fit_skeleton(kpts, params, seed, body_lengths=dict(sc.BODY_LENGTHS), lambda_bone=2.0,
                                     lambda_smooth=0.5, max_iter=20, return_info=True)
    assert got.shape == (T, 17, 3) and got.dtype == np.float32 and np.isfinite(got).all()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got_resid.view(np.uint32), info["resid"].view(np.uint32))
    assert not np.array_equal(got, seed)
    # nobody measured the lengths: the medians of kpts_3d's frames (joint 7 has 7 frames, below
    # min_frames, so its two segments are off)
    from mvpose import people
    cli.pose_refinement_main(["--run_path", str(run), "--refinement_types", "skeleton_fit", "--kpts_2d",
                              str(run / "kpts_2d.npy"), "--kpts_3d", str(run / "kpts_3d.npy"), "--extrinsic_params_dir",
                              str(ext), "--intrinsic_params_dir", str(intr), "--ignore_body_lengths",
                              "--refinement_params_yaml", str(run / "params.yaml")])
    pairs = np.array(list(refine.SEGMENTS.values()), np.int32)
    lengths = people.estimate_bone_lengths(torch.tensor(k3), pairs)
    off = [s for s, (a, b) in enumerate(pairs) if 7 in (a, b)]
    assert len(off) == 2 and torch.isnan(lengths[off]).all() and int(torch.isfinite(lengths).sum()) == len(pairs) - 2
    want2 = refine.fit_skeleton(kpts, params, seed, segments=(pairs, lengths), lambda_bone=2.0, lambda_smooth=0.5,
                                max_iter=20)
    got2 = np.load(out["skeleton_fit"])
    assert np.array_equal(got2.view(np.uint32), want2.view(np.uint32)) and not np.array_equal(got2, got)
    with pytest.raises(ValueError, match="skeleton_fit"):
        cli.pose_refinement_main(["--run_path", str(run), "--refinement_types", "no_such_type", "--kpts_3d",
                                  str(run / "kpts_3d.npy")])


def write_camera_folders(cams, ext, intr):
    """The camera files the command line reads, written by the package's own writers; returns the
    parameters read back through the loaders the command line uses."""
    from mvpose import geometry
    names = [f"cam{i}" for i in range(len(cams))]
    for name, c in zip(names, cams):
        geometry.write_camera_parameters(name, c["K"], c["dist"], str(intr))
        geometry.write_rotation_translation(name, c["R"], c["T"], str(ext))
    geometry.save_camera_names(str(ext), dict(enumerate(names)), names[0])
    cameras, _ = geometry.load_camera_names(str(ext))
    return {i: geometry.get_params_from_name(cameras[i], intrinsic_params_dir=str(intr),
                                             extrinsic_params_dir=str(ext))[1] for i in cameras}
