"""GPU: the maximum-likelihood refinement kernel (mvp_triangulate_refine) against its fp64 numpy
restatement (tests/tri_refine_ref.py, checked on the CPU in test_triangulate_refine.py), and the
Python / command-line fronts built on it.

Bounds (include/mvpose.h states the algorithm; both sides run it in fp64 from the same float32
seed, so they differ by summation order and FMA contraction only):
  xyz   within 1e-4 world units of the restatement's float32 point (the two fp64 minimisers
        differ by ~1e-7 or less; a float32 store at |coordinate| < 512 rounds to 6.1e-5 at most);
  cov   rtol 1e-4 + atol 1e-5 x the point's largest diagonal entry;
  cost  rtol 1e-5 + atol 1e-6;
  the failure (0x80) and not-converged (0x40) bits equal; trial counts may differ (an accept tie
  may go either way); failed points equal the seed bit for bit."""
import os

import numpy as np
import pytest
import torch

import tri_refine_ref as ref
from mvpose import synthetic as syn

pytestmark = pytest.mark.gpu
WEIGHTS = {"unit": ref.W_UNIT, "conf": ref.W_CONF, "heatmap": ref.W_GAUSS}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mvpose import ops as _ops
    return _ops


def make_case(T, J, V, seed, rig_seed=3):
    """cams, gt (T, J, 3), kpts (T, J, 3, V) f32, gauss (T, V, J, 6) f64: points around the subject,
    per-view anisotropic noise (eigenvalues 0.5..30 px²), Gaussians with the noise's covariance and
    a mean a fraction of a pixel off the keypoint (so the heatmap mode reads its own observation)."""
    rng = np.random.default_rng(seed)
    cams = syn.make_rig(V, seed=rig_seed)
    gt = syn.SUBJECT_CENTER + rng.uniform(-60.0, 60.0, (T, J, 3))
    kpts = np.zeros((T, J, 3, V), np.float32)
    gauss = np.zeros((T, V, J, 6))
    for v, cam in enumerate(cams):
        ev = rng.uniform(0.5, 30.0, (T, J, 2))
        th = rng.uniform(0, np.pi, (T, J))
        c, s = np.cos(th), np.sin(th)
        Rm = np.stack([np.stack([c, -s], -1), np.stack([s, c], -1)], -2)
        S = np.einsum("tjab,tjb,tjcb->tjac", Rm, ev, Rm)
        obs = syn.project(gt, cam) + np.einsum("tjab,tjb->tja", Rm, rng.normal(size=(T, J, 2)) * np.sqrt(ev))
        kpts[:, :, :2, v] = obs
        kpts[:, :, 2, v] = rng.uniform(0.3, 1.0, (T, J))
        gauss[:, v, :, :2] = obs + rng.uniform(-0.3, 0.3, (T, J, 2))
        gauss[:, v, :, 2], gauss[:, v, :, 3], gauss[:, v, :, 4], gauss[:, v, :, 5] = (
            S[..., 0, 0], S[..., 0, 1], S[..., 0, 1], S[..., 1, 1])
    return cams, gt, kpts, gauss


def run_device(ops, cams, kpts, ci, seed, weights, gauss=None, mask=None, **kw):
    cams_d = torch.tensor(ops.pack_cameras(syn.reference_camera_params(cams)), device="cuda")
    kd = torch.tensor(np.ascontiguousarray(kpts), device="cuda")
    sd = torch.tensor(np.ascontiguousarray(seed), device="cuda")
    gd = torch.tensor(np.ascontiguousarray(gauss), device="cuda") if weights == "heatmap" else None
    md = torch.tensor(mask, device="cuda") if mask is not None else None
    xyz, cov, cost, status = ops.triangulate_refine(kd, cams_d, ci, sd, weights=weights, gauss=gd, mask=md, **kw)
    torch.cuda.synchronize()
    return xyz.cpu().numpy(), cov.cpu().numpy(), cost.cpu().numpy(), status.cpu().numpy()


def run_reference(cams, kpts, ci, seed, weights, gauss=None, mask=None, **kw):
    V = kpts.shape[-1]
    bits = None
    if mask is not None:
        bits = (mask.reshape(-1, len(ci)).astype(np.int64) << np.arange(len(ci))).sum(1).astype(np.uint8)
    return ref.refine(kpts.reshape(-1, 3, V), cams, list(ci), seed.reshape(-1, 3), mask_bits=bits,
                      weights=WEIGHTS[weights], gauss=gauss if weights == "heatmap" else None, **kw)


def compare(dev, r, seed):
    xyz, cov, cost, status = dev
    lead = status.shape
    xyz, cost, status = xyz.reshape(-1, 3), cost.reshape(-1), status.reshape(-1)
    cov = cov.reshape(-1, 3, 3)
    seed = seed.reshape(-1, 3)
    assert xyz.dtype == np.float32 and cov.dtype == np.float32 and cost.dtype == np.float32 and status.dtype == np.uint8
    failed = (r["status"] & 0x80) != 0
    np.testing.assert_array_equal(status & 0x80, r["status"] & 0x80, err_msg=f"failure bits {lead}")
    np.testing.assert_array_equal(status & 0x40, r["status"] & 0x40, err_msg="not-converged bits")
    assert (status[failed] == 0x80).all()
    assert np.array_equal(xyz[failed].view(np.uint32), seed[failed].view(np.uint32)), "failed points must be the seed"
    assert np.isnan(cov[failed]).all() and np.isnan(cost[failed]).all()
    ok = ~failed
    d = np.abs(xyz[ok].astype(np.float64) - r["xyz"][ok].astype(np.float64))
    rcov = r["cov"][:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)
    np.testing.assert_array_equal(cov, cov.transpose(0, 2, 1))                     # symmetric
    np.testing.assert_array_equal(np.isnan(cov), np.isnan(rcov))
    fin = ok & np.isfinite(rcov).all((1, 2))
    atol = 1e-5 * np.max(np.abs(np.diagonal(rcov[fin], axis1=1, axis2=2)), axis=1)[:, None, None]
    cd = np.abs(cov[fin] - rcov[fin]) - (1e-4 * np.abs(rcov[fin]) + atol)
    print(f"n={len(status)} failed={int(failed.sum())} max|dxyz|={d.max() if d.size else 0:.3g} "
          f"cov excess={cd.max() if cd.size else 0:.3g} trials dev max={int((status[ok] & 63).max()) if ok.any() else 0} "
          f"ref max={int((r['status'][ok] & 63).max()) if ok.any() else 0}")
    assert (d <= 1e-4).all(), d.max()
    assert (cd <= 0).all(), cd.max()
    np.testing.assert_allclose(cost[ok], r["cost"][ok], rtol=1e-5, atol=1e-6)


def dlt(ops, cams, kpts, ci):
    cams_d = torch.tensor(ops.pack_cameras(syn.reference_camera_params(cams)), device="cuda")
    return ops.triangulate(torch.tensor(kpts, device="cuda"), cams_d, ci, mode=ops.TRI_ALL_VIEWS).cpu().numpy()


@pytest.mark.parametrize("weights", ["unit", "conf", "heatmap"])
@pytest.mark.parametrize("V", [2, 3, 4, 8])
def test_matches_restatement_on_clean_inputs(ops, V, weights):
    """n in {1, 65, 257, 6·17}, every listed view usable; every point converges within the default
    max_iter."""
    for T, J in ((1, 1), (65, 1), (257, 1), (6, 17)):
        cams, gt, kpts, gauss = make_case(T, J, V, seed=100 * V + T)
        ci = list(range(V))
        seed = dlt(ops, cams, kpts, ci)
        dev = run_device(ops, cams, kpts, ci, seed, weights, gauss)
        r = run_reference(cams, kpts, ci, seed, weights, gauss)
        assert (r["status"] & 0xC0 == 0).all()
        compare(dev, r, seed)
        assert (dev[3] & 0xC0 == 0).all()
        assert dev[0].shape == (T, J, 3) and dev[1].shape == (T, J, 3, 3) and dev[2].shape == (T, J)


@pytest.mark.parametrize("weights", ["unit", "heatmap"])
def test_subset_and_permutation_of_cameras(ops, weights):
    cams, gt, kpts, gauss = make_case(5, 17, 5, seed=21)
    ci = [3, 0, 4]
    seed = dlt(ops, cams, kpts, ci)
    compare(run_device(ops, cams, kpts, ci, seed, weights, gauss), run_reference(cams, kpts, ci, seed, weights, gauss),
            seed)


@pytest.mark.parametrize("V", [4, 8])
def test_masks_from_the_robust_triangulation(ops, V):
    """One view of every third point pushed 80 px: triangulate_robust drops it, and its inlier mask
    and point seed the refinement, which must then ignore the pushed view."""
    cams, gt, kpts, gauss = make_case(4, 17, V, seed=33)
    kpts[:, :, :2, :] = np.stack([syn.project(gt, c) for c in cams], -1)     # 1 px noise: clean inliers
    kpts[:, :, :2, :] += np.random.default_rng(5).normal(0, 1.0, kpts[:, :, :2, :].shape).astype(np.float32)
    flat = kpts.reshape(-1, 3, V)
    flat[::3, 0, 1] += 80.0
    cams_d = torch.tensor(ops.pack_cameras(syn.reference_camera_params(cams)), device="cuda")
    ci = list(range(V))
    xyz, inl, _ = ops.triangulate_robust(torch.tensor(kpts, device="cuda"), cams_d, ci, inlier_px=10.0)
    seed, mask = xyz.cpu().numpy(), inl.cpu().numpy()
    assert (~mask.reshape(-1, V)[::3, 1]).all() and mask.reshape(-1, V)[1::3].all()
    for weights in ("unit", "conf"):
        dev = run_device(ops, cams, kpts, ci, seed, weights, mask=mask)
        r = run_reference(cams, kpts, ci, seed, weights, mask=mask)
        assert not r["used"][::3, 1].any()
        compare(dev, r, seed)
        err = np.linalg.norm(dev[0].reshape(-1, 3) - gt.reshape(-1, 3), axis=1)
        assert err.max() < 5.0                # the pushed view moved nothing: 80 px would be ~25 cm


def test_invalid_views_and_failures(ops):
    """NaN x, conf < min_conf, an all-zero Gaussian, a Gaussian that is not positive definite, points
    left with fewer than 2 used views, a NaN seed and a seed behind a camera."""
    for V, weights in ((2, "unit"), (3, "heatmap"), (4, "heatmap"), (4, "conf")):
        cams, gt, kpts, gauss = make_case(6, 17, V, seed=40 + V)
        ci = list(range(V))
        seed = dlt(ops, cams, kpts, ci)
        k, g, s = kpts.reshape(-1, 3, V), gauss.transpose(0, 2, 1, 3).reshape(-1, V, 6).copy(), seed.reshape(-1, 3)
        k[0::7, 0, 0] = np.nan                       # view 0 unusable
        k[3::11, 1, V - 1] = np.inf
        g[2::5, 1] = 0.0                             # empty heatmap in view 1
        g[4::9, 0, 2:] = [1.0, 5.0, 5.0, 1.0]        # + floor·I: det < 0
        g[6::13, V - 1, 3] = np.nan
        k[5, 0, :] = np.nan                          # no view at all
        k[8, 0, 1:] = np.nan                         # one view
        s[9] = [0.0, 0.0, -500.0]                    # behind camera 0
        k[9, 2, :] = 0.9                             # ... which is used
        s[10, 2] = np.nan
        gauss2 = np.ascontiguousarray(g.reshape(6, 17, V, 6).transpose(0, 2, 1, 3))
        kw = dict(min_conf=0.4)
        dev = run_device(ops, cams, kpts, ci, seed, weights, gauss2, **kw)
        r = run_reference(cams, kpts, ci, seed, weights, gauss2, **kw)
        assert (r["status"][[5, 8, 9, 10]] == 0x80).all()
        if V > 2:
            assert (r["status"] & 0x80 == 0).sum() > 60
        compare(dev, r, seed)


@pytest.mark.parametrize("weights", ["unit", "heatmap"])
def test_max_iter_zero_and_one(ops, weights):
    cams, gt, kpts, gauss = make_case(3, 17, 4, seed=50)
    ci = [0, 1, 2, 3]
    seed = dlt(ops, cams, kpts, ci)
    dev = run_device(ops, cams, kpts, ci, seed, weights, gauss, max_iter=0)
    r = run_reference(cams, kpts, ci, seed, weights, gauss, max_iter=0)
    compare(dev, r, seed)
    assert np.array_equal(dev[0].view(np.uint32), seed.view(np.uint32)) and (dev[3] == 0x40).all()
    assert np.isfinite(dev[1]).all() and np.isfinite(dev[2]).all()
    off = (seed + np.float32(5.0 / np.sqrt(3.0))).astype(np.float32)          # 5 cm off
    dev = run_device(ops, cams, kpts, ci, off, weights, gauss, max_iter=1)
    r = run_reference(cams, kpts, ci, off, weights, gauss, max_iter=1)
    compare(dev, r, off)
    assert (dev[3] == 0x41).all()


def test_rms_error_on_heteroscedastic_views(ops):
    """On the heteroscedastic inputs (V = 4, true covariances) the kernel's rms error against
    ground truth is within 0.1 % of the restatement's."""
    cams, gt, kpts, gauss = ref.hetero_inputs(4)
    ci = [0, 1, 2, 3]
    seed = ref.dlt_seed(kpts, cams, ci).reshape(kpts.shape[0], 17, 3)
    dev = run_device(ops, cams, kpts, ci, seed, "heatmap", gauss, cov_floor=0.0)
    r = run_reference(cams, kpts, ci, seed, "heatmap", gauss, cov_floor=0.0)
    compare(dev, r, seed)
    rms_d = np.sqrt(((dev[0].reshape(-1, 3) - gt) ** 2).sum(1).mean())
    rms_r = np.sqrt(((r["X"] - gt) ** 2).sum(1).mean())
    print(f"rms device {rms_d:.5f} restatement {rms_r:.5f}")
    assert abs(rms_d / rms_r - 1) <= 1e-3


def test_argument_checks_of_the_front(ops):
    cams, gt, kpts, gauss = make_case(2, 17, 3, seed=1)
    cams_d = torch.tensor(ops.pack_cameras(syn.reference_camera_params(cams)), device="cuda")
    kd, sd = torch.tensor(kpts, device="cuda"), torch.zeros((2, 17, 3), device="cuda")
    with pytest.raises(ValueError):
        ops.triangulate_refine(kd, cams_d, [0, 1, 2], sd, weights="huber")
    with pytest.raises(ValueError):
        ops.triangulate_refine(kd, cams_d, [0, 1, 2], sd, weights="heatmap")
    with pytest.raises(ValueError):
        ops.triangulate_refine(kd, cams_d, [0, 1, 2], sd[:1])
    with pytest.raises(ValueError):
        ops.triangulate_refine(kd, cams_d, [0, 1, 2], sd, weights="heatmap",
                               gauss=torch.zeros((2, 17, 3, 6), dtype=torch.float64, device="cuda"))
    with pytest.raises(TypeError):
        ops.triangulate_refine(kd, cams_d, [0, 1, 2], sd, mask=torch.ones((2, 17, 3), device="cuda"))


# ------------------------------------------------------------------ the fronts
@pytest.mark.parametrize("method,refine", [("reference", "unit"), ("all_views", "conf"), ("robust", "heatmap")])
def test_get_pose_3d_refine_equals_ops(ops, method, refine):
    from mvpose import pose_estimation
    cams, gt, kpts, gauss = make_case(3, 17, 3, seed=60)
    kpts.reshape(-1, 3, 3)[::4, 0, 2] += 60.0
    params = syn.reference_camera_params(cams)
    out, info = pose_estimation.get_pose_3D(params, kpts, method=method, refine=refine, heatmaps_2d=gauss,
                                            cov_floor=0.5, return_info=True)
    plain, pinfo = pose_estimation.get_pose_3D(params, kpts, method=method, return_info=True)
    assert "cov" not in pinfo
    np.testing.assert_array_equal(info["seed"], plain)
    mask = info["inliers"] if method == "robust" else None
    ci = [0, 1, 2]
    dev = run_device(ops, cams, kpts, ci, plain, refine, gauss, mask=mask, cov_floor=0.5)
    np.testing.assert_array_equal(out, dev[0])
    np.testing.assert_array_equal(info["cov"], dev[1])
    np.testing.assert_array_equal(info["refine_cost"], dev[2])
    np.testing.assert_array_equal(info["refine_status"], dev[3])
    assert info["cov"].shape == (3, 17, 3, 3) and (info["refine_status"] & 0x80 == 0).any()


@pytest.fixture(scope="module")
def refine_pipe(ops):
    from mvpose import pipeline
    cams = syn.make_rig(3, seed=3)
    p = pipeline.MultiViewPipeline(syn.reference_camera_params(cams), camera_indices=(0, 1, 2),
                                   mode=ops.TRI_ALL_VIEWS, max_frames=12, seed=5, refine="heatmap", cov_floor=1.0)
    return p


def test_pipeline_refine_outputs(ops, refine_pipe):
    """MultiViewPipeline(refine="heatmap"): kpts_3d is ops.triangulate_refine of the pipeline's own
    kpts_2d, heatmaps_2d and seed; every point that did not fail has a finite covariance."""
    p = refine_pipe
    T = 3
    frames = torch.tensor(syn.make_frames(T * 3, seed=1).reshape(T, 3, 720, 1280, 3), device="cuda")
    out = p.process(frames)
    torch.cuda.synchronize()
    assert out["kpts_3d"].shape == (T, 17, 3) and out["kpts_3d_seed"].shape == (T, 17, 3)
    assert out["kpts_3d_cov"].shape == (T, 17, 3, 3) and out["kpts_3d_cov"].dtype == torch.float32
    assert out["tri_refine_cost"].shape == (T, 17) and out["tri_refine_status"].dtype == torch.uint8
    seed = ops.triangulate(out["kpts_2d"], p.cams, [0, 1, 2], mode=ops.TRI_ALL_VIEWS)
    assert torch.equal(torch.nan_to_num(seed), torch.nan_to_num(out["kpts_3d_seed"]))
    xyz, cov, cost, status = ops.triangulate_refine(out["kpts_2d"], p.cams, [0, 1, 2], seed, weights="heatmap",
                                                    gauss=out["heatmaps_2d"], cov_floor=1.0)
    assert torch.equal(torch.nan_to_num(xyz), torch.nan_to_num(out["kpts_3d"]))
    assert torch.equal(torch.nan_to_num(cov), torch.nan_to_num(out["kpts_3d_cov"]))
    assert torch.equal(status, out["tri_refine_status"])
    ok = (status & 0x80) == 0
    print(f"refined {int(ok.sum())} of {ok.numel()} points")
    assert ok.any()
    assert torch.isfinite(out["kpts_3d_cov"][ok]).all() and torch.isfinite(out["kpts_3d"][ok]).all()


def test_pipeline_refine_with_overlapped_moments(refine_pipe):
    """The refinement reads heatmaps_2d, which overlap_moments computes on a side stream: the
    outputs are bit-identical to the serial path's, across buffer reuse."""
    p = refine_pipe
    T = 3
    fa = torch.tensor(syn.make_frames(T * 3, seed=11).reshape(T, 3, 720, 1280, 3), device="cuda")
    fb = torch.tensor(syn.make_frames(T * 3, seed=12).reshape(T, 3, 720, 1280, 3), device="cuda")
    serial = [{k: v.clone() for k, v in p.process(f).items()} for f in (fa, fb)]
    outs = [p.process(f, {}, overlap_moments=True) for f in (fa, fb, fa, fb)]
    torch.cuda.synchronize()
    for i, o in enumerate(outs):
        for k in ("kpts_2d", "heatmaps_2d", "kpts_3d", "kpts_3d_seed", "kpts_3d_cov", "tri_refine_cost",
                  "tri_refine_status"):
            assert torch.equal(torch.nan_to_num(o[k]), torch.nan_to_num(serial[i % 2][k])), (i, k)


def test_pipeline_without_refine_is_unchanged(ops):
    from mvpose import pipeline
    cams = syn.make_rig(2, seed=3)
    p = pipeline.MultiViewPipeline(syn.reference_camera_params(cams), max_frames=4, seed=5)
    frames = torch.tensor(syn.make_frames(4, seed=1).reshape(2, 2, 720, 1280, 3), device="cuda")
    assert sorted(p.process(frames)) == ["heatmaps_2d", "kpts_2d", "kpts_3d"]


def test_cli_writes_the_refinement_files(ops, tmp_path, monkeypatch):
    """record_and_estimate_pose on .npy recordings: only the reference's files without --refine;
    with it also the seed, the covariances and the status, the settings in recording_log.yaml."""
    import yaml
    from mvpose import cli, geometry
    cams = syn.make_rig(3, seed=4)
    ext = tmp_path / "configurations" / "1" / "extrinsic_camera_parameters"
    names = ["camA", "camB", "camC"]
    for name, c in zip(names, cams):
        geometry.write_camera_parameters(name, c["K"], c["dist"], str(tmp_path / "intrinsic_camera_parameters"))
        geometry.write_rotation_translation(name, c["R"], c["T"], str(ext))
    geometry.save_camera_names(str(ext), dict(enumerate(names)), "camA")
    rec = tmp_path / "configurations" / "1" / "recordings" / "0"
    rec.mkdir(parents=True)
    rng = np.random.default_rng(0)
    paths = []
    for v in range(3):
        np.save(rec / f"camera{v}.npy", rng.integers(0, 256, (3, 360, 640, 3), dtype=np.uint8))
        paths.append(str(rec / f"camera{v}.npy"))
    monkeypatch.setenv("MVPOSE_RANDOM_WEIGHTS", "1")
    monkeypatch.setenv("MVPOSE_NO_DETECTOR", "1")
    monkeypatch.chdir(tmp_path)
    argv = ["--camera_names", *names, "--configuration_number", "1", "--recording_paths", *paths]
    inputs = {f"camera{v}.npy" for v in range(3)}
    cli.record_and_estimate_pose_main(argv)
    assert set(os.listdir(rec)) - inputs == {"kpts_2d.npy", "heatmaps_2d.npy", "kpts_3d.npy", "recording_log.yaml"}
    plain3 = np.load(rec / "kpts_3d.npy")
    with open(rec / "recording_log.yaml") as f:
        assert "refine" not in yaml.safe_load(f)
    log = cli.record_and_estimate_pose_main(argv + ["--triangulation", "all_views", "--refine", "heatmap",
                                                    "--cov_floor", "2.0"])
    assert set(os.listdir(rec)) - inputs == {
        "kpts_2d.npy", "heatmaps_2d.npy", "kpts_3d.npy", "recording_log.yaml", "kpts_3d_inliers.npy",
        "kpts_3d_seed.npy", "kpts_3d_cov.npy", "kpts_3d_refine_status.npy"}
    with open(rec / "recording_log.yaml") as f:
        saved = yaml.safe_load(f)
    assert saved["refine"] == "heatmap" and saved["cov_floor"] == 2.0 and saved["kpts_3d_cov"] == log["kpts_3d_cov"]
    k3, s3, cov, st = (np.load(rec / f"{n}.npy") for n in ("kpts_3d", "kpts_3d_seed", "kpts_3d_cov",
                                                           "kpts_3d_refine_status"))
    assert k3.shape == (2, 17, 3) and k3.dtype == np.float32 and s3.shape == (2, 17, 3)
    assert cov.shape == (2, 17, 3, 3) and cov.dtype == np.float32 and st.shape == (2, 17) and st.dtype == np.uint8
    assert plain3.shape == (2, 17, 3)
    failed = (st & 0x80) != 0
    assert np.array_equal(k3[failed].view(np.uint32), s3[failed].view(np.uint32))
    assert np.isfinite(cov[~failed]).all()
