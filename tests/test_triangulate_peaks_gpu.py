"""GPU: peak-selecting triangulation (mvp_triangulate_peaks) against the numpy restatement of
tests/tri_peaks_ref.py on the cases of tests/tri_peaks_cases.py, whose margins the CPU suite
checks (tests/test_triangulate_peaks.py): given those, masks and selections are determined
whatever the rounding order, the float32 points must be BIT-identical (the final solve is the
oracle's DLT over exactly the masked views' selected candidates) and the errors agree to the
robust test's rtol 1e-6 + atol 1e-6 px."""
import ctypes

import numpy as np
import pytest
import torch

from mvpose import synthetic as syn
import tri_peaks_cases as cases
from tri_peaks_ref import INLIER_PX, MIN_MARGIN, PeaksReference
from test_triangulate_robust_gpu import _bits_equal, contaminated

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mvpose import ops as _ops
    return _ops


def _cams_dev(ops, cams):
    return torch.tensor(ops.pack_cameras(syn.reference_camera_params(cams)), device="cuda")


def _device(ops, cams, peaks, ci, **kw):
    out = ops.triangulate_peaks(torch.tensor(np.ascontiguousarray(peaks), device="cuda"), _cams_dev(ops, cams), ci, **kw)
    torch.cuda.synchronize()
    xyz, inl, sel, err, kp = out
    assert (xyz.dtype, inl.dtype, sel.dtype, err.dtype, kp.dtype) == (torch.float32, torch.bool, torch.int8,
                                                                      torch.float32, torch.float32)
    return tuple(a.cpu().numpy() for a in out)


def _compare(ops, cams, peaks, ci, ref=None, res=None, **kw):
    """Device vs reference on the same input: margins, masks, selections, bits, errors, kpts."""
    if res is None:
        ref = PeaksReference(cams, ci)
        res = ref(peaks, **kw)
    rx, rm, rs, re = res
    print(f"reference: margin {ref.margin:.3g} px, candidate gap {ref.gap:.3g} px")
    assert ref.margin > MIN_MARGIN and ref.gap > MIN_MARGIN
    dx, dm, ds, de, dk = _device(ops, cams, peaks, ci, **kw)
    assert np.array_equal(dm, rm), f"{(dm != rm).any(-1).sum()} masks differ"
    assert np.array_equal(ds, rs), f"{(ds != rs).any(-1).sum()} selections differ"
    _bits_equal(dx, rx)
    np.testing.assert_allclose(de, re, rtol=1e-6, atol=1e-6, equal_nan=True)
    assert np.array_equal(dk, ref.select(peaks, rm, rs), equal_nan=True)
    return dx, dm, ds, de, dk


# ------------------------------------------------------------------ 1. one slot = the robust kernel
@pytest.mark.parametrize("V,seed", [(3, 1), (4, 2), (8, 3)])
def test_one_slot_is_triangulate_robust(ops, V, seed):
    cams, k, truth = contaminated(V, seed, max_bad=3 if V == 8 else 1)
    if V == 3:
        k[:, :, 2, :][~truth] = 0.05
    ci = list(range(V))
    kd, cd = torch.tensor(k, device="cuda"), _cams_dev(ops, cams)
    rx, rm, re = ops.triangulate_robust(kd, cd, ci, inlier_px=INLIER_PX)
    px, pm, ps, pe, pk = ops.triangulate_peaks(kd[:, :, None].contiguous(), cd, ci, inlier_px=INLIER_PX)
    assert torch.equal(pm, rm) and np.array_equal(pm.cpu().numpy(), truth)
    assert torch.equal(px.view(torch.int32), rx.view(torch.int32))
    np.testing.assert_allclose(pe.cpu().numpy(), re.cpu().numpy(), rtol=1e-6, atol=1e-6, equal_nan=True)
    assert torch.equal(ps, torch.where(rm, 0, -1).to(torch.int8))
    assert torch.equal(pk.view(torch.int32), kd.view(torch.int32))


# ------------------------------------------------------------------ 2. several slots
@pytest.mark.parametrize("V,M", cases.CASES)
def test_masks_selections_and_bits(ops, V, M):
    cams, peaks, tmask, tslot, ref, res = cases.case_with_reference(V, M)
    dx, dm, ds, de, dk = _compare(ops, cams, peaks, list(range(V)), ref=ref, res=res, inlier_px=INLIER_PX,
                                  min_conf=cases.MIN_CONF)
    assert np.array_equal(dm, tmask) and np.array_equal(ds, tslot)
    assert np.isfinite(dx).all() and (de[dm] <= INLIER_PX).all()


# ------------------------------------------------------------------ 3. other cases
@pytest.mark.parametrize("n", [1, 64, 65])
def test_sizes(ops, n):
    cams, peaks, _, _, _, _ = cases.case_with_reference(4, 2)
    _compare(ops, cams, np.ascontiguousarray(peaks.reshape(-1, 2, 3, 4)[:n]), [0, 1, 2, 3], inlier_px=INLIER_PX,
             min_conf=cases.MIN_CONF)


def test_listed_subset_in_any_order(ops):
    """View i reads column cam_idx[i] with camera cam_idx[i]'s parameters; the columns that are
    not listed keep slot 0 in out_kpts."""
    cams, peaks, tmask, tslot, _, _ = cases.case_with_reference(8, 2)
    ci = [6, 0, 3, 5, 2]
    dx, dm, ds, de, dk = _compare(ops, cams, np.ascontiguousarray(peaks[:4]), ci, inlier_px=INLIER_PX,
                                  min_conf=cases.MIN_CONF)
    assert np.array_equal(dm, tmask[:4][..., ci]) and np.array_equal(ds, tslot[:4][..., ci])
    rest = [v for v in range(8) if v not in ci]
    assert np.array_equal(dk[..., rest], peaks[:4, :, 0][..., rest], equal_nan=True)


def test_behind_the_cameras_and_too_few_views(ops):
    """Every candidate of a point behind a camera of a distortion-free rig: +inf, not an inlier
    (the robust test's construction, with a second candidate 80-300 px off in every view); points
    with one valid view, or none, fail: NaN xyz, empty mask, every sel -1, NaN errors."""
    cams = syn.make_rig(4, seed=21, distortion=False)
    rng = np.random.default_rng(22)
    c = -cams[1]["R"].T @ cams[1]["T"].reshape(3)
    pts = np.array([c + t * (c - syn.SUBJECT_CENTER) + rng.normal(0, 20.0, 3) for t in rng.uniform(0.1, 0.6, 60)])
    depth = np.stack([(pts @ cm["R"].T + cm["T"].reshape(3))[:, 2] for cm in cams], -1)
    keep = (np.abs(depth) > 30).all(-1) & ((depth > 0).sum(-1) >= 2) & (depth[:, 1] < 0)
    pts, depth = pts[keep], depth[keep]
    n = len(pts)
    assert n >= 4
    peaks = np.zeros((n + 2, 2, 3, 4), np.float32)
    peaks[:, :, :2] = np.nan
    for v, cm in enumerate(cams):
        peaks[:n, 0, :2, v] = syn.project(pts, cm, distortion=False)
        r, th = rng.uniform(80.0, 300.0, (n, 1)), rng.uniform(0.0, 2 * np.pi, (n, 1))
        peaks[:n, 1, :2, v] = peaks[:n, 0, :2, v] + (r * np.hstack([np.cos(th), np.sin(th)])).astype(np.float32)
    peaks[:n, 0, 2], peaks[:n, 1, 2] = 0.9, 0.5
    peaks[n, 0, :, 2] = (640.0, 360.0, 0.9)                 # one valid view; the last point has none
    dx, dm, ds, de, dk = _compare(ops, cams, peaks, [0, 1, 2, 3])
    assert np.array_equal(dm[:n], depth > 0) and (ds[:n][depth > 0] == 0).all() and (ds[:n][depth < 0] == -1).all()
    assert np.isposinf(de[:n][depth < 0]).all()
    for p in (n, n + 1):
        assert np.isnan(dx[p]).all() and not dm[p].any() and (ds[p] == -1).all() and np.isnan(de[p]).all()
    assert np.array_equal(dk[n:], peaks[n:, 0], equal_nan=True)


def test_nullable_outputs(ops):
    """out_err and out_kpts NULL, each in turn: the other outputs do not change."""
    from mvpose import _lib
    cams, peaks, _, _, _, _ = cases.case_with_reference(4, 4)
    pd, cd = torch.tensor(peaks, device="cuda"), _cams_dev(ops, cams)
    want = ops.triangulate_peaks(pd, cd, [0, 1, 2, 3], min_conf=cases.MIN_CONF)
    n = peaks.shape[0] * peaks.shape[1]
    ci = (ctypes.c_int * 4)(0, 1, 2, 3)
    for drop in ("err", "kpts"):
        xyz, bits, sel = torch.empty_like(want[0]), torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty_like(want[2])
        err = None if drop == "err" else torch.empty_like(want[3])
        kp = None if drop == "kpts" else torch.empty_like(want[4])
        _lib.call("mvp_triangulate_peaks", _lib.ptr(pd), n, 4, 4, _lib.ptr(cd), 4, ci, 4, INLIER_PX, cases.MIN_CONF,
                  _lib.ptr(xyz), _lib.ptr(bits), _lib.ptr(sel), _lib.ptr(err), _lib.ptr(kp), _lib.stream(pd.device))
        assert torch.equal(xyz.view(torch.int32), want[0].view(torch.int32)) and torch.equal(sel, want[2])
        assert torch.equal(ops._unpack_view_bits(bits, 4).reshape(want[1].shape), want[1])
        if err is not None:
            assert torch.equal(err.view(torch.int32), want[3].view(torch.int32))
        if kp is not None:
            assert torch.equal(kp.view(torch.int32), want[4].view(torch.int32))


# ------------------------------------------------------------------ 4. the point of the feature
def test_a_wrong_argmax_is_recovered(ops):
    """Three views; in one of them the argmax (slot 0) is a decoy and the truth is the second mode.
    Robust triangulation of the argmaxes loses that view; the peak-selecting one keeps all three
    with the truth's slot, and hands on a kpts_2d with the mode corrected."""
    cams, peaks, tmask, tslot, _, _ = cases.case_with_reference(3, 2)
    peaks = peaks.copy()
    peaks[:, :, 0, 2][np.isnan(peaks[:, :, 0, 0])] = 0.0    # an unusable argmax stays unusable for the robust call
    pts = np.argwhere((tslot > 0).sum(-1) == 1)
    valid0 = np.isfinite(peaks[:, :, 0, 0]) & (peaks[:, :, 0, 2] >= cases.MIN_CONF)
    pts = [tuple(p) for p in pts if valid0[tuple(p)].all()]
    assert len(pts) >= 10
    t, j = map(np.array, zip(*pts))
    sub = np.ascontiguousarray(peaks[t, j])                                    # (n, 2, 3, 3)
    pd, cd = torch.tensor(sub, device="cuda"), _cams_dev(ops, cams)
    _, rmask, _ = ops.triangulate_robust(pd[:, 0].contiguous(), cd, [0, 1, 2], min_conf=cases.MIN_CONF)
    _, pmask, psel, _, pk = ops.triangulate_peaks(pd, cd, [0, 1, 2], min_conf=cases.MIN_CONF)
    decoy = tslot[t, j] > 0                                                    # (n, 3): the view whose argmax is wrong
    assert (rmask.sum(-1) == 2).all()
    assert pmask.all() and np.array_equal(psel.cpu().numpy(), tslot[t, j])
    pk = pk.cpu().numpy()
    assert np.array_equal(np.moveaxis(pk, 1, 2)[decoy], np.moveaxis(sub[:, 1], 1, 2)[decoy])
    assert np.array_equal(np.moveaxis(pk, 1, 2)[~decoy], np.moveaxis(sub[:, 0], 1, 2)[~decoy])


# ------------------------------------------------------------------ 5. stream, pipeline, drop-ins
def test_non_default_stream(ops):
    cams, peaks, _, _, _, _ = cases.case_with_reference(4, 4)
    pd, cd = torch.tensor(peaks, device="cuda"), _cams_dev(ops, cams)
    a = ops.triangulate_peaks(pd, cd, [0, 1, 2, 3], min_conf=cases.MIN_CONF)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        b = ops.triangulate_peaks(pd, cd, [0, 1, 2, 3], min_conf=cases.MIN_CONF)
    st.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))


def test_get_pose_3D_method(ops):
    from mvpose import pose_estimation as pe
    cams, peaks, tmask, tslot, _, (rx, rm, rs, re) = cases.case_with_reference(4, 2)
    cp = syn.reference_camera_params(cams)
    out, info = pe.get_pose_3D(cp, peaks[:, :, 0], camera_indices=[0, 1, 2, 3], method="peaks", peaks=peaks,
                               inlier_px=INLIER_PX, min_conf=cases.MIN_CONF, return_info=True)
    _bits_equal(out, rx)
    assert np.array_equal(info["inliers"], tmask) and np.array_equal(info["sel"], tslot)
    assert info["kpts_selected"].shape == peaks[:, :, 0].shape and info["reproj_err"].shape == tmask.shape


def test_pipeline_mode_and_estimator_peaks(ops):
    """Random weights, as the other pipeline tests: the TRI_PEAKS outputs equal the ops composition
    on the estimator's flip-averaged maps with the run's crop geometry; kpts_2d is the argmax."""
    from mvpose import pipeline
    cams = syn.make_rig(3, seed=51)
    cp = syn.reference_camera_params(cams)
    kw = dict(camera_indices=(0, 1, 2), inlier_px=15.0, min_conf=0.05, max_frames=3, seed=0)
    frames = torch.tensor(syn.make_frames(3, seed=52).reshape(1, 3, 720, 1280, 3), device="cuda")
    boxes = np.array([[[100.0, 50.0, 900.0, 700.0], [np.nan] * 4, [300.0, 10.0, 1200.0, 650.0]]])
    thr = -1e9                    # random weights: whatever the maps' values, every local maximum is a peak
    p = pipeline.MultiViewPipeline(cp, mode=ops.TRI_PEAKS, max_peaks=3, peak_thr=thr, peak_min_rel=0.2,
                                   refine="conf", **kw)
    out = p.process(frames, bboxes=boxes)
    geo = p.estimator._geo_dev[p.estimator._avg_k][2][:3]
    peaks, _ = ops.heatmap_peaks(p.estimator.avg[:3], geo, max_peaks=3, radius=1, thr=thr, min_rel=0.2, n_views=3)
    assert out["kpts_2d_peaks"].shape == (1, 17, 3, 3, 3)
    assert torch.equal(out["kpts_2d_peaks"].view(torch.int32), peaks.view(torch.int32))
    xyz, inl, sel, err, kp = ops.triangulate_peaks(peaks, p.cams, [0, 1, 2], inlier_px=15.0, min_conf=0.05)
    for name, want in (("kpts_3d_seed", xyz), ("tri_reproj_err", err), ("kpts_2d_selected", kp)):
        assert torch.equal(out[name].view(torch.int32), want.view(torch.int32)), name
    assert torch.equal(out["tri_inliers"], inl) and torch.equal(out["tri_peak_sel"], sel)
    ref = ops.triangulate_refine(kp, p.cams, [0, 1, 2], xyz, weights="conf", mask=inl, min_conf=0.05)[0]
    assert torch.equal(out["kpts_3d"].view(torch.int32), ref.view(torch.int32))
    # kpts_2d is the argmax decode, as without the mode, and the first mode is that keypoint
    assert torch.equal(out["kpts_2d_peaks"][:, :, 0].view(torch.int32), out["kpts_2d"].view(torch.int32))
    r = p.estimator.run(frames.reshape(3, 720, 1280, 3), bboxes=boxes.reshape(3, 4))
    k2 = torch.cat([r["keypoints"], r["scores"][..., None]], -1).permute(1, 2, 0)[None]      # (1, 17, 3, V)
    assert "peaks" not in r and torch.equal(out["kpts_2d"].view(torch.int32), k2.contiguous().view(torch.int32))


def test_cli_writes_the_peak_files(ops, tmp_path, monkeypatch):
    """record_and_estimate_pose --triangulation peaks on three recordings (random weights, no
    detector): kpts_2d_peaks.npy and the settings in recording_log.yaml; the saved peaks then
    serve a run that does not repeat the 2D stage, and their absence is named."""
    import yaml
    from mvpose import cli, geometry, pose_estimation as pe
    cams = syn.make_rig(3, seed=71)
    ext = tmp_path / "configurations" / "1" / "extrinsic_camera_parameters"
    names = ["camA", "camB", "camC"]
    for name, c in zip(names, cams):
        geometry.write_camera_parameters(name, c["K"], c["dist"], str(tmp_path / "intrinsic_camera_parameters"))
        geometry.write_rotation_translation(name, c["R"], c["T"], str(ext))
    geometry.save_camera_names(str(ext), dict(enumerate(names)), "camA")
    monkeypatch.setenv("MVPOSE_RANDOM_WEIGHTS", "1")
    monkeypatch.setenv("MVPOSE_NO_DETECTOR", "1")
    monkeypatch.chdir(tmp_path)
    rec = tmp_path / "configurations" / "1" / "recordings" / "cli"
    rec.mkdir(parents=True)
    rng = np.random.default_rng(3)
    paths = []
    for v in range(3):
        np.save(rec / f"camera{v}.npy", rng.integers(0, 256, (3, 360, 640, 3), dtype=np.uint8))
        paths.append(str(rec / f"camera{v}.npy"))
    log = cli.record_and_estimate_pose_main(["--camera_names", *names, "--configuration_number", "1",
                                             "--recording_paths", *paths, "--triangulation", "peaks",
                                             "--max_peaks", "3", "--peak_threshold", "0.02", "--peak_min_rel", "0.2",
                                             "--inlier_px", "25"])
    with open(rec / "recording_log.yaml") as f:
        saved = yaml.safe_load(f)
    assert (saved["triangulation"], saved["max_peaks"], saved["peak_threshold"], saved["peak_min_rel"]) == \
        ("peaks", 3, 0.02, 0.2)
    pk, k2 = np.load(log["kpts_2d_peaks"]), np.load(log["kpts_2d"])
    assert pk.shape == (2, 17, 3, 3, 3) and pk.dtype == np.float32 and k2.shape == (2, 17, 3, 3)
    cp = {i: geometry.get_params_from_name(n, extrinsic_params_dir=str(ext))[1] for i, n in enumerate(names)}
    xyz, inl, sel, err, kp = ops.triangulate_peaks(torch.tensor(pk, device="cuda"),
                                                   torch.tensor(ops.pack_cameras(cp), device="cuda"), [0, 1, 2],
                                                   inlier_px=25.0)
    _bits_equal(np.load(log["kpts_3d"]), xyz.cpu().numpy())
    assert np.array_equal(np.load(log["kpts_3d_peak_sel"]), sel.cpu().numpy())
    assert np.array_equal(np.load(log["kpts_2d_selected"]), kp.cpu().numpy(), equal_nan=True)
    again = pe.estimate_pose_from_video(names, paths, None, extrinsic_params_dir=str(ext), recompute_kpts_2d=False,
                                        triangulation="peaks", inlier_px=25.0)
    _bits_equal(again[2], xyz.cpu().numpy())
    (rec / "kpts_2d_peaks.npy").unlink()
    with pytest.raises(FileNotFoundError, match="kpts_2d_peaks.npy"):
        pe.estimate_pose_from_video(names, paths, None, extrinsic_params_dir=str(ext), recompute_kpts_2d=False,
                                    triangulation="peaks")


def test_get_pose_2D_returns_the_peaks_when_asked(ops):
    """get_pose_2D(max_peaks=) on the V frames of one time step: a third result, the estimator's
    peaks of that run, whose first slot is the (17, 3, V) keypoints; without it, two results."""
    from mvpose import pose_estimation as pe
    from mvpose.estimator import BatchPoseEstimator
    est = BatchPoseEstimator(seed=0, max_frames=3)
    frames = syn.make_frames(3, seed=53)
    k2, heat, pk = pe.get_pose_2D(list(frames), est, max_peaks=3, peak_thr=-1e9, peak_min_rel=0.2)
    r = est.run(torch.tensor(frames, device="cuda"), n_views=3, max_peaks=3, peak_thr=-1e9, peak_min_rel=0.2)
    assert pk.shape == (17, 3, 3, 3) and pk.dtype == np.float32 and len(heat) == 3
    assert np.array_equal(pk, r["peaks"][0].cpu().numpy(), equal_nan=True)
    assert np.array_equal(pk[:, 0], k2)
    two = pe.get_pose_2D(list(frames), est)
    assert len(two) == 2 and np.array_equal(two[0], k2)
    with pytest.raises(ValueError, match="max_peaks"):          # a per-frame callable has no heatmaps to offer
        pe.get_pose_2D(list(frames), lambda f: None, max_peaks=2)


def test_peaks_take_the_frame_offsets(ops, tmp_path, monkeypatch):
    """estimate_pose_from_video(triangulation="peaks", sync="pose") on unsynchronised keypoints and
    their peak lists (the argmax first, a decoy second): the peaks are cut to the common instants
    with the keypoints, and the points are ops.triangulate_peaks of the aligned peaks."""
    import sync_ref
    from mvpose import geometry, pose_estimation as pe, sync
    from test_frame_sync_gpu import TRUE
    cams, k = sync_ref.shifted_case(120, TRUE, seed=3)
    rng = np.random.default_rng(5)
    peaks = np.stack([k, k], 2)                                               # (T, 17, 2, 3, V)
    r, th = rng.uniform(80.0, 300.0, k[:, :, 0].shape), rng.uniform(0.0, 2 * np.pi, k[:, :, 0].shape)
    peaks[:, :, 1, 0] += (r * np.cos(th)).astype(np.float32)
    peaks[:, :, 1, 1] += (r * np.sin(th)).astype(np.float32)
    peaks[:, :, 1, 2] *= np.float32(0.5)
    ext = tmp_path / "configurations" / "1" / "extrinsic_camera_parameters"
    names = ["camA", "camB", "camC", "camD"]
    for name, c in zip(names, cams):
        geometry.write_camera_parameters(name, c["K"], c["dist"], str(tmp_path / "intrinsic_camera_parameters"))
        geometry.write_rotation_translation(name, c["R"], c["T"], str(ext))
    geometry.save_camera_names(str(ext), dict(enumerate(names)), "camA")
    rec = tmp_path / "configurations" / "1" / "recordings" / "0"
    rec.mkdir(parents=True)
    np.save(rec / "kpts_2d.npy", k)
    np.save(rec / "kpts_2d_peaks.npy", peaks)
    monkeypatch.chdir(tmp_path)
    paths = [str(rec / f"camera{v}.npy") for v in range(4)]
    k1, _, x1, info = pe.estimate_pose_from_video(names, paths, None, extrinsic_params_dir=str(ext),
                                                  recompute_kpts_2d=False, triangulation="peaks", sync="pose",
                                                  max_lag=8, return_info=True)
    assert info["frame_offsets"].tolist() == list(TRUE)
    (want_k, want_p), _ = sync.apply_frame_offsets([k, peaks], np.array(TRUE), (3, 4))
    assert len(want_p) < len(peaks) and np.array_equal(k1, want_k) and np.array_equal(info["peaks"], want_p)
    cp = {i: geometry.get_params_from_name(n, extrinsic_params_dir=str(ext))[1] for i, n in enumerate(names)}
    xyz, inl, sel, _, kp = ops.triangulate_peaks(torch.tensor(want_p, device="cuda"),
                                                 torch.tensor(ops.pack_cameras(cp), device="cuda"), [0, 1, 2, 3])
    _bits_equal(x1, xyz.cpu().numpy())
    assert np.array_equal(info["sel"], sel.cpu().numpy()) and np.array_equal(info["kpts_selected"], kp.cpu().numpy())
    assert np.array_equal(np.load(rec / "kpts_2d_peaks.npy"), peaks)          # a loaded file is not written back
