"""GPU: the epipolar lag-cost scan (mvp_epipolar_lag_cost) against the numpy restatement
tests/sync_ref.py, and the synchronisation fronts on shifted synthetic keypoints.

cnt must be equal exactly.  sum: both sides are fp64 on the same f32 undistorted pixels; a term's
relative error is about eps · (coordinate scale / d) ≈ 1e-13 at d ≈ 1 px (the cancellation in
x_bᵀ F x_a), summation order adds about N · eps, so rtol 1e-9 leaves three orders of margin
without hiding a wrong term.  The measured maximum is printed (1.3e-13 over the shapes below, at
T = 2, J = 1, where one small term is the whole sum)."""
import numpy as np
import pytest
import torch

import sync_ref as ref
from mvpose import synthetic as syn

pytestmark = pytest.mark.gpu
RTOL = 1e-9
TRUE = (0, 3, -5, 2)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mvpose import ops as _ops
    return _ops


def _random_case(T, J, n_cams, seed, invalid=0.0):
    """Moving synthetic subject, 1 px noise, the first J joints; `invalid`: that share of the
    keypoints gets a NaN coordinate or a confidence of 0.05."""
    cams = syn.make_rig(n_cams, seed=seed)
    k = syn.make_kpts_2d(syn.make_poses(T, seed=seed, jitter=0.0), cams, seed=seed + 1)[:, :J].copy()
    if invalid:
        rng = np.random.default_rng(seed + 2)
        r = rng.uniform(size=(T, J, n_cams))
        k[:, :, 0, :][r < invalid / 2] = np.nan
        k[:, :, 2, :][(r >= invalid / 2) & (r < invalid)] = 0.05
    return cams, k


def _device(ops, cams, k, ci, L, min_conf=0.0, trunc_px=20.0):
    cams_d = torch.tensor(ops.pack_cameras(syn.reference_camera_params(cams)), device="cuda")
    s, n, pairs = ops.epipolar_lag_cost(torch.tensor(k, device="cuda"), cams_d, ci, L, min_conf=min_conf,
                                        trunc_px=trunc_px)
    assert s.dtype == torch.float64 and n.dtype == torch.int64
    return s.cpu().numpy(), n.cpu().numpy(), pairs


def _compare(ops, cams, k, ci, L, min_conf=0.0, trunc_px=20.0):
    ds, dn, dp = _device(ops, cams, k, ci, L, min_conf, trunc_px)
    rs, rn, rp = ref.lag_cost(k, cams, list(ci), L, min_conf, trunc_px)
    assert dp == rp and ds.shape == rs.shape == (len(rp), 2 * L + 1)
    assert np.array_equal(dn, rn)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(rs != 0, np.abs(ds - rs) / np.abs(rs), np.abs(ds))
    print(f"T={k.shape[0]} J={k.shape[1]} nv={len(ci)} L={L}: max rel |sum - ref| = {rel.max():.3g}")
    np.testing.assert_allclose(ds, rs, rtol=RTOL, atol=0)
    return ds, dn


def _tile(ops, J):
    return ops.epipolar_lag_cost_plan(100000, J, 2, 0)[0]


def _shape_cases():
    # (T as a function of the tile B, L or "T-1", J, cam_idx, cameras in the rig)
    return [
        (lambda B: 1, 0, 17, (0, 1), 2),
        (lambda B: 2, 1, 1, (0, 1), 2),
        (lambda B: 2, 0, 17, (2, 0, 3), 4),
        (lambda B: B - 1, 8, 17, (0, 1, 2), 3),
        (lambda B: B - 1, "T-1", 1, (0, 1), 2),
        (lambda B: B, 1, 17, (2, 0, 3), 4),
        (lambda B: B, "T-1", 17, (0, 1), 2),
        (lambda B: B + 1, 8, 17, tuple(range(8)), 8),
        (lambda B: B + 1, 0, 1, (0, 1, 2), 3),
        (lambda B: 2 * B + 1, 1, 17, (0, 1), 2),
        (lambda B: 2 * B + 1, 8, 1, (2, 0, 3), 4),
        (lambda B: 2 * B + 1, "T-1", 17, (0, 1, 2), 3),
        (lambda B: 2 * B + 1, "T-1", 1, (1, 0), 2),
    ]


@pytest.mark.parametrize("case", range(len(_shape_cases())))
def test_kernel_matches_restatement(ops, case):
    """T in {1, 2, B-1, B, B+1, 2B+1}, L in {0, 1, 8, T-1} (halo shorter than, equal to and longer
    than the tile; more lags than one chunk holds), J in {1, 17}, 2 / 3 / 8 views, cam_idx out of
    order and skipping a column."""
    fT, L, J, ci, n_cams = _shape_cases()[case]
    T = fT(_tile(ops, J))
    L = T - 1 if L == "T-1" else L
    cams, k = _random_case(T, J, n_cams, seed=10 + case)
    ds, dn = _compare(ops, cams, k, ci, L)
    assert dn[:, L].min() == T * J                 # lag 0 sees every keypoint
    assert (dn[:, 0] == (T - L) * J).all()         # the overlap shrinks with the lag


def test_tile_is_what_the_plan_reports(ops):
    B = _tile(ops, 17)
    assert B >= 8
    assert ops.epipolar_lag_cost_plan(5, 17, 2, 0)[0] == 5          # a tile never exceeds the recording
    assert ops.epipolar_lag_cost_plan(100000, 17, 4, 60)[1] > 4 * 100000 * 17 * 8


def test_invalid_keypoints(ops):
    """20 % of the keypoints NaN or below min_conf; view 1 entirely invalid: its pairs give
    cnt = 0 and sum = 0."""
    cams, k = _random_case(150, 17, 4, seed=40, invalid=0.2)
    k[:, :, 2, 1] = np.nan
    k[::2, :, 1, 1] = np.inf
    ds, dn = _compare(ops, cams, k, (0, 1, 2, 3), 8, min_conf=0.1)
    dead = [0, 3, 4]                                # pairs (0,1), (1,2), (1,3)
    assert (dn[dead] == 0).all() and (ds[dead] == 0).all()
    live = [1, 2, 5]
    assert (dn[live] > 0).all() and (dn[live, 8] < 150 * 17 * 0.75).all()


def test_truncation(ops):
    """tau = 0.5 px against 1 px noise and 3-frame offsets: most terms sit at tau²."""
    cams, k = ref.shifted_case(100, TRUE, seed=5)
    ds, dn = _compare(ops, cams, k, (0, 1, 2, 3), 8, trunc_px=0.5)
    assert (ds <= dn * 0.25).all() and (ds > dn * 0.25 * 0.5).all()


def test_deterministic_on_a_side_stream(ops):
    cams, k = _random_case(300, 17, 4, seed=50, invalid=0.1)
    cams_d = torch.tensor(ops.pack_cameras(syn.reference_camera_params(cams)), device="cuda")
    kd = torch.tensor(k, device="cuda")
    a = ops.epipolar_lag_cost(kd, cams_d, (0, 1, 2, 3), 20)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        b = ops.epipolar_lag_cost(kd, cams_d, (0, 1, 2, 3), 20)
    st.synchronize()
    assert torch.equal(a[0].view(torch.int64), b[0].view(torch.int64)) and torch.equal(a[1], b[1])


def test_argument_errors(ops):
    from mvpose import _lib
    cams, k = _random_case(10, 17, 2, seed=60)
    cams_d = torch.tensor(ops.pack_cameras(syn.reference_camera_params(cams)), device="cuda")
    kd = torch.tensor(k, device="cuda")
    for kw, what in ((dict(cam_idx=(0, 1), max_lag=10), "max_lag"), (dict(cam_idx=(0,), max_lag=2), "n_cam_idx"),
                     (dict(cam_idx=(0, 1), max_lag=2, trunc_px=0.0), "trunc_px"),
                     (dict(cam_idx=(0, 1), max_lag=2, trunc_px=-1.0), "trunc_px"),
                     (dict(cam_idx=(0, 1), max_lag=-1), "max_lag"), (dict(cam_idx=(0, 2), max_lag=2), "cam_idx")):
        with pytest.raises(_lib.MvposeError, match=what):
            ops.epipolar_lag_cost(kd, cams_d, **kw)
    with pytest.raises(ValueError):
        ops.epipolar_lag_cost(kd[0], cams_d, (0, 1), 2)
    with pytest.raises(TypeError):
        ops.epipolar_lag_cost(kd.double(), cams_d, (0, 1), 2)
    # a short workspace is refused before any launch
    out = torch.zeros((1, 5), dtype=torch.float64, device="cuda")
    cnt = torch.zeros((1, 5), dtype=torch.int64, device="cuda")
    work = torch.empty(64, dtype=torch.uint8, device="cuda")
    ci = (_lib.c_int * 2)(0, 1)
    rc = _lib.lib.mvp_epipolar_lag_cost(kd.data_ptr(), 10, 17, 2, cams_d.data_ptr(), 2, ci, 2, 2, 0.0, 20.0,
                                        work.data_ptr(), 64, out.data_ptr(), cnt.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == -1 and "workspace_bytes" in _lib.last_error() and (out == 0).all()


# ------------------------------------------------------------------ fronts
def test_estimate_frame_offsets(ops):
    from mvpose import sync
    cams, k = ref.shifted_case(240, TRUE, seed=0)
    cp = syn.reference_camera_params(cams)
    off, info = sync.estimate_frame_offsets(k, cp, max_lag=8)
    assert off.dtype == np.int64 and off.tolist() == list(TRUE)
    assert info["pairs"][3] == (1, 2) and info["reason"] == ["", "", "", "edge", "", ""]
    rs, rn, _ = ref.lag_cost(k, cams, [0, 1, 2, 3], 8)
    assert np.array_equal(info["cost_cnt"], rn)
    np.testing.assert_allclose(info["cost_sum"], rs, rtol=RTOL)
    r = ref.solve_offsets(rs, rn, info["pairs"], 4, 240 * 17)
    np.testing.assert_allclose(info["s"], r["s"], rtol=0, atol=1e-6)
    # a subset of the cameras, listed by key: view 0 is camera 2
    off, info = sync.estimate_frame_offsets(k, cp, camera_indices=[2, 0, 3], max_lag=8)
    assert off.tolist() == [0, 5, 7]
    # a motionless subject carries no timing
    cams, k = ref.shifted_case(120, TRUE, seed=0, still=True)
    off, info = sync.estimate_frame_offsets(k, syn.reference_camera_params(cams), max_lag=8)
    assert info["reason"] == ["contrast"] * 6 and off.tolist() == [0] + [sync.NO_OFFSET] * 3


@pytest.fixture(scope="module")
def shifted_project(tmp_path_factory):
    """A project directory with four cameras and a kpts_2d.npy of unsynchronised keypoints."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mvpose import geometry
    root = tmp_path_factory.mktemp("sync_proj")
    cams, k = ref.shifted_case(120, TRUE, seed=3)
    ext = root / "configurations" / "1" / "extrinsic_camera_parameters"
    names = ["camA", "camB", "camC", "camD"]
    for name, c in zip(names, cams):
        geometry.write_camera_parameters(name, c["K"], c["dist"], str(root / "intrinsic_camera_parameters"))
        geometry.write_rotation_translation(name, c["R"], c["T"], str(ext))
    geometry.save_camera_names(str(ext), dict(enumerate(names)), "camA")
    rec = root / "configurations" / "1" / "recordings" / "0"
    rec.mkdir(parents=True)
    np.save(rec / "kpts_2d.npy", k)
    return root, names, str(ext), rec, k


def test_estimate_pose_from_video_sync(ops, shifted_project, monkeypatch):
    from mvpose import pose_estimation as pe, sync
    root, names, ext, rec, k = shifted_project
    monkeypatch.chdir(root)
    paths = [str(rec / f"camera{v}.npy") for v in range(4)]
    kw = dict(extrinsic_params_dir=ext, recompute_kpts_2d=False, triangulation="robust", return_info=True)
    k0, h0, x0, i0 = pe.estimate_pose_from_video(names, paths, None, **kw)
    k1, h1, x1, i1 = pe.estimate_pose_from_video(names, paths, None, sync="pose", max_lag=8, **kw)
    assert i1["frame_offsets"].tolist() == list(TRUE) and i1["frame_first"].tolist() == [3, 0, 8, 1]
    assert i1["sync_pairs"]["reason"][3] == "edge"
    (want,), _ = sync.apply_frame_offsets([k0], np.array(TRUE), (3,))
    assert np.array_equal(k0, k) and np.array_equal(k1, want) and h1 is None
    assert x1.shape == (len(want), 17, 3)
    e0, e1 = i0["reproj_err"], i1["reproj_err"]
    m0, m1 = float(np.mean(e0[np.isfinite(e0)])), float(np.mean(e1[np.isfinite(e1)]))
    print(f"mean reproj_err: unsynchronised {m0:.3f} px, synchronised {m1:.3f} px")
    assert m1 < m0 and i1["inliers"].mean() > i0["inliers"].mean()
    # sync=None is the call without the argument
    kn, hn, xn, inn = pe.estimate_pose_from_video(names, paths, None, sync=None, **kw)
    assert np.array_equal(kn, k0) and np.array_equal(xn.view(np.uint32), x0.view(np.uint32))
    assert np.array_equal(inn["inliers"], i0["inliers"]) and "frame_offsets" not in inn
    np.testing.assert_array_equal(inn["reproj_err"], e0)
    # the default method too
    d0 = pe.estimate_pose_from_video(names, paths, None, extrinsic_params_dir=ext, recompute_kpts_2d=False)
    d1 = pe.estimate_pose_from_video(names, paths, None, extrinsic_params_dir=ext, recompute_kpts_2d=False, sync=None)
    assert len(d0) == len(d1) == 3 and np.array_equal(d0[2].view(np.uint32), d1[2].view(np.uint32))


def test_cli_sync_from_pose(ops, shifted_project, monkeypatch):
    """record_and_estimate_pose --sync_from_pose with the 2D stage replaced by the shifted
    synthetic keypoints: frame_offsets.npy, the aligned arrays and the log entries are written;
    without the flag the log and the files are the usual ones."""
    import yaml
    from mvpose import cli, pose_estimation as pe, sync
    root, names, ext, _, k = shifted_project
    monkeypatch.chdir(root)
    hm = np.random.default_rng(0).normal(size=(len(k), 4, 17, 6))
    monkeypatch.setattr(pe, "load_frames", lambda paths, *a, **kw: {i: np.zeros((1, 2, 2, 3), np.uint8) for i in paths})
    monkeypatch.setattr(pe, "build_estimator", lambda *a, **kw: None)
    monkeypatch.setattr(pe, "run_pose_est", lambda *a, **kw: (k.copy(), hm.copy()))
    rec =root / "configurations" / "1" / "recordings" / "cli_sync"
    rec.mkdir(parents=True)
    paths = [str(rec / f"camera{v}.npy") for v in range(4)]
    base = ["--camera_names", *names, "--configuration_number", "1", "--recording_paths", *paths]
    log = cli.record_and_estimate_pose_main(base + ["--sync_from_pose", "--max_lag", "8"])
    with open(rec / "recording_log.yaml") as f:
        saved = yaml.safe_load(f)
    assert saved["sync"] == {"method": "pose", "max_lag": 8, "offsets": list(TRUE),
                             "rejected_pairs": [["camB", "camC", "edge"]]}
    off = np.load(log["frame_offsets"])
    assert off.dtype == np.int64 and off.tolist() == list(TRUE)
    (ka, ha), _ = sync.apply_frame_offsets([k, hm], off, (3, 1))
    assert np.array_equal(np.load(log["kpts_2d"]), ka) and np.array_equal(np.load(log["heatmaps_2d"]), ha)
    assert np.load(log["kpts_3d"]).shape == (len(ka), 17, 3)
    # without the flag: no sync entries, no frame_offsets.npy, the unaligned arrays
    rec2 = root / "configurations" / "1" / "recordings" / "cli_plain"
    rec2.mkdir(parents=True)
    paths2 = [str(rec2 / f"camera{v}.npy") for v in range(4)]
    log2 = cli.record_and_estimate_pose_main(["--camera_names", *names, "--configuration_number", "1",
                                              "--recording_paths", *paths2])
    assert sorted(log2) == ["detector_model", "estimator_model", "heatmaps_2d", "kpts_2d", "kpts_3d",
                            "recording_paths"]
    assert sorted(p.name for p in rec2.iterdir()) == ["heatmaps_2d.npy", "kpts_2d.npy", "kpts_3d.npy",
                                                      "recording_log.yaml"]
    assert np.array_equal(np.load(log2["kpts_2d"]), k)
    # keypoints that carry no timing: the command line raises
    _, still = ref.shifted_case(len(k), TRUE, seed=3, still=True)
    monkeypatch.setattr(pe, "run_pose_est", lambda *a, **kw: (still.copy(), hm.copy()))
    with pytest.raises(ValueError, match="camB"):
        cli.record_and_estimate_pose_main(base + ["--sync_from_pose", "--max_lag", "8"])
