"""CPU: pose-based frame synchronisation — the numpy restatement (tests/sync_ref.py) recovers known
offsets, mvpose.sync's pair / global logic agrees with it, apply_frame_offsets is exact indexing,
and the fronts' argument handling."""
import numpy as np
import pytest

import sync_ref as ref

TRUE = (0, 3, -5, 2)
L = 8
T = 240
J = 17


@pytest.fixture(scope="module")
def curves():
    """seed -> (cams, kpts, sum, cnt, pairs) of the (0, 3, -5, 2) case at L = 8, computed once."""
    out = {}
    for seed in range(4):
        cams, k = ref.shifted_case(T, TRUE, seed=seed)
        out[seed] = (cams, k) + ref.lag_cost(k, cams, [0, 1, 2, 3], L)
    return out


@pytest.mark.parametrize("seed", range(4))
def test_restatement_recovers_integer_offsets(curves, seed):
    """True offsets (0, 3, -5, 2), make_poses(jitter=0), 1 px noise: recovered exactly; pair (1, 2)
    has a true lag of 8, the edge of the scan, and is rejected for that; the other five pairs
    still fix every offset."""
    from mvpose import sync
    _, _, s, n, pairs = curves[seed]
    r = ref.solve_offsets(s, n, pairs, 4, T * J)
    assert pairs[3] == (1, 2)
    assert r["reason"] == ["", "", "", "edge", "", ""]
    assert r["lag"] == [-3, 5, -2, 8, 1, -7]
    assert np.array_equal(r["offsets"], TRUE)
    # the package's own logic on the same curves
    off, info = sync.offsets_from_curves(s, n, pairs, 4, T * J)
    assert off.dtype == np.int64 and np.array_equal(off, TRUE)
    assert info["reason"] == r["reason"] and info["lag"].tolist() == r["lag"]
    assert info["accepted"].tolist() == r["accepted"]
    np.testing.assert_allclose(info["s"], r["s"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(info["lag_subframe"], r["sub"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(info["contrast"], r["contrast"], rtol=1e-12)
    acc = info["accepted"]
    assert np.isnan(info["residual"][~acc]).all() and (np.abs(info["residual"][acc]) < 0.1).all()


def test_short_recording():
    """T = 40, the prototype's other length."""
    cams, k = ref.shifted_case(40, TRUE, seed=1)
    s, n, pairs = ref.lag_cost(k, cams, [0, 1, 2, 3], L)
    r = ref.solve_offsets(s, n, pairs, 4, 40 * J)
    assert np.array_equal(r["offsets"], TRUE) and r["reason"][3] == "edge"


def test_subframe_estimate_is_sane():
    """Truth built by linear interpolation between poses, offsets (0, 3.4, -4.3, 2.25), seeds 0-7:
    the parabola's sub-frame lag is within 0.5 frame of the truth on every non-edge pair.  This is
    a sanity bound on an informational output, not an accuracy claim: the vertex of a parabola
    through three samples of a truncated-quadratic cost is biased towards the integer lag."""
    truth = np.array(TRUE) + np.array([0, 0.4, 0.7, 0.25])
    worst = 0.0
    for seed in range(8):
        cams, k = ref.shifted_case(T, truth, seed=seed)
        s, n, pairs = ref.lag_cost(k, cams, [0, 1, 2, 3], L)
        from mvpose import sync
        _, info = sync.offsets_from_curves(s, n, pairs, 4, T * J)
        for p, (a, b) in enumerate(pairs):
            if info["reason"][p] != "edge":
                worst = max(worst, abs(info["lag_subframe"][p] - (truth[a] - truth[b])))
    print("worst |sub-frame lag - truth|:", worst)
    assert worst < 0.5


def test_unconnected_camera_gets_no_offset(curves):
    """Only pairs (0, 1) and (2, 3) accepted: cameras 2 and 3 hang together but not on camera 0."""
    from mvpose import sync
    _, _, s, n, pairs = curves[0]
    s = s.copy()
    for p in (1, 2, 3, 4):       # flatten the curves of (0,2), (0,3), (1,2), (1,3): no contrast
        s[p] = n[p] * 5.0
    off, info = sync.offsets_from_curves(s, n, pairs, 4, T * J)
    assert info["reason"] == ["", "contrast", "contrast", "contrast", "contrast", ""]
    assert off.tolist() == [0, 3, sync.NO_OFFSET, sync.NO_OFFSET]
    assert np.isnan(info["s"][2:]).all()
    r = ref.solve_offsets(s, n, pairs, 4, T * J)
    assert np.isnan(r["offsets"][2:]).all() and r["offsets"][1] == 3
    # too little overlap everywhere
    off, info = sync.offsets_from_curves(s, n, pairs, 4, 4 * T * J)
    assert info["reason"] == ["overlap"] * 6 and (off[1:] == sync.NO_OFFSET).all()
    with pytest.raises(ValueError):
        sync.apply_frame_offsets([np.zeros((10, 4))], off, (1,))


def test_apply_frame_offsets_slices():
    from mvpose import sync
    rng = np.random.default_rng(0)
    k = rng.normal(size=(30, J, 3, 4)).astype(np.float32)
    h = rng.normal(size=(30, 4, J, 6))
    off = np.array(TRUE)
    (ka, ha, none), first = sync.apply_frame_offsets([k, h, None], off, (3, 1, 0))
    # common instants tau in [3, 30 - 5): camera v contributes frames tau - s_v
    assert first.tolist() == [3, 0, 8, 1] and none is None
    assert ka.shape == (22, J, 3, 4) and ha.shape == (22, 4, J, 6)
    assert ka.dtype == k.dtype and ha.dtype == h.dtype
    for v, f in enumerate(first):
        assert np.array_equal(ka[..., v], k[f:f + 22, ..., v])
        assert np.array_equal(ha[:, v], h[f:f + 22, v])
    (same,), first = sync.apply_frame_offsets([k], np.zeros(4, np.int64), (3,))
    assert np.array_equal(same, k) and first.tolist() == [0, 0, 0, 0]
    with pytest.raises(ValueError):
        sync.apply_frame_offsets([k], np.array([0, 20, -10, 0]), (3,))     # no common frame
    with pytest.raises(ValueError):
        sync.apply_frame_offsets([k], np.array([0, 1, 2]), (3,))           # three offsets, four cameras


def test_apply_undoes_the_shift():
    """Noise-free shifted keypoints, cut by the true offsets: every camera shows the same poses."""
    from mvpose import sync, synthetic as syn
    cams, k = ref.shifted_case(60, TRUE, seed=2, noise_px=0.0)
    (ka,), first = sync.apply_frame_offsets([k], np.array(TRUE), (3,))
    poses = syn.make_poses(60 + 3 + 5 + 1, seed=2, jitter=0.0)   # shifted_case's instants
    # instant tau of the cut = pose index tau - min(s) = tau + 5, tau from max(s) = 3
    for v, cam in enumerate(cams):
        np.testing.assert_allclose(ka[:, :, :2, v], syn.project(poses[8:8 + len(ka)], cam), rtol=0, atol=1e-3)


def test_flags_parse_only_with_extensions():
    from mvpose import cli
    argv = ["--camera_names", "a", "b", "--sync_from_pose", "--max_lag", "12"]
    args = cli.record_and_estimate_pose_parser(extensions=True).parse_args(argv)
    assert args.sync_from_pose is True and args.max_lag == 12
    with pytest.raises(SystemExit):
        cli.record_and_estimate_pose_parser().parse_args(argv)
    args = cli.record_and_estimate_pose_parser(extensions=True).parse_args(["--camera_names", "a"])
    assert args.sync_from_pose is False and args.max_lag is None


def test_front_arguments(tmp_path, monkeypatch):
    from mvpose import cli, pose_estimation
    with pytest.raises(ValueError, match="sync"):
        pose_estimation.estimate_pose_from_video(["a", "b"], ["x", "y"], None, sync="audio")
    monkeypatch.chdir(tmp_path)
    with pytest.raises(NotImplementedError, match="--sync_from_pose"):
        cli.record_and_estimate_pose(["a", "b"], configuration_number=1, recording_paths=["x", "y"],
                                     synchronize_video=True)


def _camera_dicts(camera_params, positions):
    cams = [{"K": np.asarray(K, np.float64), "R": np.asarray(R, np.float64), "T": np.asarray(Tr, np.float64),
             "dist": np.asarray(d, np.float64)} for K, R, Tr, d in camera_params.values()]
    return cams, list(positions)


def test_motionless_subject_is_rejected(tmp_path, monkeypatch):
    """A subject that does not move carries no timing: every pair is rejected for contrast and
    estimate_pose_from_video(sync="pose") raises, naming the cameras.  (The scan is the numpy
    restatement here; tests/test_frame_sync_gpu.py runs the same case through the kernel.)"""
    from mvpose import geometry, pose_estimation, sync
    cams, k = ref.shifted_case(120, TRUE, seed=0, still=True)
    s, n, pairs = ref.lag_cost(k, cams, [0, 1, 2, 3], L)
    off, info = sync.offsets_from_curves(s, n, pairs, 4, 120 * J)
    assert info["reason"] == ["contrast"] * 6 and (info["contrast"] < 1.2).all()
    assert off.tolist() == [0] + [sync.NO_OFFSET] * 3

    def lag_cost(kpts_2d, camera_params, positions, max_lag, min_conf, trunc_px, device=None):
        c, ci = _camera_dicts(camera_params, positions)
        return ref.lag_cost(kpts_2d, c, ci, max_lag, min_conf, trunc_px)
    monkeypatch.setattr(sync, "_lag_cost", lag_cost)
    ext = tmp_path / "configurations" / "1" / "extrinsic_camera_parameters"
    names = ["camA", "camB", "camC", "camD"]
    for name, c in zip(names, cams):
        geometry.write_camera_parameters(name, c["K"], c["dist"], str(tmp_path / "intrinsic_camera_parameters"))
        geometry.write_rotation_translation(name, c["R"], c["T"], str(ext))
    geometry.save_camera_names(str(ext), dict(enumerate(names)), "camA")
    rec = tmp_path / "rec"
    rec.mkdir()
    np.save(rec / "kpts_2d.npy", k)
    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError, match="camB.*camC.*camD"):
        pose_estimation.estimate_pose_from_video(names, [str(rec / f"camera{v}.npy") for v in range(4)], None,
                                                 extrinsic_params_dir=str(ext), recompute_kpts_2d=False,
                                                 sync="pose", max_lag=L)
