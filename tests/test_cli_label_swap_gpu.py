"""GPU: estimate_pose_from_video(fix_swaps=...) and record_and_estimate_pose --fix_label_swaps on a
synthetic recording whose 2D stage is replaced by keypoints with injected left/right exchanges
(tests/label_swap_cases.py), as tests/test_frame_sync_gpu.py drives sync="pose"."""
import numpy as np
import pytest
import torch

import label_swap_cases as cases

pytestmark = pytest.mark.gpu
NAMES = ["camA", "camB", "camC", "camD"]


@pytest.fixture(scope="module")
def project(tmp_path_factory):
    """A project directory with four cameras; the scene's swapped and clean arrays."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mvpose import geometry
    root = tmp_path_factory.mktemp("swap_proj")
    sc = cases.scene(4, 240, 3, "limbs")
    ext = root / "configurations" / "1" / "extrinsic_camera_parameters"
    for name, c in zip(NAMES, sc["cams"]):
        geometry.write_camera_parameters(name, c["K"], c["dist"], str(root / "intrinsic_camera_parameters"))
        geometry.write_rotation_translation(name, c["R"], c["T"], str(ext))
    geometry.save_camera_names(str(ext), dict(enumerate(NAMES)), "camA")
    return root, str(ext), sc


def _stub_2d_stage(monkeypatch, pe, k, hm):
    monkeypatch.setattr(pe, "load_frames", lambda paths, *a, **kw: {i: np.zeros((1, 2, 2, 3), np.uint8) for i in paths})
    monkeypatch.setattr(pe, "build_estimator", lambda *a, **kw: None)
    monkeypatch.setattr(pe, "run_pose_est", lambda *a, **kw: (k.copy(), hm.copy()))


def _recording(root, name):
    rec = root / "configurations" / "1" / "recordings" / name
    rec.mkdir(parents=True)
    return rec, [str(rec / f"camera{v}.npy") for v in range(4)]


@pytest.mark.parametrize("method", ["reference", "robust"])
def test_estimate_pose_from_video_fix_swaps(project, monkeypatch, method):
    from mvpose import pose_estimation as pe
    root, ext, sc = project
    monkeypatch.chdir(root)
    _, paths = _recording(root, f"api_{method}")
    kw = dict(extrinsic_params_dir=ext, triangulation=method, return_info=True)
    _stub_2d_stage(monkeypatch, pe, sc["clean"], sc["gauss_clean"])
    kc, hc, xc, ic = pe.estimate_pose_from_video(NAMES, paths, None, **kw)
    _stub_2d_stage(monkeypatch, pe, sc["kpts"], sc["gauss"])
    k0, h0, x0, i0 = pe.estimate_pose_from_video(NAMES, paths, None, **kw)
    k1, h1, x1, i1 = pe.estimate_pose_from_video(NAMES, paths, None, fix_swaps="limbs", **kw)
    # the labels come back, in the keypoints and in the heatmap Gaussians, and with them the 3D points
    assert i1["label_swaps"].dtype == np.uint8 and np.array_equal(i1["label_swaps"], sc["truth"])
    assert cases.same_bits(k1, sc["clean"]) and cases.same_bits(h1, sc["gauss_clean"])
    assert cases.same_bits(x1, xc) and not cases.same_bits(x0, xc)
    if method == "robust":
        assert np.array_equal(i1["inliers"], ic["inliers"])
    # None is the call without the argument: the swapped labels pass through
    kn, hn, xn, inn = pe.estimate_pose_from_video(NAMES, paths, None, fix_swaps=None, **kw)
    assert cases.same_bits(kn, k0) and cases.same_bits(k0, sc["kpts"]) and cases.same_bits(hn, h0)
    assert cases.same_bits(xn, x0) and "label_swaps" not in inn and "label_swaps" not in i0
    with pytest.raises(ValueError, match="fix_swaps"):
        pe.estimate_pose_from_video(NAMES, paths, None, fix_swaps="face", **kw)


def test_cli_fix_label_swaps(project, monkeypatch):
    import yaml
    from mvpose import cli, pose_estimation as pe
    root, ext, sc = project
    monkeypatch.chdir(root)
    _stub_2d_stage(monkeypatch, pe, sc["clean"], sc["gauss_clean"])
    rec0, paths0 = _recording(root, "cli_clean")
    base = ["--camera_names", *NAMES, "--configuration_number", "1", "--recording_paths"]
    log0 = cli.record_and_estimate_pose_main(base + paths0)
    _stub_2d_stage(monkeypatch, pe, sc["kpts"], sc["gauss"])
    rec1, paths1 = _recording(root, "cli_fixed")
    log1 = cli.record_and_estimate_pose_main(base + paths1 + ["--fix_label_swaps", "limbs"])
    with open(rec1 / "recording_log.yaml") as f:
        saved = yaml.safe_load(f)
    assert saved["fix_label_swaps"] == {"units": "limbs", "exchanged": int(np.unpackbits(sc["truth"]).sum())}
    assert np.array_equal(np.load(log1["label_swaps"]), sc["truth"])
    assert cases.same_bits(np.load(log1["kpts_2d"]), sc["clean"])
    assert cases.same_bits(np.load(log1["heatmaps_2d"]), sc["gauss_clean"])
    assert cases.same_bits(np.load(log1["kpts_3d"]), np.load(log0["kpts_3d"]))
    # without the flag: the usual files and log entries, the swapped labels as the 2D stage gave them
    rec2, paths2 = _recording(root, "cli_plain")
    log2 = cli.record_and_estimate_pose_main(base + paths2)
    assert sorted(log2) == sorted(log0) == ["detector_model", "estimator_model", "heatmaps_2d", "kpts_2d", "kpts_3d",
                                            "recording_paths"]
    assert sorted(p.name for p in rec2.iterdir()) == ["heatmaps_2d.npy", "kpts_2d.npy", "kpts_3d.npy",
                                                      "recording_log.yaml"]
    assert cases.same_bits(np.load(log2["kpts_2d"]), sc["kpts"])
    assert not cases.same_bits(np.load(log2["kpts_3d"]), np.load(log0["kpts_3d"]))
