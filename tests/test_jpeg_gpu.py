"""GPU: the split JPEG decode — host entropy decoding (mvp_jpeg_parse_many) + device
reconstruction (mvp_jpeg_reconstruct, csrc/jpeg_recon.hip) — returns, on the device, exactly the
BGR frames the host readers return today (libjpeg through PIL): the matrix of
tests/test_jpeg_parse.py, slices, mixed sampling, full-size grids, the AVI and frame<N>.jpg
containers with the memory guard and the host switch, per-frame fallback, and the drop-in
command line fed MJPEG recordings."""
import numpy as np
import pytest
import torch

import jpeg_ref as J
from test_cli_gpu import project  # noqa: F401  (the synthetic project directory fixture)

pytestmark = pytest.mark.gpu

CASES = J.matrix()


@pytest.fixture(scope="module")
def video():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mvpose import video as v
    return v


def host(datas):
    return np.stack([J.pil_bgr(d) for d in datas])


@pytest.mark.parametrize("size", J.SIZES, ids=[f"{w}x{h}" for w, h in J.SIZES])
def test_matrix_equals_pil(video, size):
    """Every case of the CPU matrix with this frame size (all samplings, qualities, Huffman table
    kinds and restart settings) in one call: frames of mixed sampling share the launches."""
    datas = [J.case_bytes(c) for c in CASES if c[1] == size]
    assert len(datas) == 16
    t = {}
    got = video.decode_jpeg_device(datas, threads=4, timings=t)
    assert got.is_cuda and got.dtype == torch.uint8 and got.shape == (16, size[1], size[0], 3)
    assert t["fallback"] == 0 and t["frames"] == 16
    ref = host(datas)
    out = got.cpu().numpy()
    for k, c in enumerate(c for c in CASES if c[1] == size):
        np.testing.assert_array_equal(out[k], ref[k], err_msg=c[0])


@pytest.mark.parametrize("width", [2, 4, 5, 6])
def test_narrow_frames(video, width):
    """Both sides of libjpeg's switch from replicated to triangle-filtered chroma (a chroma plane
    more than 2 samples wide)."""
    datas = [J.encode(J.image(width, 5, "noise", seed=s), subsampling=sub, quality=95)
             for s, sub in enumerate((1, 2, 0, 2))]
    np.testing.assert_array_equal(video.decode_jpeg_device(datas).cpu().numpy(), host(datas))


def test_slices_of_a_frame_list(video):
    datas = [J.encode(J.image(70, 45, ("ramp", "noise")[k % 2], seed=k), subsampling=k % 3, quality=75)
             for k in range(12)]
    ref = host(datas)
    for sl in [(0, None), (0, -1), (3, 7), (5, 6)]:
        got = video.decode_jpeg_device(datas[slice(*sl)], size=(45, 70))
        np.testing.assert_array_equal(got.cpu().numpy(), ref[slice(*sl)], err_msg=f"slice {sl}")


def test_mixed_subsampling(video):
    datas = [J.encode(J.image(70, 45, "noise", seed=k), subsampling=(2, 0)[k % 2], quality=90) for k in range(4)]
    np.testing.assert_array_equal(video.decode_jpeg_device(datas).cpu().numpy(), host(datas))


def test_more_frames_than_one_launch(video):
    """The launches take JPEG_LAUNCH_FRAMES frames each and share their scratch planes."""
    n = video.JPEG_LAUNCH_FRAMES + 3
    datas = [J.encode(J.image(17, 9, "noise", seed=k), subsampling=k % 3, quality=90) for k in range(n)]
    np.testing.assert_array_equal(video.decode_jpeg_device(datas).cpu().numpy(), host(datas))


def skeleton_rgb(n, seed, h, w):
    from mvpose import synthetic as syn
    return syn.make_skeleton_frames(n, seed=seed, h=h, w=w)[0]


@pytest.mark.parametrize("w,h,sub,n", [(1280, 720, 2, 2), (1920, 1080, 1, 1)])
def test_full_size_frames(video, w, h, sub, n):
    """The real grid sizes; 1080 is no multiple of 16, so the last MCU row is cropped."""
    datas = [J.encode(fr, subsampling=sub, quality=90) for fr in skeleton_rgb(n, 5, h, w)]
    np.testing.assert_array_equal(video.decode_jpeg_device(datas).cpu().numpy(), host(datas))


def test_full_size_420_with_an_odd_height(video):
    """h2v2 at a full-size width with an odd number of chroma rows: the bottom row has no row below."""
    data = J.encode(skeleton_rgb(1, 6, 1080, 1280)[0][:1077], subsampling=2, quality=90)
    np.testing.assert_array_equal(video.decode_jpeg_device([data]).cpu().numpy(), host([data]))


@pytest.fixture(scope="module")
def recording(tmp_path_factory, video):
    """12 frames as a Motion-JPEG AVI and as a frame<N>.jpg directory, + the host readers' frames."""
    root = tmp_path_factory.mktemp("jpegrec")
    frames = np.stack([J.image(70, 45, ("ramp", "noise")[k % 2], seed=k) for k in range(12)])
    avi = root / "cam0.avi"
    video.write_avi(avi, frames, codec="mjpeg", quality=85)
    d = root / "cam1"
    d.mkdir()
    from PIL import Image
    for k, fr in enumerate(frames):
        Image.fromarray(fr).save(d / f"frame{k}.jpg", quality=80, subsampling=(2, 1, 0)[k % 3])
    return {str(avi): video.read_avi(avi), str(d): video.read_image_dir(d)}


def test_containers_on_the_device(video, recording, monkeypatch):
    from mvpose import pose_estimation as pe
    for p, ref in recording.items():
        assert isinstance(ref, np.ndarray) and ref.shape == (12, 45, 70, 3)
        got = video.read_recording(p, 0, -1, device="cuda")
        assert isinstance(got, torch.Tensor) and got.is_cuda
        np.testing.assert_array_equal(got.cpu().numpy(), ref[:-1], err_msg=p)
        got = video.read_recording(p, 3, 7, device=torch.device("cuda", 0))
        np.testing.assert_array_equal(got.cpu().numpy(), ref[3:7], err_msg=p)
        small = video.read_recording(p, 0, -1, device="cuda", max_device_bytes=1)     # the memory guard
        assert isinstance(small, np.ndarray)
        np.testing.assert_array_equal(small, ref[:-1], err_msg=p)
        exact = video.read_recording(p, 0, -1, device="cuda", max_device_bytes=11 * 45 * 70 * 3)
        assert isinstance(exact, torch.Tensor)
    paths = list(recording)
    dev = pe.load_frames(paths, (0, -1), device=pe.video_device())
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in dev.values())
    monkeypatch.setenv("MVPOSE_VIDEO_DECODE", "host")
    assert pe.video_device() is None
    hst = pe.load_frames(paths, (0, -1), device=pe.video_device())
    for k, p in enumerate(paths):
        assert isinstance(hst[k], np.ndarray)
        np.testing.assert_array_equal(hst[k], recording[p][:-1])
        np.testing.assert_array_equal(dev[k].cpu().numpy(), hst[k])


def test_unsupported_frames_fall_back_one_by_one(video):
    rgb = [J.image(70, 45, "noise", seed=k) for k in range(5)]
    datas = [J.encode(fr, subsampling=2, quality=90) for fr in rgb]
    datas[2] = J.encode(rgb[2], subsampling=2, quality=90, progressive=True)
    t = {}
    got = video.decode_jpeg_device(datas, timings=t)
    np.testing.assert_array_equal(got.cpu().numpy(), host(datas))
    assert t["fallback"] == 1 and t["frames"] == 5
    assert all(t[k] >= 0 for k in ("parse", "pack", "launch"))
    # a frame whose range condition only the scan shows (found by the parse, not the probe)
    from test_jpeg_parse import dqt_out_of_range
    odd = [J.encode(J.image(16, 16, "ramp"), subsampling=0, quality=90), dqt_out_of_range()]
    got = video.decode_jpeg_device(odd, timings=t)
    np.testing.assert_array_equal(got.cpu().numpy(), host(odd))
    assert t["fallback"] == 1


def test_broken_and_wrong_size_frames_raise_as_the_host_reader_does(video, tmp_path):
    frames = np.stack([J.image(70, 45, "noise", seed=k) for k in range(3)])
    good = [J.encode(fr, subsampling=2, quality=90) for fr in frames]
    with pytest.raises(ValueError, match="stream header says"):
        video.decode_jpeg_device(good + [J.encode(J.image(64, 45, "ramp"))])
    with pytest.raises(ValueError, match="stream header says"):           # ... and when PIL decodes it
        video.decode_jpeg_device(good + [J.encode(J.image(64, 45, "ramp"), progressive=True)])
    cut = good[1][:len(good[1]) // 2]
    with pytest.raises(OSError) as dev_err:
        video.decode_jpeg_device([good[0], cut, good[2]])
    with pytest.raises(OSError) as host_err:
        video._decode_jpeg(cut)
    assert type(dev_err.value) is type(host_err.value) and str(dev_err.value) == str(host_err.value)
    # through the AVI reader: a frame of another size than the stream header's
    avi = tmp_path / "bad.avi"
    video.write_avi(avi, frames, codec="mjpeg")
    raw = avi.read_bytes()
    info = video.parse_avi(raw)
    d, n = info.chunks[1]
    small = J.encode(J.image(62, 45, "ramp"), quality=20)
    assert len(small) <= n
    patched = raw[:d] + small + b"\0" * (n - len(small)) + raw[d + n:]
    avi.write_bytes(patched)
    with pytest.raises(ValueError, match="frame 1 is"):
        video.read_avi(avi)
    with pytest.raises(ValueError, match="frame 1 is"):
        video.read_avi(avi, device="cuda")


def test_decode_on_a_side_stream_orders_the_caller(video):
    """decode_jpeg_device(stream=side): the result is allocated on `side`, and the caller's current
    stream waits for `side` before the call returns, so the copy back below (on the current
    stream, no device-wide synchronize) reads finished frames.  As for the mp4v decode, this pins
    the path; a missing wait is a race and need not fail here."""
    datas = [J.encode(J.image(70, 45, "noise", seed=k), subsampling=k % 3, quality=90) for k in range(6)]
    side = torch.cuda.Stream()
    got = video.decode_jpeg_device(datas, stream=side)
    np.testing.assert_array_equal(got.cpu().numpy(), host(datas))


def test_mjpeg_recordings_match_npy(project, monkeypatch, tmp_path):  # noqa: F811
    """record_and_estimate_pose on per-camera Motion-JPEG AVIs (8 skeleton frames, 2 cameras; the
    device decode is the default) writes kpts_2d / heatmaps_2d / kpts_3d equal, bit for bit, to
    the run fed .npy stacks of the PIL-decoded frames."""
    from mvpose import cli, video
    root, names, _, _ = project
    monkeypatch.setenv("MVPOSE_RANDOM_WEIGHTS", "1")
    monkeypatch.setenv("MVPOSE_NO_DETECTOR", "1")
    monkeypatch.chdir(root)
    runs = {}
    for kind in ("avi", "npy"):
        rec = root / "configurations" / "1" / "recordings" / f"mjpeg_{kind}"
        rec.mkdir(parents=True, exist_ok=True)
        paths = []
        for v in range(2):
            avi = tmp_path / f"camera{v}.avi"
            if kind == "avi":
                video.write_avi(avi, skeleton_rgb(8, 20 + v, 352, 640), codec="mjpeg")
                p = rec / f"camera{v}.avi"
                p.write_bytes(avi.read_bytes())
            else:
                p = rec / f"camera{v}.npy"
                np.save(p, video.read_recording(avi, 0, None))
            paths.append(str(p))
        log = cli.record_and_estimate_pose_main(["--camera_names", *names, "--configuration_number", "1",
                                                 "--recording_paths", *paths])
        runs[kind] = {k: np.load(log[k]) for k in ("kpts_2d", "heatmaps_2d", "kpts_3d")}
    assert runs["avi"]["kpts_2d"].shape == (7, 17, 3, 2)              # 8 frames, the last dropped ([0, -1])
    for k in ("kpts_2d", "heatmaps_2d", "kpts_3d"):
        np.testing.assert_array_equal(runs["avi"][k], runs["npy"][k], err_msg=k)
