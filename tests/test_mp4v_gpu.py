"""GPU: the split MPEG-4 Part 2 decode — host entropy decoding (mvp_mp4v_parse) + device
reconstruction (mvp_mp4v_reconstruct, csrc/mp4v_recon.hip) — returns, on the device, exactly the
BGR frames the host decoder (mvp_mp4v_decode) writes: every frame, every slice, every container
(MP4 / AVI / raw), mixed macroblock types (1MV, 4MV, skip, intra-in-P), a not-coded VOP, sizes
that are not multiples of 16 with vectors past the picture edge, MPEG quantisation, GOPs of
different lengths decoded as parallel slots, and the rarer paths of tests/test_mp4v_paths.py
(video packets with lost macroblocks, the intra DC through the AC VLC, saturated and 384-entry
macroblocks, frames of one macroblock and less).  Replaces cv.VideoCapture's decode of the
reference's mp4v recordings (utils.py:849-909; synchronize_videos.py:64,240); parity against
cv2 / FFmpeg is unpinned (neither exists in this image)."""
import numpy as np
import pytest
import torch

import mp4v_writer as W
from test_mp4v_split import mixed_stream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def video():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mvpose import video as v
    return v


def _gops(n_gops, w_mb, h_mb, seed, vol=None, qt=0):
    """n_gops GOPs of different lengths (mixed_stream: I + P + not-coded + P ...) back to back."""
    cfg, samples = None, []
    for g in range(n_gops):
        c, s, w, h = mixed_stream(w_mb, h_mb, 1 + (g % 3), seed + g, vol_wh=vol, quant_type=qt)
        cfg = c
        samples += s
    return cfg, samples, w, h


@pytest.mark.parametrize("w_mb,h_mb,vol,qt", [(4, 3, None, 0), (5, 3, (72, 40), 0), (4, 3, None, 1),
                                              (3, 2, (41, 19), 0)])
def test_device_frames_equal_host_frames(video, w_mb, h_mb, vol, qt):
    cfg, samples, w, h = _gops(5, w_mb, h_mb, 10 * w_mb + h_mb, vol, qt)
    host = video.decode_mp4v(cfg, samples, 0, None, threads=1)
    for sl in [(0, None), (0, -1), (3, 11), (7, 8), (len(samples) - 1, None)]:
        got = video.decode_mp4v_device(cfg, samples, *sl, threads=4)
        torch.cuda.synchronize()
        assert got.is_cuda and got.dtype == torch.uint8 and got.shape[1:] == (h, w, 3)
        np.testing.assert_array_equal(got.cpu().numpy(), host[slice(*sl)], err_msg=f"slice {sl}")


def test_device_decode_720p_stream(video):
    """The bench's 1280x720 mp4v workload shape (I + 11 P, +-3 px motion): 2 GOPs, bit-identical."""
    rng = np.random.default_rng(3)
    w, h = 1280, 720
    mw, mh = w // 16, h // 16

    def intra():
        b = np.zeros((6, 64), np.int64)
        for n in range(6):
            b[n, 0] = rng.integers(40, 160) if n < 4 else rng.integers(80, 140)
            m = rng.random(63) < 0.05
            b[n, 1:][m] = rng.integers(-4, 5, m.sum())
        return {"q": 6, "blocks": b, "ac_pred": False}

    def inter():
        b = np.zeros((6, 64), np.int64)
        m = rng.random((6, 64)) < 0.01
        b[m] = rng.integers(-2, 3, m.sum())
        return {"type": "inter", "mv": (int(rng.integers(-6, 7)), int(rng.integers(-6, 7))), "blocks": b}

    vw = W.VopWriter(w, h)
    i_vop = vw.i_vop([[intra() for _ in range(mw)] for _ in range(mh)], 6)
    p_vops = [vw.p_vop([[inter() for _ in range(mw)] for _ in range(mh)], 6, rounding=k % 2) for k in range(2)]
    samples = ([i_vop] + [p_vops[k % 2] for k in range(11)]) * 2
    cfg = W.vol_header(w, h)
    host = video.decode_mp4v(cfg, samples)
    got = video.decode_mp4v_device(cfg, samples).cpu().numpy()
    np.testing.assert_array_equal(got, host)


def test_read_recording_device_containers(video, tmp_path):
    """MP4, AVI (XVID) and raw .m4v containers through read_recording(device=...): the host
    reader's frames, on the device; the reference's [0, -1] slice drops the last frame."""
    from test_mp4v import _write_avi_mp4v
    cfg, samples, w, h = _gops(3, 4, 3, 77)
    host = video.decode_mp4v(cfg, samples)
    mp4 = tmp_path / "cam0_synced.mp4"
    mp4.write_bytes(W.mp4_file(cfg, samples, w, h, chunk=2))
    m4v = tmp_path / "cam0.m4v"
    m4v.write_bytes(cfg + b"".join(samples))
    avi = tmp_path / "cam0.avi"
    _write_avi_mp4v(avi, [cfg + samples[0]] + samples[1:], w, h)
    for p in (mp4, m4v, avi):
        got = video.read_recording(p, 0, -1, device="cuda")
        assert isinstance(got, torch.Tensor) and got.is_cuda
        np.testing.assert_array_equal(got.cpu().numpy(), host[:-1], err_msg=str(p))


# ------------------------------------------------------------------ the paths of tests/test_mp4v_paths.py
import test_mp4v_paths as P  # noqa: E402  (the CPU builders, shared)

PATH_STREAMS = {
    "mpeg_custom": lambda n_p, seed: P.mpeg_gop(n_p, seed, "custom"),     # quant_type 1, loaded matrices, saturation
    "packets_lost": P.packet_gop,                                        # video packets, MB_LOST in coded VOPs
    "dc_switch": P.dc_switch_gop,                                        # intra DC through the AC VLC (mask bit 0)
    "magnitudes": P.magnitude_gop,                                       # -2048 / 2047 entries, 384 per MB, clip8
    "one_macroblock": P.tiny_gop,                                        # 16 x 16: a one-block grid
    "vol_8x8": lambda n_p, seed: P.tiny_gop(n_p, seed, vol_wh=(8, 8)),   # the frame is a corner of one macroblock
}


def _concat(gops):
    assert all(g.cfg == gops[0].cfg for g in gops)
    return gops[0].cfg, [s for g in gops for s in g.samples], gops[0].w, gops[0].h


@pytest.mark.parametrize("name", list(PATH_STREAMS))
def test_device_equals_host_on_the_rarer_paths(video, name):
    """Three GOPs of different lengths (4, 2 and 3 VOPs: a launch mixes intra, inter, lost and
    absent jobs across the slots), each in a fresh slot on the device and a fresh decoder on the
    host (decode_mp4v), whole and as an interior slice."""
    cfg, samples, w, h = _concat([PATH_STREAMS[name](n_p, 300 + n_p) for n_p in (3, 1, 2)])
    host = video.decode_mp4v(cfg, samples, 0, None, threads=1)
    assert host.shape == (9, h, w, 3)
    for sl in [(0, None), (2, 7)]:
        got = video.decode_mp4v_device(cfg, samples, *sl, threads=3)
        np.testing.assert_array_equal(got.cpu().numpy(), host[slice(*sl)], err_msg=f"slice {sl}")


def test_device_dense_gop_stitches_coefficient_chunks(video):
    """Every macroblock of every VOP holds 384 entries: mvp_mp4v_parse_many returns before the
    GOP's end (asserted on its `done`), so decode_mp4v_device stitches several chunks per GOP."""
    dense = [P.dense_gop(3, 95), P.dense_gop(1, 96)]
    done, _ = P.parse_many_done(dense[0])
    assert 1 <= done < len(dense[0].samples)
    cfg, samples, w, h = _concat(dense)
    host = video.decode_mp4v(cfg, samples, 0, None, threads=1)
    for sl in [(0, None), (1, 5)]:
        got = video.decode_mp4v_device(cfg, samples, *sl, threads=2)
        np.testing.assert_array_equal(got.cpu().numpy(), host[slice(*sl)], err_msg=f"slice {sl}")


def test_device_decode_on_a_side_stream_orders_the_caller(video):
    """decode_mp4v_device(stream=side) returns a tensor the caller's current stream may read at
    once: it is allocated on `side` and the current stream waits for `side` before the call
    returns.  The copy back below runs on the current stream and waits for that stream alone (no
    device-wide synchronize).  The defect this guards against was a race (output allocated on one
    stream, written on another, nothing ordering the two), so this test cannot be relied on to
    fail without the fix: it pins the path, not the bug."""
    st = P.packet_gop(3, 310)
    host = video.decode_mp4v(st.cfg, st.samples, 0, None, threads=1)
    side = torch.cuda.Stream()
    got = video.decode_mp4v_device(st.cfg, st.samples, stream=side)
    np.testing.assert_array_equal(got.cpu().numpy(), host)
