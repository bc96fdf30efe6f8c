"""CPU: the host half of the split JPEG decode (csrc/jpeg.cpp).  mvp_jpeg_parse's offsets and
quantised coefficients, reconstructed by the numpy restatement of libjpeg's arithmetic
(tests/jpeg_ref.py), equal PIL's decode of the same bytes bit for bit; what the parser does not
take is reported as unsupported, what is broken as an error."""
import io

import numpy as np
import pytest

import jpeg_ref as J

CASES = J.matrix()


@pytest.fixture(scope="module")
def video():
    from mvpose import video
    return video


def decode(video, data):
    info, qt, off, coef = video.parse_jpeg(data)
    assert info["status"] == 0, video.JPEG_UNSUPPORTED.get(int(info["status"]))
    return J.reconstruct(info, qt, off, coef)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_parse_then_reference_equals_pil(video, case):
    data = J.case_bytes(case)
    info = video.jpeg_info(data, check_range=True)
    w, h = case[1]
    sub = case[2]["subsampling"]
    assert (info["width"], info["height"], info["status"]) == (w, h, 0)
    assert (info["components"], info["h_samp"], info["v_samp"]) == {
        0: (3, 1, 1), 1: (3, 2, 1), 2: (3, 2, 2), "gray": (1, 1, 1)}[sub]
    np.testing.assert_array_equal(decode(video, data), J.pil_bgr(data))


@pytest.mark.parametrize("width", [1, 2, 3, 4, 5, 6, 7])
@pytest.mark.parametrize("sub", [1, 2])
def test_narrow_frames(video, width, sub):
    """libjpeg upsamples a chroma plane of at most 2 samples by replication, wider ones with the
    triangle filter: the widths on both sides of that switch."""
    data = J.encode(J.image(width, 5, "noise", seed=width), subsampling=sub, quality=95)
    np.testing.assert_array_equal(decode(video, data), J.pil_bgr(data))


@pytest.mark.parametrize("sub", J.SUBSAMPLINGS)
def test_frame_without_huffman_tables(video, sub):
    """Motion-JPEG's habit: no DHT segments (the Annex K tables are meant) and an 'AVI1' APP0."""
    data = J.encode(J.image(70, 45, "noise", seed=3), subsampling=sub, quality=75)
    bare = J.strip_dht(data)
    assert b"\xff\xc4" not in bare[:bare.index(b"\xff\xda")] and len(bare) < len(data)
    np.testing.assert_array_equal(decode(video, bare), decode(video, data))
    np.testing.assert_array_equal(decode(video, bare), J.pil_bgr(data))


def test_fill_bytes_and_trailer(video):
    data = J.encode(J.image(70, 45, "ramp"), subsampling=2, quality=75, restart_marker_blocks=3)
    ref = J.pil_bgr(data)
    sos = data.index(b"\xff\xda")
    rst = data.index(b"\xff\xd1", sos)
    padded = data[:sos] + b"\xff\xff" + data[sos:rst] + b"\xff\xff\xff" + data[rst:-2] + b"\xff" + data[-2:]
    padded += b"junk after the end \xff\xd8\xff\xda\x00"
    np.testing.assert_array_equal(decode(video, padded), ref)
    np.testing.assert_array_equal(J.pil_bgr(padded), ref)


def dqt_out_of_range():
    """A frame whose luma table is rewritten to 255 everywhere: noise coded at quality 100 has
    coefficients far above 32767 / 255 = 128."""
    data = bytearray(J.encode(J.image(16, 16, "noise"), subsampling=0, quality=100))
    p = data.index(b"\xff\xdb")
    assert data[p + 4] == 0                               # 8-bit table 0
    data[p + 5:p + 5 + 64] = b"\xff" * 64
    return bytes(data)


def test_unsupported_frames_are_reported(video):
    rgb = J.image(70, 45, "ramp")
    base = J.encode(rgb, subsampling=2, quality=75)
    assert video.jpeg_info(base, check_range=True)["status"] == 0
    prog = J.encode(rgb, subsampling=2, quality=75, progressive=True)
    adobe = J.insert_segment(base, 0xEE, b"Adobe\0\x64\0\0\0\0\0")        # transform 0
    reasons = {v: k for k, v in video.JPEG_UNSUPPORTED.items()}
    assert video.jpeg_info(prog)["status"] == reasons["process"]
    assert video.jpeg_info(adobe)["status"] == reasons["colour"]
    assert video.jpeg_info(dqt_out_of_range(), check_range=True)["status"] == reasons["range"]
    for data in (prog, adobe, dqt_out_of_range()):
        info, qt, off, coef = video.parse_jpeg(data)
        assert info["status"] != 0 and qt is None and off is None and coef is None
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(rgb).convert("CMYK").save(b, "JPEG")
    assert video.jpeg_info(b.getvalue())["status"] in (reasons["components"], reasons["colour"])


def truncations(data):
    sos = data.index(b"\xff\xda")
    return sorted({1, 3, 11, data.index(b"\xff\xdb") + 7, data.index(b"\xff\xc0") + 5, sos + 1, sos + 9, sos + 14,
                   sos + 15, (sos + len(data)) // 2, len(data) - 40, len(data) - 3, len(data) - 2})


def test_truncated_frames_are_errors(video):
    from mvpose import _lib
    for kw in ({}, {"restart_marker_blocks": 3}):
        data = J.encode(J.image(70, 45, "noise"), subsampling=2, quality=90, **kw)
        for cut in truncations(data):
            with pytest.raises(_lib.MvposeError, match="jpeg:"):
                video.jpeg_info(data[:cut], check_range=True)
            with pytest.raises(_lib.MvposeError, match="jpeg:"):
                video.parse_jpeg(data[:cut])               # (the headers alone may still be whole)


def test_every_prefix_of_a_small_frame_is_an_error(video):
    """Also where the zero bits fed past the end decode to a coefficient that would fail the
    range condition: the truncation is what gets reported."""
    from mvpose import _lib
    for sub, kw in ((0, {"restart_marker_rows": 1}), (2, {})):
        data = J.encode(J.image(16, 16, "noise"), subsampling=sub, quality=30, **kw)
        assert data[-2:] == b"\xff\xd9"
        for cut in range(len(data)):
            with pytest.raises(_lib.MvposeError):
                video.jpeg_info(data[:cut], check_range=True)


def test_malformed_frames_are_errors(video):
    from mvpose import _lib
    data = J.encode(J.image(70, 45, "noise"), subsampling=2, quality=90, restart_marker_blocks=3)
    sos = data.index(b"\xff\xda")
    rst = data.index(b"\xff\xd0", sos)
    bad = [b"", b"\xff", b"not a jpeg at all", data[2:],
           data[:rst + 1] + b"\xd3" + data[rst + 2:],                     # a restart marker out of turn
           data[:sos + 20] + b"\xff\xd9" + data[sos + 22:]]               # EOI inside the scan
    for b in bad:
        with pytest.raises(_lib.MvposeError):
            video.parse_jpeg(b)
    # every byte of the scan flipped in turn: an error or some decode, never a crash
    rng = np.random.default_rng(0)
    for _ in range(200):
        m = bytearray(data)
        m[int(rng.integers(2, len(m)))] = int(rng.integers(0, 256))
        try:
            video.parse_jpeg(bytes(m))
        except _lib.MvposeError:
            pass


def test_parse_many_matches_parse(video):
    import ctypes
    from mvpose import _lib
    datas = [J.case_bytes(c) for c in CASES if c[1] == (70, 45)][:6]
    n = len(datas)
    blocks, plane = ctypes.c_int(), ctypes.c_int64()
    _lib.call("mvp_jpeg_scratch", 70, 45, ctypes.byref(blocks), ctypes.byref(plane))
    stride = blocks.value + 1
    ptrs = (ctypes.c_char_p * n)(*datas)
    sizes = np.array([len(d) for d in datas], np.uint64)
    info = np.zeros(n, video.JPEG_INFO_DTYPE)
    qt = np.zeros((n, 3, 64), np.uint16)
    off = np.zeros((n, stride), np.uint32)
    coef = np.zeros(n * 64 * blocks.value + 64, np.uint32)
    ncoef = np.zeros(n, np.int64)
    done = ctypes.c_int()
    _lib.call("mvp_jpeg_parse_many", n, ctypes.addressof(ptrs), sizes.ctypes.data, info.ctypes.data, qt.ctypes.data,
              off.ctypes.data, stride, coef.ctypes.data, coef.size, ncoef.ctypes.data, ctypes.byref(done))
    assert done.value == n
    first = np.cumsum(ncoef) - ncoef
    for k, data in enumerate(datas):
        i1, q1, o1, c1 = video.parse_jpeg(data)
        assert info[k] == i1
        np.testing.assert_array_equal(qt[k], q1)
        np.testing.assert_array_equal(off[k, :o1.size], o1)
        np.testing.assert_array_equal(coef[first[k]:first[k] + ncoef[k]], c1)
    # a buffer with room for three frames' bounds stops there, without an error
    room = sum(video._jpeg_entry_bound(int(info[k]["blocks"]), len(datas[k])) for k in range(3))
    _lib.call("mvp_jpeg_parse_many", n, ctypes.addressof(ptrs), sizes.ctypes.data, info.ctypes.data, qt.ctypes.data,
              off.ctypes.data, stride, coef.ctypes.data, room, ncoef.ctypes.data, ctypes.byref(done))
    assert 3 <= done.value < n
