"""numpy restatement of libjpeg's baseline reconstruction, from parsed coefficients only (no
Huffman code here): dequantisation, jidctint.c's "islow" IDCT, jdsample.c's "fancy" h2v1 / h2v2
upsampling and jdcolor.c's fixed-point YCbCr -> RGB.  The oracle between mvp_jpeg_parse's output
and PIL's decode (tests/test_jpeg_parse.py), and the image / case generators both JPEG test files
share."""
import io

import numpy as np

CONST_BITS, PASS1_BITS = 13, 2


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _idct8(d, n):
    """One 8-point pass of jpeg_idct_islow over d[0..7] (int32 arrays), descaled by n."""
    z2, z3 = d[2], d[6]
    z1 = (z2 + z3) * 4433
    tmp2 = z1 - z3 * 15137
    tmp3 = z1 + z2 * 6270
    z2, z3 = d[0], d[4]
    tmp0 = (z2 + z3) << CONST_BITS
    tmp1 = (z2 - z3) << CONST_BITS
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = d[7], d[5], d[3], d[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3, z4 = z3 * -16069 + z5, z4 * -3196 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    return [_descale(v, n) for v in (tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0,
                                     tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3)]


def idct_islow(blocks):
    """(n, 8, 8) int32 dequantised coefficients -> (n, 8, 8) uint8 samples: the column pass, the
    row pass, + 128, clamped."""
    b = blocks.astype(np.int32)
    ws = np.stack(_idct8([b[:, k, :] for k in range(8)], CONST_BITS - PASS1_BITS), axis=1)
    out = np.stack(_idct8([ws[:, :, k] for k in range(8)], CONST_BITS + PASS1_BITS + 3), axis=2)
    return np.clip(out + 128, 0, 255).astype(np.uint8)


def _h_fancy(p, rnd_even, rnd_odd, shift, edge_scale):
    """Triangle filter along x of int32 rows p: out[2i] = 3 p[i] + p[i-1], out[2i+1] = 3 p[i] +
    p[i+1]; the first / last outputs have no outside neighbour: edge_scale * p."""
    h, w = p.shape
    out = np.empty((h, 2 * w), np.int32)
    out[:, 0] = (edge_scale * p[:, 0] + rnd_even) >> shift
    out[:, 2::2] = (3 * p[:, 1:] + p[:, :-1] + rnd_even) >> shift
    out[:, 1:-1:2] = (3 * p[:, :-1] + p[:, 1:] + rnd_odd) >> shift
    out[:, -1] = (edge_scale * p[:, -1] + rnd_odd) >> shift
    return out


def upsample(plane, hs, vs):
    """A chroma plane of its REAL size -> hs x vs times as large, as jdsample.c does it: fancy only
    for planes more than 2 samples wide, replication otherwise."""
    p = plane.astype(np.int32)
    if hs == 1:
        return p
    if p.shape[1] <= 2:
        return np.repeat(np.repeat(p, vs, axis=0), 2, axis=1)
    if vs == 1:
        out = _h_fancy(p, 1, 2, 2, 4)
        out[:, 0], out[:, -1] = p[:, 0], p[:, -1]
        return out
    up = np.concatenate([p[:1], p[:-1]])
    down = np.concatenate([p[1:], p[-1:]])
    rows = np.empty((2 * p.shape[0], p.shape[1]), np.int32)
    rows[0::2] = 3 * p + up
    rows[1::2] = 3 * p + down
    return _h_fancy(rows, 8, 7, 4, 4)


def reconstruct(info, qt, off, coef):
    """mvp_jpeg_parse's output of one frame -> its (H, W, 3) uint8 BGR pixels."""
    W, H, nc = int(info["width"]), int(info["height"]), int(info["components"])
    hs, vs = int(info["h_samp"]), int(info["v_samp"])
    mcu_w, mcu_h = -(-W // (8 * hs)), -(-H // (8 * vs))
    per = hs * vs + nc - 1
    nb = per * mcu_w * mcu_h
    assert nb == int(info["blocks"]) and off.size == nb + 1 and off[-1] == coef.size
    q = np.zeros((nb, 64), np.int32)
    owner = np.repeat(np.arange(nb), np.diff(off.astype(np.int64)))
    q[owner, coef >> 16] = (coef & 0xffff).astype(np.uint16).view(np.int16)
    j = np.arange(nb) % per
    comp = np.where(j < hs * vs, 0, j - hs * vs + 1)
    pix = idct_islow((q * qt.astype(np.int32)[comp]).reshape(nb, 8, 8))
    m = np.arange(nb) // per
    mx, my = m % mcu_w, m // mcu_w
    planes = []
    for c in range(nc):
        sel = comp == c
        bx = np.where(c == 0, mx * hs + j % hs, mx)[sel]
        by = np.where(c == 0, my * vs + j // hs, my)[sel]
        ch, cv = (hs, vs) if c == 0 else (1, 1)
        pl = np.zeros((8 * mcu_h * cv, 8 * mcu_w * ch), np.uint8)
        for b, x, y in zip(pix[sel], bx, by):
            pl[8 * y:8 * y + 8, 8 * x:8 * x + 8] = b
        planes.append(pl)
    Y = planes[0][:H, :W].astype(np.int32)
    if nc == 1:
        return np.repeat(Y[:, :, None], 3, axis=2).astype(np.uint8)
    rw, rh = -(-W // hs), -(-H // vs)
    cb = upsample(planes[1][:rh, :rw], hs, vs)[:H, :W] - 128
    cr = upsample(planes[2][:rh, :rw], hs, vs)[:H, :W] - 128
    r = Y + ((91881 * cr + 32768) >> 16)
    g = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = Y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([b, g, r], axis=2), 0, 255).astype(np.uint8)


# ---------------------------------------------------------------- images and cases
SIZES = ((70, 45), (17, 9), (16, 16), (8, 8), (1, 1))        # (W, H)
QUALITIES = (30, 75, 90, 100)
RESTARTS = ({}, {"restart_marker_blocks": 3}, {"restart_marker_rows": 1})
SUBSAMPLINGS = (0, 1, 2, "gray")                              # PIL: 0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0


def image(w, h, kind, seed=0):
    """(h, w, 3) uint8 RGB: a smooth colour ramp, or uniform noise (at quality 100 it drives the
    IDCT to its clamps)."""
    if kind == "noise":
        return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    ph = 0.37 * seed
    return np.stack([127.5 + 127.5 * np.sin(x / 9.0 + ph), 127.5 + 127.5 * np.cos(y / 7.0 + ph),
                     (255.0 * (x + y) / max(1, w + h - 2) + 40 * seed) % 256], axis=2).astype(np.uint8)


def encode(rgb, subsampling=2, quality=90, **opts):
    """PIL's JPEG bytes of an RGB image; subsampling "gray" saves its luma as a 1-component file."""
    from PIL import Image
    im = Image.fromarray(rgb)
    b = io.BytesIO()
    if subsampling == "gray":
        im.convert("L").save(b, "JPEG", quality=quality, **opts)
    else:
        im.save(b, "JPEG", quality=quality, subsampling=subsampling, **opts)
    return b.getvalue()


def pil_bgr(data):
    """What the host reader returns for a frame today: PIL's RGB decode, as BGR."""
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[:, :, ::-1]


def matrix():
    """The trimmed cross product: for every subsampling, every size x every quality (20 cases),
    with optimize, the restart setting and the content cycling underneath at coprime periods, so
    every value of every axis occurs for every subsampling.  -> [(id, size, kwargs for encode,
    content kind)]."""
    cases = []
    for sub in SUBSAMPLINGS:
        i = 0
        for size in SIZES:
            for quality in QUALITIES:
                opts = dict(RESTARTS[i % 3], optimize=bool(i % 2))
                kind = ("ramp", "noise")[(i // 2 + i // 6) % 2]
                rs = "-".join(f"{k.split('_')[-1]}{v}" for k, v in RESTARTS[i % 3].items()) or "norst"
                cid = f"{sub}-{size[0]}x{size[1]}-q{quality}-{'opt' if opts['optimize'] else 'std'}-{rs}-{kind}"
                cases.append((cid, size, dict(subsampling=sub, quality=quality, **opts), kind))
                i += 1
    return cases


def case_bytes(case, seed=0):
    _, (w, h), kw, kind = case
    return encode(image(w, h, kind, seed), **kw)


def strip_dht(data, app0=b"AVI1\0\0\0\0\0\0\0\0\0\0"):
    """The frame without its DHT segments and with an 'AVI1' APP0 segment in front (what
    Motion-JPEG AVI writers emit)."""
    out, p = bytearray(data[:2]), 2
    out += b"\xff\xe0" + (len(app0) + 2).to_bytes(2, "big") + app0
    while data[p + 1] != 0xDA:
        n = 2 + int.from_bytes(data[p + 2:p + 4], "big")
        if data[p + 1] != 0xC4:
            out += data[p:p + n]
        p += n
    return bytes(out + data[p:])


def insert_segment(data, marker, payload):
    """The frame with one more marker segment right after SOI."""
    return data[:2] + bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload + data[2:]


if __name__ == "__main__":
    # python tests/jpeg_ref.py DIR: the matrix's frames (+ a DHT-less, a progressive and an Adobe
    # one) as files, for the stand-alone sanitizer run of tools/jpeg_parse_check.cpp
    import os
    import sys
    out = sys.argv[1]
    os.makedirs(out, exist_ok=True)
    frames = {c[0]: case_bytes(c) for c in matrix()}
    base = encode(image(70, 45, "noise", 3), subsampling=2, quality=75)
    frames["dhtless"] = strip_dht(base)
    frames["progressive"] = encode(image(70, 45, "ramp"), subsampling=2, quality=75, progressive=True)
    frames["adobe"] = insert_segment(base, 0xEE, b"Adobe\0\x64\0\0\0\0\0")
    for name, data in frames.items():
        with open(os.path.join(out, f"{name}.jpg"), "wb") as f:
            f.write(data)
    print(f"{len(frames)} frames -> {out}")
