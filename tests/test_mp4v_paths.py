"""CPU: the parts of the MPEG-4 Part 2 decoder (csrc/mp4v.cpp) that the plain streams of
tests/test_mp4v.py never enter, each held bit for bit to tests/mp4v_writer.py's independent
restatement (W.reconstruct) and, for the same streams, parse mode + the restated device
reconstruction (test_mp4v_split.reconstruct_records) held to the host decoder:

  stream builder        decoder paths reached (asserted from the stream's construction)
  --------------------  -----------------------------------------------------------------------
  mpeg_gop              dequant() quant_type 1: default / loaded / short-list matrices, intra and
                        inter formula, saturation to -2048 and 2047, mismatch control both ways
  packet_gop            at_resync, video_packet_header (quant_scale, header_extension_code), the
                        resync_x / resync_y / first_line branches of pred_dc and pred_mv, AC
                        prediction at packet boundaries (LAYOUTS says which layout reaches what)
  packet_gop + lost     MB_LOST records in coded VOPs (grey, then the picture two VOPs back)
  dc_switch_gop         intra_dc_vlc_thr 1-7: the intra DC through the AC VLC, the switch on the QP
                        before DQUANT, blocks whose only event is the DC, the parser's mask bit 0
  header variants       verid 2 / 5, VBV block, extended PAR, fixed_vop_rate, no object layer id
  magnitude_gop         escape-3 levels saturating at QP 31, the -2048 coefficient entry, a
                        macroblock of 384 entries, clip8 on both sides in inter + residual
  dense_gop             384 entries in every macroblock: mvp_mp4v_parse_many stops early
  tiny streams          one macroblock (mb_w == 1) with 4MV; a VOL smaller than a macroblock

tests/test_mp4v_gpu.py runs the same builders through the device kernel.  Parity against cv2 /
FFmpeg stays UNPINNED (neither exists here); the packet-boundary rules are the standard's
(7.4.3.3, 7.6.5), which FFmpeg's first-slice-line bookkeeping implements."""
import collections
import ctypes

import numpy as np
import pytest

import mp4v_writer as W
from mvpose import _lib, video
from test_mp4v import _planes
from test_mp4v_split import REC, _host_yuv, _parse, reconstruct_records

Stream = collections.namedtuple("Stream", "cfg samples w h vops kw stats")
MW, MH = 4, 3                       # the 64 x 48 grid of the issue: the smallest that reaches every branch
FIRST_ROW, FIRST_COL = np.arange(1, 8), 8 * np.arange(1, 8)


# ------------------------------------------------------------------ macroblock content
def _dc_level(pix, q, luma):
    return max(1, int(round(pix * 8 / W.dc_scale(q, luma))))


def _intra(rng, q, ac_pred=True, amp=6, density=0.15, flat=False):
    """An intra macroblock around mid grey; every block holds first-row and first-column
    coefficients, so AC prediction from a wrong block changes the picture."""
    b = np.zeros((6, 64), np.int64)
    for n in range(6):
        b[n, 0] = _dc_level(rng.integers(60, 200) if n < 4 else rng.integers(100, 156), q, n < 4)
        if flat:
            continue
        m = rng.random(63) < density
        b[n, 1:][m] = rng.integers(-amp, amp + 1, m.sum())
        for line in (FIRST_ROW, FIRST_COL):
            at = rng.choice(line, 3, replace=False)
            b[n, at] = rng.choice([-1, 1], 3) * rng.integers(1, amp + 1, 3)
    return {"q": q, "blocks": b, "ac_pred": ac_pred}


def _residual(rng, density=0.08, amp=4):
    b = np.zeros((6, 64), np.int64)
    m = rng.random((6, 64)) < density
    b[m] = rng.integers(-amp, amp + 1, m.sum())
    return b


def _spike(mb, block, pos, level):
    """One coefficient alone in its block (besides an intra DC): it saturates without its row or
    column of the IDCT leaving int16."""
    keep = mb["blocks"][block, 0] if mb.get("type", "intra") == "intra" else 0
    mb["blocks"][block] = 0
    mb["blocks"][block, 0] = keep
    mb["blocks"][block, pos] = level


def gop(n_p, seed, *, w_mb=MW, h_mb=MH, q0=6, q_range=(2, 12), packets=(), lost=(), p_types=None, fcode=1, dc_thr=0,
        mvmax=9, vol_wh=None, qwalk=None, edit=None, **vol_kw):
    """An I-VOP and n_p P-VOPs.  packets / lost: per VOP (cycled) the packet list of W.VopWriter
    and the lost macroblock numbers.  The first P-VOP is all 4MV; later ones draw from p_types.
    qwalk(k, n, q) -> the QP of macroblock n of VOP k (default: a random DQUANT walk);
    edit(k, mbs): changes VOP k's macroblocks in place before it is written."""
    rng = np.random.default_rng(seed)
    w, h = 16 * w_mb, 16 * h_mb
    vw = W.VopWriter(w, h)
    lim = min(mvmax, (32 << (fcode - 1)) - 1)
    p_types = p_types or (["inter", "inter4v", "skip", "intra"], [0.25, 0.25, 0.1, 0.4])
    samples, vops = [], []
    for k in range(n_p + 1):
        pk = list(packets[k % len(packets)]) if packets else []
        gone = set(lost[k % len(lost)]) if lost else set()
        opts = dict((e, {}) if isinstance(e, int) else e for e in pk)
        q, rows = q0, []
        for y in range(h_mb):
            row = []
            for x in range(w_mb):
                n = y * w_mb + x
                if n in gone:
                    row.append(None)
                    continue
                q = opts.get(n, {}).get("q", q)
                t = "intra" if k == 0 else "inter4v" if k == 1 else str(rng.choice(p_types[0], p=p_types[1]))
                if t in ("intra", "inter"):
                    q = int(qwalk(k, n, q) if qwalk else np.clip(q + rng.integers(-2, 3), *q_range))
                if t == "intra":
                    mb = dict(_intra(rng, q), type="intra")
                elif t == "skip":
                    mb = {"type": "skip"}
                elif t == "inter":
                    mb = {"type": "inter", "q": q, "blocks": _residual(rng),
                          "mv": (int(rng.integers(-lim, lim + 1)), int(rng.integers(-lim, lim + 1)))}
                else:
                    mb = {"type": "inter4v", "q": q, "blocks": _residual(rng),
                          "mvs": [(int(rng.integers(-lim, lim + 1)), int(rng.integers(-lim, lim + 1))) for _ in range(4)]}
                row.append(mb)
            rows.append(row)
        if edit:
            edit(k, rows)
        if k == 0:
            samples.append(vw.i_vop(rows, q0, dc_thr=dc_thr, packets=pk))
        else:
            samples.append(vw.p_vop(rows, q0, rounding=k % 2, fcode=fcode, dc_thr=dc_thr, packets=pk))
        vops.append(("I" if k == 0 else "P", rows, q0, k % 2 if k else 0))
    vol_kw.setdefault("resync_disable", 0 if packets else 1)
    kw = {key: vol_kw[key] for key in ("quant_type", "intra_matrix", "inter_matrix") if key in vol_kw}
    vol_w, vol_h = vol_wh or (w, h)
    return Stream(W.vol_header(vol_w, vol_h, **vol_kw), samples, vol_w, vol_h, vops, kw, vw.stats)


def check(st, restatement=True):
    """host decoder == W.reconstruct (int32 / int16-safe IDCT inputs asserted), and parse mode +
    the restated device reconstruction == host decoder.  -> (host I420 buffers, parsed samples)"""
    host = _host_yuv(st.cfg, st.samples)
    if restatement:
        exp = W.reconstruct(st.w, st.h, st.vops, strict_idct=True, **st.kw)
        for k, (buf, ef) in enumerate(zip(host, exp)):
            for p, (g, e) in enumerate(zip(_planes(buf, st.w, st.h), ef)):
                np.testing.assert_array_equal(g, e, err_msg=f"host vs restatement: VOP {k} plane {p}")
    parsed = _parse(st.cfg, st.samples)
    for k, (g, e) in enumerate(zip(reconstruct_records(parsed, st.w, st.h), host)):
        np.testing.assert_array_equal(g, e, err_msg=f"records vs host: VOP {k}")
    return host, parsed


def _kinds(parsed):
    return [p[0].view(REC)["kind"].copy() for p in parsed]


# ------------------------------------------------------------------ MPEG quantisation
def _custom_matrices(seed=40):
    rng = np.random.default_rng(seed)
    intra = rng.integers(8, 41, 64)
    intra[0] = 8
    return intra, rng.integers(10, 41, 64)


MPEG_MATRICES = {
    "default": (None, None),
    "custom": _custom_matrices(),
    "short": ([8, 12, 14, 40, 9, 31, 17, 22, 13, 25], [33, 16, 11, 28, 19]),    # zigzag order, then a 0
}
SPIKE = 1500       # (2 * 1500 * q * W) // 16 >= 187 * 2 * 8 > 2047 for every QP >= 2 and weight >= 8


def mpeg_gop(n_p, seed, matrices="custom"):
    """MPEG quantisation: I-VOP with DQUANT and AC prediction, P-VOPs with intra-in-P, 1MV + DQUANT,
    4MV; one coefficient saturating on each side in an intra and in an inter macroblock."""
    im, pm = MPEG_MATRICES[matrices]

    def edit(k, mbs):
        if k > 1:
            return
        _spike(mbs[0][1], 0, 10, SPIKE)
        _spike(mbs[0][1], 3, 17, -SPIKE)
        _spike(mbs[1][2], 5, 27, -SPIKE)
        _spike(mbs[2][0], 1, 12, SPIKE)

    return gop(n_p, seed, quant_type=1, intra_matrix=im, inter_matrix=pm, edit=edit)


def mpeg_census(st):
    """From the restatement: per (intra, inter), the pre-mismatch sum parities seen and the counts
    of coefficients at each saturation bound."""
    mats = [W.expand_matrix(st.kw["inter_matrix"], W.DEFAULT_INTER_MATRIX),
            W.expand_matrix(st.kw["intra_matrix"], W.DEFAULT_INTRA_MATRIX)]
    seen = {True: collections.Counter(), False: collections.Counter()}
    for _, mbs, _, _ in st.vops:
        for mb in (m for row in mbs for m in row if m and m["type"] != "skip"):
            intra = mb["type"] == "intra"
            for n in range(6):
                if not intra and not mb["blocks"][n].any():
                    continue
                d = W.dequant_mpeg(mb["blocks"][n], mb["q"], intra, n < 4, mats[int(intra)], mismatch=False)
                seen[intra]["even" if int(d.sum()) % 2 == 0 else "odd"] += 1
                seen[intra]["hi"] += int((d[1:] == 2047).sum())
                seen[intra]["lo"] += int((d[1:] == -2048).sum())
    return seen


def test_default_matrices_are_the_standards_listing():
    """The writer's default matrices are symmetric where the standard's are and keep its corner
    values; expand_matrix repeats a short list's last value over the rest of the zigzag order."""
    assert W.DEFAULT_INTRA_MATRIX[[0, 7, 56, 63]].tolist() == [8, 27, 27, 45]
    assert W.DEFAULT_INTER_MATRIX[[0, 7, 56, 63]].tolist() == [16, 23, 23, 33]
    m = W.expand_matrix([8, 12, 14])
    assert m[[0, 1, 8]].tolist() == [8, 12, 14] and (np.delete(m, [0, 1, 8]) == 14).all()


@pytest.mark.parametrize("matrices", list(MPEG_MATRICES))
def test_mpeg_quantisation(matrices):
    """quant_type 1 against dequant_mpeg: default matrices (a wrong entry in either listing fails
    here), loaded intra + inter matrices, the short-list form."""
    st = mpeg_gop(2, 50, matrices)
    seen = mpeg_census(st)
    for intra in (True, False):
        assert seen[intra]["even"] and seen[intra]["odd"], seen          # mismatch control toggles and does not
        assert seen[intra]["hi"] and seen[intra]["lo"], seen             # both saturation bounds
    types = {m["type"] for _, mbs, _, _ in st.vops[1:] for row in mbs for m in row}
    assert {"intra", "inter", "inter4v"} <= types
    qs = [m["q"] for _, mbs, _, _ in st.vops for row in mbs for m in row if "q" in m]
    assert len(set(qs)) > 3                                              # DQUANT moved the QP
    check(st)


def test_loaded_matrices_change_the_picture():
    """The loaded matrices reach the inverse quantisation: the same coefficients under the default
    and the loaded matrices decode to different pictures (so test_mpeg_quantisation's custom cases
    cannot pass on a decoder that ignores the load)."""
    a = _host_yuv(*mpeg_gop(1, 51, "default")[:2])
    b = _host_yuv(*mpeg_gop(1, 51, "short")[:2])
    assert all((x != y).any() for x, y in zip(a, b))


# ------------------------------------------------------------------ video packets
# name: (packet lists per VOP, lost macroblocks per VOP, what the layout reaches).  Macroblock n is
# (n % 4, n // 4) on the 4 x 3 grid; rx / ry are the decoder's resync_x / resync_y.
LAYOUTS = {
    "mid_row": ([[5]], (), "rx = 1 mid-row: the left / above-left / above candidates of macroblock 5 lie in the "
                "previous packet; row 2 holds mb_x + 1 == rx at mb_x == 0 (pred_mv takes C alone) in the first line"),
    "last_column": ([[3, 7]], (), "rx = 3: row ry + 1 holds mb_x == 0 and mb_x + 1 == rx (median of A, 0, C) inside the "
                    "first packet line, and first_line ends at (rx, ry + 1) with B outside the packet"),
    "row_start": ([[4, 8]], (), "rx = 0: first_line ends one full row later; only the top candidates are outside"),
    "one_macroblock": ([[5, 6], [1, 2, 11]], (), "packets of a single macroblock: every candidate outside, mid-row "
                       "and in the last column"),
    "quant_scale": ([[(6, {"q": 11})], [(2, {"q": 3}), (9, {"q": 12})]], (), "quant_scale replaces the running QP; AC "
                    "prediction rescales across the QP step inside the packet only"),
    "hec": ([[(2, {"hec": True}), (7, {"hec": True, "q": 5})]], (), "header_extension_code: the time fields, "
            "vop_coding_type, intra_dc_vlc_thr and (P) fcode are stepped over"),
    "lost": ([[6], [(3, {"hec": True}), 11], [(9, {"q": 4})]], ([4, 5], [1, 2, 10], [7, 8]), "macroblock_number jumps: "
             "MB_LOST records; grey in the first two coded VOPs, the picture two VOPs back in the third"),
}


def packet_gop(n_p, seed, layout="lost", fcode=1):
    """The I-VOP's first packet starts (unless its header sets quant_scale) at QP 4 on a macroblock
    whose block 0 reconstructs to DC 128 x 8 = 1024: block 2 then sees A = B = C = 1024 and
    predicts from the left, from outside the packet; blocks 0, 4 and 5 of every packet start do
    so anyway (A = B = C = 1024)."""
    packets, lost, _ = LAYOUTS[layout]
    opts = dict((e, {}) if isinstance(e, int) else e for e in packets[0])
    first = min(opts)
    pin = "q" not in opts[first]
    rng = np.random.default_rng(seed + 500)

    def qwalk(k, n, q):
        step = int(rng.integers(-2, 3))
        if k == 0 and pin and n <= first:
            return 4 if n == first else int(np.clip(q + step, 4, 6))
        return int(np.clip(q + step, 2, 12))

    def edit(k, mbs):
        if k == 0 and pin:
            mbs[first // MW][first % MW]["blocks"][0, 0] = 128

    return gop(n_p, seed, packets=packets, lost=lost, fcode=fcode, mvmax=40, qwalk=qwalk, edit=edit)


@pytest.mark.parametrize("fcode", [1, 3])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_video_packets(layout, fcode):
    """I-VOP and P-VOPs (the first all 4MV, so 4MV macroblocks stand on both sides of every
    boundary; then intra-in-P with AC prediction, 1MV, not-coded) cut into video packets."""
    st = packet_gop(3, 60 + fcode, layout, fcode)
    packets, lost, _ = LAYOUTS[layout]
    n_headers = sum(len(packets[k % len(packets)]) for k in range(4))
    assert st.stats["packets"] == n_headers
    assert st.stats["hec"] == sum(isinstance(e, tuple) and bool(e[1].get("hec")) for k in range(4)
                                  for e in packets[k % len(packets)])
    assert all(mb["ac_pred"] for mb in st.vops[0][1][1] if mb)           # AC prediction on across the boundaries
    assert {m["type"] for m in st.vops[1][1][1] if m} == {"inter4v"}
    host, parsed = check(st)
    for k, kinds in enumerate(_kinds(parsed)):
        gone = sorted(lost[k % len(lost)]) if lost else []
        assert np.flatnonzero(kinds == 3).tolist() == gone, f"VOP {k}"


def test_packet_after_a_byte_aligned_macroblock():
    """A macroblock that ends on a byte boundary is followed by a whole byte of stuffing (0x7f)
    before the resync marker; video_packet_header used to skip only to the next boundary and read
    the marker from the stuffing byte ("invalid TCOEF code" on this very stream)."""
    st = packet_gop(3, 61, "last_column", 1)
    assert st.stats["aligned_packets"] >= 1
    check(st)


def test_layouts_reach_every_packet_branch():
    """From the layouts alone: the packet start positions and first-packet-line shapes the case
    table claims."""
    starts = {name: {(n % MW, n // MW) for pk in spec[0] for n in (e if isinstance(e, int) else e[0] for e in pk)}
              for name, spec in LAYOUTS.items()}
    assert (1, 1) in starts["mid_row"]                                    # mid-row, rx == 1
    assert {(3, 0), (3, 1)} <= starts["last_column"]                      # last column, a row below it exists
    assert {(0, 1), (0, 2)} == starts["row_start"]
    assert {(1, 1), (2, 1)} <= starts["one_macroblock"] and {(1, 0), (2, 0)} <= starts["one_macroblock"]
    assert any(isinstance(e, tuple) and "q" in e[1] for pk in LAYOUTS["quant_scale"][0] for e in pk)
    assert any(isinstance(e, tuple) and e[1].get("hec") for pk in LAYOUTS["hec"][0] for e in pk)
    everywhere = set().union(*starts.values())
    assert any(0 < x < MW - 1 for x, _ in everywhere) and any(x == MW - 1 for x, _ in everywhere)
    assert any(x == 0 for x, _ in everywhere)
    # the DC-1024 packet start of packet_gop: block 2 predicts its AC from outside the packet
    for name in ("mid_row", "last_column", "row_start", "one_macroblock", "hec", "lost"):
        first = min(e if isinstance(e, int) else e[0] for e in LAYOUTS[name][0][0])
        mb = packet_gop(0, 61, name).vops[0][1][first // MW][first % MW]
        assert mb["blocks"][0, 0] * W.dc_scale(mb["q"], True) == 1024 and mb["ac_pred"], name


def test_lost_macroblocks_show_the_older_picture():
    """A gap in the first and second coded VOP is grey (no older picture exists), a gap in the
    third shows the first VOP's pixels: asserted on the host frames themselves, besides the
    restatement."""
    st = packet_gop(2, 62, "lost")
    host, parsed = check(st)
    y = [_planes(b, st.w, st.h)[0] for b in host]
    assert (y[0][16:32, 0:32] == 128).all()                               # macroblocks 4, 5 of the I-VOP
    assert (y[1][0:16, 16:48] == 128).all() and (y[1][32:48, 32:48] == 128).all()      # 1, 2 and 10 of the first P
    np.testing.assert_array_equal(y[2][16:32, 48:64], y[0][16:32, 48:64])  # 7 of the second P: two VOPs back
    np.testing.assert_array_equal(y[2][32:48, 0:16], y[0][32:48, 0:16])    # 8
    assert (y[0][16:32, 48:64] != 128).any()


# ------------------------------------------------------------------ intra_dc_vlc_thr
WALK = [0, 2, 2, -1, -2, -1, 2, 1, -2, 2, -1, -1]       # DQUANT of macroblocks 0..11, from threshold - 2


def dc_switch_gop(n_p, seed, code=3):
    """intra_dc_vlc_thr `code`: a QP walk across its threshold in both directions, in the I-VOP and
    in P-VOPs whose macroblocks are intra (DQUANT) or 4MV; flat macroblocks whose blocks code the
    DC alone, or nothing."""
    thr = W.DC_VLC_QP[code] or 12

    def qwalk(k, n, q):
        return q + WALK[n]

    def edit(k, mbs):
        if k == 1:
            return
        for n in (2, 6, 7):                # flat intra macroblocks: blocks 1-3 repeat block 0's DC
            mb = mbs[n // MW][n % MW]
            if mb["type"] != "intra":
                continue
            mb["blocks"][:, 1:] = 0
            mb["blocks"][1:4, 0] = mb["blocks"][0, 0]
            mb["ac_pred"] = False

    return gop(n_p, seed, q0=thr - 2, dc_thr=code, qwalk=qwalk, edit=edit, p_types=(["intra", "inter4v"], [0.8, 0.2]))


@pytest.mark.parametrize("code", [1, 2, 3, 4, 5, 6, 7])
def test_intra_dc_vlc_thr(code):
    st = dc_switch_gop(2, 70 + code, code)
    thr = W.DC_VLC_QP[code]
    qs = np.cumsum(WALK) + (thr or 12) - 2                     # the I-VOP's QP per macroblock
    before = np.concatenate([[qs[0]], qs[:-1]])               # the QP in force before each DQUANT
    assert [m["q"] for row in st.vops[0][1] for m in row] == qs.tolist()
    if code < 7:
        use = before < thr
        flips = np.diff(use.astype(int))
        assert (flips == 1).any() and (flips == -1).any()     # the walk crosses the threshold both ways
        assert ((qs < thr) != use).any()                      # and somewhere only the QP before DQUANT decides right
        assert st.stats["dc_vlc"] >= 6 * use.sum() and st.stats["dc_ac"] >= 6 * (~use).sum()
    else:
        assert st.stats["dc_vlc"] == 0
    assert st.stats["dc_ac_only"] and st.stats["dc_ac_uncoded"]
    assert any(m["type"] == "intra" for _, mbs, _, _ in st.vops[1:] for row in mbs for m in row)
    check(st)


# ------------------------------------------------------------------ header variants
VARIANTS = [dict(verid=2), dict(verid=5), dict(vbv=True), dict(par_extended=(4, 3)), dict(fixed_vop_rate=1),
            dict(object_layer_identifier=False), dict(verid=2, vbv=True, par_extended=(16, 11), fixed_vop_rate=7),
            dict(verid=2, quant_type=1, intra_matrix=MPEG_MATRICES["short"][0], inter_matrix=MPEG_MATRICES["short"][1])]


@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: "+".join(v))
def test_vol_header_variants_decode_alike(variant):
    """Every optional VOL field the parser steps over: the frames of the plain header."""
    base = {k: v for k, v in variant.items() if k in ("quant_type", "intra_matrix", "inter_matrix")}
    plain = gop(2, 80, **base)
    other = gop(2, 80, **variant)
    assert plain.samples == other.samples and plain.cfg != other.cfg
    for a, b in zip(_host_yuv(plain.cfg, plain.samples), check(other)[0]):
        np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------------ magnitudes
def magnitude_gop(n_p, seed):
    """QP 31 throughout.  Escape-3 levels that saturate to 2047 and -2048 (at most one per block
    row and column), an intra and an inter macroblock with all 384 coefficients, and inter
    residuals of +-2047 at the DC: the IDCT adds +-256 to every pixel, past both ends of clip8
    whatever the prediction."""
    rng = np.random.default_rng(seed)

    def edit(k, mbs):
        if k == 0:
            for row in mbs:
                for mb in row:
                    mb["blocks"][:, 1:] = 0
                    mb["ac_pred"] = False
            _spike(mbs[0][0], 0, 10, 2047)
            _spike(mbs[0][0], 1, 17, -2047)
            b = mbs[0][1]["blocks"]
            b[0, [9, 19, 26, 37]] = [300, -300, 40, -40]
            b[4, [12, 33]] = [-2047, 2047]
            full = mbs[1][1]["blocks"]
            full[:, 1:] = rng.choice([-1, 1], (6, 63))
            return
        for n, row in enumerate(mbs):
            for mb in row:
                mb["blocks"][:] = 0
        flat = [mb for row in mbs for mb in row]
        flat[0]["blocks"][:, 0] = [2047, -2047, 2047, -2047, -2047, 2047]
        flat[3]["blocks"][:, 0] = [-2047, 2047, -2047, 2047, 2047, -2047]
        flat[5]["blocks"][:] = rng.choice([-1, 1], (6, 64))
        flat[6]["blocks"][2, [10, 27]] = [2047, -2047]
        flat[9]["blocks"][:, 0] = 30

    inter = (["inter", "inter4v"], [0.5, 0.5])
    return gop(n_p, seed, q0=31, qwalk=lambda k, n, q: q, edit=edit, p_types=inter, mvmax=5)


def test_magnitudes():
    st = magnitude_gop(2, 90)
    assert st.stats["esc3"] >= 10
    lo = hi = 0
    for kind, mbs, _, _ in st.vops:
        for mb in (m for row in mbs for m in row):
            for n in range(6):
                intra = mb["type"] == "intra"
                d = W.dequant_h263(mb["blocks"][n], 31, intra, n < 4)
                lo += int((d[1 if intra else 0:] == -2048).sum())
                hi += int((d[1 if intra else 0:] == 2047).sum())
                if not intra and abs(int(mb["blocks"][n][0])) == 2047:
                    res = W.simple_idct(d, strict=True)
                    assert (res >= 256).all() or (res <= -256).all()     # clip8 on that side for any prediction
    assert lo >= 8 and hi >= 8
    host, parsed = check(st)
    for k, (rec, coef, _, _) in enumerate(parsed):
        nnz = rec.view(REC)["nnz"].sum(1)
        assert nnz.max() == 384 and nnz[5] == 384, f"VOP {k}"            # the parser's per-macroblock capacity
        values = (coef & 0xFFFF).astype(np.uint16).view(np.int16)
        assert (values == -2048).any() and (values == 2047).any()        # both extremes through the 16-bit packing
    for buf in host[1:]:
        y = _planes(buf, st.w, st.h)[0]
        assert (y[0:8, 0:8] == 255).all() and (y[0:8, 8:16] == 0).all()   # macroblock 0: +2047 and -2047 at the DC


# ------------------------------------------------------------------ dense, tiny
def dense_gop(n_p, seed):
    """Every macroblock of every VOP holds 384 non-zero coefficients (QP 2, +-1 levels)."""
    rng = np.random.default_rng(seed + 1000)

    def edit(k, mbs):
        for mb in (m for row in mbs for m in row):
            first = 1 if mb["type"] == "intra" else 0
            mb["blocks"][:, first:] = rng.choice([-1, 1], (6, 64 - first))
            mb["ac_pred"] = False

    return gop(n_p, seed, q0=2, qwalk=lambda k, n, q: q, edit=edit, p_types=(["inter", "inter4v"], [0.5, 0.5]))


def parse_many_done(st):
    """How many samples one mvp_mp4v_parse_many call takes when given decode_mp4v_device's buffer
    for the whole GOP (one worst-case sample + 24 entries per macroblock and sample)."""
    ps = video.Mp4vParser(st.cfg)
    try:
        n, nmb = len(st.samples), ps.n_mb
        ptrs = (ctypes.c_char_p * n)(*st.samples)
        sizes = np.array([len(x) for x in st.samples], np.uint64)
        rec = np.zeros(n * nmb * video.MB_REC_BYTES, np.uint8)
        ncoef, vops = np.zeros(n, np.int64), np.zeros((n, 2), np.int32)
        cap = nmb * 384 + n * nmb * 24
        buf = np.zeros(cap, np.uint32)
        done = ctypes.c_int()
        _lib.call("mvp_mp4v_parse_many", ps._h, n, ptrs, sizes.ctypes.data, rec.ctypes.data, buf.ctypes.data, cap,
                  ncoef.ctypes.data, vops.ctypes.data, ctypes.byref(done))
        return done.value, ncoef[:done.value]
    finally:
        ps.close()


def test_dense_gop_fills_every_macroblock_and_stops_parse_many_early():
    st = dense_gop(3, 95)
    host, parsed = check(st)
    for rec, coef, _, _ in parsed:
        assert (rec.view(REC)["nnz"] == 64).all() and coef.size == MW * MH * 384
    done, ncoef = parse_many_done(st)
    assert 1 <= done < len(st.samples) and (ncoef == MW * MH * 384).all()


def tiny_gop(n_p, seed, vol_wh=None):
    """One macroblock (mb_w == 1: every motion vector candidate beside and above it is off the
    grid), the first P-VOP 4MV; vol_wh: a VOL smaller than the macroblock."""
    return gop(n_p, seed, w_mb=1, h_mb=1, vol_wh=vol_wh, mvmax=12)


def test_one_macroblock_frame():
    st = tiny_gop(3, 96)
    assert st.vops[1][1][0][0]["type"] == "inter4v"
    check(st)


def test_vol_smaller_than_a_macroblock():
    """An 8 x 8 VOL: the records rebuild the host's pictures (vectors clamp at the visible edge,
    which W.reconstruct's macroblock-aligned planes do not model), and the I-VOP is the visible
    corner of the restated one."""
    st = tiny_gop(3, 97, vol_wh=(8, 8))
    host, _ = check(st, restatement=False)
    exp = W.reconstruct(16, 16, st.vops[:1])[0]
    for g, e in zip(_planes(host[0], 8, 8), exp):
        np.testing.assert_array_equal(g, e[:g.shape[0], :g.shape[1]])
