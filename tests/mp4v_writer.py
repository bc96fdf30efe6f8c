"""Test infrastructure: an MPEG-4 Part 2 Simple Profile bitstream WRITER and a numpy restatement
of the decoder's reconstruction (inverse quantisation, FFmpeg's simple IDCT, half-pel motion
compensation), for tests/test_mp4v.py.

The writer takes what a decoder must reconstruct — per macroblock the final quantised
coefficients, QP, motion vectors — and emits the VOL / VOP syntax of ISO/IEC 14496-2: intra DC
differentials against the DC prediction, AC prediction residuals, CBP, DQUANT, MV differences
against the median prediction, TCOEF events with their escapes.  Its VLC tables are a separate
transcription of the standard's (the decoder's live in csrc/mp4v_tables.h): a transcription error
on either side fails the round trip.  Prediction rules follow FFmpeg's mpeg4 decoder where the
standard leaves room (slice-edge DC predictors, MV prediction on the first row).

Beyond the plain stream it writes what a decoder claims to accept: MPEG quantisation with default,
loaded and short-list matrices (dequant_mpeg restates 7.4.4 with mismatch control), video packets
(resync marker, macroblock_number, quant_scale, header_extension_code) with the standard's
"outside the packet" predictor rules and macroblocks no packet holds, intra_dc_vlc_thr 1-7 (the
intra DC as the first TCOEF event), and the VOL header's optional fields.  Parity against cv2 /
FFmpeg stays unpinned: neither exists here.
"""
from __future__ import annotations

import collections

import numpy as np

# ------------------------------------------------------------------ tables (ISO/IEC 14496-2 annex B)
MCBPC_I = [(1, 1), (1, 3), (2, 3), (3, 3), (1, 4), (1, 6), (2, 6), (3, 6)]          # + 4 for dquant
MCBPC_P = {0: [(1, 1), (3, 4), (2, 4), (5, 6)],        # inter
           4: [(3, 5), (4, 8), (3, 8), (3, 7)],        # intra
           8: [(3, 3), (7, 7), (6, 7), (5, 9)],        # inter + q
           12: [(4, 6), (4, 9), (3, 9), (2, 9)],       # intra + q
           16: [(2, 3), (5, 7), (4, 7), (5, 8)]}       # inter4v
CBPY = [(3, 4), (5, 5), (4, 5), (9, 4), (3, 5), (7, 4), (2, 6), (11, 4),
        (2, 5), (3, 6), (5, 4), (10, 4), (4, 4), (8, 4), (6, 4), (3, 2)]
MVD = [(1, 1), (1, 2), (1, 3), (1, 4), (3, 6), (5, 7), (4, 7), (3, 7), (11, 9), (10, 9), (9, 9), (17, 10),
       (16, 10), (15, 10), (14, 10), (13, 10), (12, 10), (11, 10), (10, 10), (9, 10), (8, 10), (7, 10), (6, 10),
       (5, 10), (4, 10), (7, 11), (6, 11), (5, 11), (4, 11), (3, 11), (2, 11), (3, 12), (2, 12)]
DC_LUM = [(3, 3), (3, 2), (2, 2), (2, 3), (1, 3), (1, 4), (1, 5), (1, 6), (1, 7), (1, 8), (1, 9), (1, 10), (1, 11)]
DC_CHROM = [(3, 2), (2, 2), (1, 2), (1, 3), (1, 4), (1, 5), (1, 6), (1, 7), (1, 8), (1, 9), (1, 10), (1, 11),
            (1, 12)]
ESCAPE = (3, 7)

# TCOEF: {(last, run, level): (code, len)} — Table B-17 (inter) transcribed from the standard's
# (last, run, level) listing; Table B-16 (intra) uses the same codewords for other events.
_INTER_ROWS = [  # (last, run, [codes for level 1..])
    (0, 0, [(0x2, 2), (0xf, 4), (0x15, 6), (0x17, 7), (0x1f, 8), (0x25, 9), (0x24, 9), (0x21, 10), (0x20, 10),
            (0x7, 11), (0x6, 11), (0x20, 11)]),
    (0, 1, [(0x6, 3), (0x14, 6), (0x1e, 8), (0xf, 10), (0x21, 11), (0x50, 12)]),
    (0, 2, [(0xe, 4), (0x1d, 8), (0xe, 10), (0x51, 12)]),
    (0, 3, [(0xd, 5), (0x23, 9), (0xd, 10)]),
    (0, 4, [(0xc, 5), (0x22, 9), (0x52, 12)]),
    (0, 5, [(0xb, 5), (0xc, 10), (0x53, 12)]),
    (0, 6, [(0x13, 6), (0xb, 10), (0x54, 12)]),
    (0, 7, [(0x12, 6), (0xa, 10)]),
    (0, 8, [(0x11, 6), (0x9, 10)]),
    (0, 9, [(0x10, 6), (0x8, 10)]),
    (0, 10, [(0x16, 7), (0x55, 12)]),
] + [(0, r, [c]) for r, c in zip(range(11, 27), [(0x15, 7), (0x14, 7), (0x1c, 8), (0x1b, 8), (0x21, 9), (0x20, 9),
                                                  (0x1f, 9), (0x1e, 9), (0x1d, 9), (0x1c, 9), (0x1b, 9), (0x1a, 9),
                                                  (0x22, 11), (0x23, 11), (0x56, 12), (0x57, 12)])] + [
    (1, 0, [(0x7, 4), (0x19, 9), (0x5, 11)]),
    (1, 1, [(0xf, 6), (0x4, 11)]),
] + [(1, r, [c]) for r, c in zip(range(2, 41), [(0xe, 6), (0xd, 6), (0xc, 6), (0x13, 7), (0x12, 7), (0x11, 7),
                                                 (0x10, 7), (0x1a, 8), (0x19, 8), (0x18, 8), (0x17, 8), (0x16, 8),
                                                 (0x15, 8), (0x14, 8), (0x13, 8), (0x18, 9), (0x17, 9), (0x16, 9),
                                                 (0x15, 9), (0x14, 9), (0x13, 9), (0x12, 9), (0x11, 9), (0x7, 10),
                                                 (0x6, 10), (0x5, 10), (0x4, 10), (0x24, 11), (0x25, 11), (0x26, 11),
                                                 (0x27, 11), (0x58, 12), (0x59, 12), (0x5a, 12), (0x5b, 12),
                                                 (0x5c, 12), (0x5d, 12), (0x5e, 12), (0x5f, 12)])]
_INTRA_ROWS = [
    (0, 0, [(0x2, 2), (0x6, 3), (0xf, 4), (0xd, 5), (0xc, 5), (0x15, 6), (0x13, 6), (0x12, 6), (0x17, 7), (0x1f, 8),
            (0x1e, 8), (0x1d, 8), (0x25, 9), (0x24, 9), (0x23, 9), (0x21, 9), (0x21, 10), (0x20, 10), (0xf, 10),
            (0xe, 10), (0x7, 11), (0x6, 11), (0x20, 11), (0x21, 11), (0x50, 12), (0x51, 12), (0x52, 12)]),
    (0, 1, [(0xe, 4), (0x14, 6), (0x16, 7), (0x1c, 8), (0x20, 9), (0x1f, 9), (0xd, 10), (0x22, 11), (0x53, 12),
            (0x55, 12)]),
    (0, 2, [(0xb, 5), (0x15, 7), (0x1e, 9), (0xc, 10), (0x56, 12)]),
    (0, 3, [(0x11, 6), (0x1b, 8), (0x1d, 9), (0xb, 10)]),
    (0, 4, [(0x10, 6), (0x22, 9), (0xa, 10)]),
    (0, 5, [(0xd, 6), (0x1c, 9), (0x8, 10)]),
    (0, 6, [(0x12, 7), (0x1b, 9), (0x54, 12)]),
    (0, 7, [(0x14, 7), (0x1a, 9), (0x57, 12)]),
    (0, 8, [(0x19, 8), (0x9, 10)]),
    (0, 9, [(0x18, 8), (0x23, 11)]),
    (0, 10, [(0x17, 8)]), (0, 11, [(0x19, 9)]), (0, 12, [(0x18, 9)]), (0, 13, [(0x7, 10)]), (0, 14, [(0x58, 12)]),
    (1, 0, [(0x7, 4), (0xc, 6), (0x16, 8), (0x17, 9), (0x6, 10), (0x5, 11), (0x4, 11), (0x59, 12)]),
    (1, 1, [(0xf, 6), (0x16, 9), (0x5, 10)]),
    (1, 2, [(0xe, 6), (0x4, 10)]), (1, 3, [(0x11, 7), (0x24, 11)]), (1, 4, [(0x10, 7), (0x25, 11)]),
    (1, 5, [(0x13, 7), (0x5a, 12)]), (1, 6, [(0x15, 8), (0x5b, 12)]),
] + [(1, r, [c]) for r, c in zip(range(7, 21), [(0x14, 8), (0x13, 8), (0x1a, 8), (0x15, 9), (0x14, 9), (0x13, 9),
                                                 (0x12, 9), (0x11, 9), (0x26, 11), (0x27, 11), (0x5c, 12),
                                                 (0x5d, 12), (0x5e, 12), (0x5f, 12)])]


def _events(rows):
    return {(last, run, lev + 1): c for last, run, codes in rows for lev, c in enumerate(codes)}


TCOEF = {True: _events(_INTRA_ROWS), False: _events(_INTER_ROWS)}
LMAX = {t: {} for t in (True, False)}
RMAX = {t: {} for t in (True, False)}
for _t, _ev in TCOEF.items():
    for (_last, _run, _lev) in _ev:
        LMAX[_t][(_last, _run)] = max(LMAX[_t].get((_last, _run), 0), _lev)
        RMAX[_t][(_last, _lev)] = max(RMAX[_t].get((_last, _lev), 0), _run)

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20,
                   13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52,
                   45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
ALT_H = np.array([0, 1, 2, 3, 8, 9, 16, 17, 10, 11, 4, 5, 6, 7, 15, 14, 13, 12, 19, 18, 24, 25, 32, 33, 26, 27, 20,
                  21, 22, 23, 28, 29, 30, 31, 34, 35, 40, 41, 48, 49, 42, 43, 36, 37, 38, 39, 44, 45, 46, 47, 50,
                  51, 56, 57, 58, 59, 52, 53, 54, 55, 60, 61, 62, 63])
ALT_V = (ALT_H % 8) * 8 + ALT_H // 8


def dc_scale(q, luma):
    if luma:
        return 8 if q < 5 else 2 * q if q < 9 else q + 8 if q < 25 else 2 * q - 16
    return 8 if q < 5 else (q + 13) // 2 if q < 25 else q - 6


# ------------------------------------------------------------------ bits
class BitWriter:
    def __init__(self):
        self.bits = []

    def put(self, value, n):
        for i in range(n - 1, -1, -1):
            self.bits.append((value >> i) & 1)

    def code(self, c):
        self.put(*c)

    def stuff(self):
        """MPEG-4 next_start_code stuffing: a 0, then 1s to the byte boundary."""
        self.bits.append(0)
        while len(self.bits) % 8:
            self.bits.append(1)

    def start_code(self, code):
        assert len(self.bits) % 8 == 0
        self.put(0x000001, 24)
        self.put(code, 8)

    def tobytes(self):
        b = self.bits + [0] * (-len(self.bits) % 8)
        return np.packbits(np.array(b, np.uint8)).tobytes()


# Default quantisation matrices (ISO/IEC 14496-2 6.3.2, raster), typed from the standard's listing.
DEFAULT_INTRA_MATRIX = np.array([
    8, 17, 18, 19, 21, 23, 25, 27,
    17, 18, 19, 21, 23, 25, 27, 28,
    20, 21, 22, 23, 24, 26, 28, 30,
    21, 22, 23, 24, 26, 28, 30, 32,
    22, 23, 24, 26, 28, 30, 32, 35,
    23, 24, 26, 28, 30, 32, 35, 38,
    25, 26, 28, 30, 32, 35, 38, 41,
    27, 28, 30, 32, 35, 38, 41, 45], np.int64)
DEFAULT_INTER_MATRIX = np.array([
    16, 17, 18, 19, 20, 21, 22, 23,
    17, 18, 19, 20, 21, 22, 23, 24,
    18, 19, 20, 21, 22, 23, 24, 25,
    19, 20, 21, 22, 23, 24, 26, 27,
    20, 21, 22, 23, 25, 26, 27, 28,
    21, 22, 23, 24, 26, 27, 28, 30,
    22, 23, 24, 26, 27, 28, 30, 31,
    23, 24, 25, 27, 28, 30, 31, 33], np.int64)


def expand_matrix(m, default=None):
    """The 64 raster weights a decoder holds after loading `m`: a full 64-entry raster matrix, or
    the short-list form (fewer than 64 values in zigzag order; the stream ends them with a 0 and
    the remaining zigzag positions repeat the last value).  None: `default`."""
    if m is None:
        return default
    a = np.asarray(m, np.int64).reshape(-1)
    if a.size == 64:
        return a
    assert 0 < a.size < 64
    out = np.empty(64, np.int64)
    out[ZIGZAG[:a.size]] = a
    out[ZIGZAG[a.size:]] = a[-1]
    return out


def _put_matrix(bw, m):
    if m is None:
        bw.put(0, 1)              # load_*_quant_mat = 0: the default matrix
        return
    bw.put(1, 1)
    a = np.asarray(m, np.int64).reshape(-1)
    vals = a[ZIGZAG] if a.size == 64 else a
    for v in vals:
        assert 1 <= v <= 255, v
        bw.put(int(v), 8)
    if a.size < 64:
        bw.put(0, 8)              # ends the list: the rest repeat the last value


def vol_header(w, h, quant_type=0, resync_disable=1, time_res=30, intra_matrix=None, inter_matrix=None, verid=1,
               vbv=False, par_extended=None, fixed_vop_rate=None, object_layer_identifier=True):
    """VOS + VO + VOL headers as FFmpeg's mpeg4 encoder writes them (object layer id, vol control
    parameters, rectangular, progressive, 8-bit), and the header variants a decoder must step
    over: verid 2 / 5 (2-bit sprite_enable, quarter_sample, newpred_enable and
    reduced_resolution_vop_enable, all 0), the 79-bit VBV block, an extended pixel aspect ratio
    (par_extended=(w, h)), fixed_vop_rate (fixed_vop_time_increment = the value given), no
    object layer identifier (the version is then 1), loaded quantisation matrices (quant_type 1:
    64 raster values, or the short-list form of expand_matrix)."""
    assert object_layer_identifier or verid == 1
    bw = BitWriter()
    bw.start_code(0xB0)
    bw.put(1, 8)                  # profile_and_level_indication: simple L1
    bw.start_code(0xB5)
    bw.put(0, 1)                  # is_visual_object_identifier
    bw.put(1, 4)                  # visual_object_type: video
    bw.put(0, 1)                  # video_signal_type
    bw.stuff()
    bw.start_code(0x00)           # video_object_start_code
    bw.start_code(0x20)           # video_object_layer_start_code
    bw.put(0, 1)
    bw.put(1, 8)                  # simple object
    if object_layer_identifier:
        bw.put(1, 1)              # is_object_layer_identifier
        bw.put(verid, 4)
        bw.put(1, 3)
    else:
        bw.put(0, 1)
    if par_extended is None:
        bw.put(1, 4)              # aspect ratio 1:1
    else:
        bw.put(15, 4)             # extended_PAR
        bw.put(par_extended[0], 8)
        bw.put(par_extended[1], 8)
    bw.put(1, 1)                  # vol_control_parameters
    bw.put(1, 2)                  # 4:2:0
    bw.put(1, 1)                  # low_delay
    if vbv:
        bw.put(1, 1)              # vbv_parameters: 79 bits, markers included
        for value, n in ((0x155, 15), (0x2AAA, 15), (0x1234, 15)):   # bit rate halves, first buffer half
            bw.put(value, n)
            bw.put(1, 1)
        bw.put(5, 3)              # latter_half_vbv_buffer_size
        bw.put(0x2AA, 11)         # first_half_vbv_occupancy
        bw.put(1, 1)
        bw.put(0x5555, 15)        # latter_half_vbv_occupancy
        bw.put(1, 1)
    else:
        bw.put(0, 1)
    bw.put(0, 2)                  # rectangular
    bw.put(1, 1)
    bw.put(time_res, 16)
    bw.put(1, 1)
    if fixed_vop_rate is None:
        bw.put(0, 1)
    else:
        bw.put(1, 1)              # fixed_vop_rate
        bw.put(fixed_vop_rate, time_bits(time_res))
    bw.put(1, 1)
    bw.put(w, 13)
    bw.put(1, 1)
    bw.put(h, 13)
    bw.put(1, 1)
    bw.put(0, 1)                  # interlaced
    bw.put(1, 1)                  # obmc_disable
    bw.put(0, 1 if verid == 1 else 2)   # sprite_enable
    bw.put(0, 1)                  # not_8_bit
    bw.put(quant_type, 1)
    if quant_type:
        _put_matrix(bw, intra_matrix)
        _put_matrix(bw, inter_matrix)
    else:
        assert intra_matrix is None and inter_matrix is None
    if verid != 1:
        bw.put(0, 1)              # quarter_sample
    bw.put(1, 1)                  # complexity_estimation_disable
    bw.put(resync_disable, 1)
    bw.put(0, 1)                  # data_partitioned
    if verid != 1:
        bw.put(0, 1)              # newpred_enable
        bw.put(0, 1)              # reduced_resolution_vop_enable
    bw.put(0, 1)                  # scalability
    bw.stuff()
    return bw.tobytes()


def time_bits(res):
    return max(1, int(res - 1).bit_length())


# ------------------------------------------------------------------ VOP writer
# intra_dc_vlc_thr (Table 6-21): the intra DC uses the dct_dc_size VLC while the running QP is below
# this value; code 0 always does, code 7 never.
DC_VLC_QP = [99, 13, 15, 17, 19, 21, 23, 0]


class VopWriter:
    """Writes I / P VOPs of w x h (multiples of 16) and tracks the predictor state a decoder
    builds, so every prediction residual it writes is against the decoder's predictor.

    Video packets: `packets` lists the macroblock numbers at which a packet starts (n, or
    (n, {"q": quant_scale, "hec": True})).  A macroblock given as None is lost: it is written
    nowhere, and the next written macroblock must start a packet.  Predictors follow the
    standard's rule, stated per candidate instead of FFmpeg's first-slice-line bookkeeping: a
    candidate block is usable only inside the picture and inside the current video packet.  An
    unusable A / B / C gives DC 1024 and AC 0 (7.4.3.3); of the three motion vector candidates,
    one unusable counts as zero, two unusable take the third's value, three give zero (7.6.5)."""

    def __init__(self, w, h, time_res=30):
        self.w, self.h = w, h
        self.mw, self.mh = w // 16, h // 16
        self.tb = time_bits(time_res)
        self.n = 0
        # what the written syntax contained, for tests that assert a path was reached: "packets"
        # (headers written; "aligned_packets" of them after a macroblock that ended on a byte
        # boundary), "hec", intra blocks by DC coding ("dc_vlc"; through the AC VLC: "dc_ac",
        # of which "dc_ac_only" hold the DC event alone and "dc_ac_uncoded" nothing), TCOEF events
        # by escape type ("esc1" / "esc2" / "esc3")
        self.stats = collections.Counter()

    # --- predictor state: luma per 8x8 block, chroma per macroblock, one border entry left / top
    def _reset(self):
        mw, mh = self.mw, self.mh
        self.dc = [np.full((2 * mh + 1, 2 * mw + 2), 1024, np.int64)] + [np.full((mh + 1, mw + 2), 1024, np.int64)
                                                                       for _ in range(2)]
        self.ac = [np.zeros((2 * mh + 1, 2 * mw + 2, 16), np.int64)] + [np.zeros((mh + 1, mw + 2, 16), np.int64)
                                                                      for _ in range(2)]
        self.mv = np.zeros((2 * mh + 1, 2 * mw + 2, 2), np.int64)
        self.mbq = np.zeros((mh + 1, mw + 2), np.int64)
        self.pkt = np.full((mh, mw), -1, np.int64)     # the video packet each macroblock was written in
        self.cur_pkt = 0

    def _usable(self, mx, my):
        return 0 <= mx < self.mw and 0 <= my < self.mh and self.pkt[my, mx] == self.cur_pkt

    def _pos(self, n, x, y):
        if n < 4:
            return 0, 2 * y + (n >> 1) + 1, 2 * x + (n & 1) + 1
        return n - 3, y + 1, x + 1

    def _neighbours(self, n, x, y):
        """Block n's A (left), B (above-left), C (above): (usable, plane, row, column, mb_x, mb_y)."""
        p, r, c = self._pos(n, x, y)
        out = []
        for dr, dc_ in ((0, -1), (-1, -1), (-1, 0)):
            rr, cc = r + dr, c + dc_
            mx, my = ((cc - 1) >> 1, (rr - 1) >> 1) if n < 4 else (cc - 1, rr - 1)
            out.append((self._usable(mx, my), p, rr, cc, mx, my))
        return out

    def _pred_dc(self, n, x, y, q):
        a, b, cc = (int(self.dc[p][r, c]) if ok else 1024 for ok, p, r, c, _, _ in self._neighbours(n, x, y))
        if abs(a - b) < abs(b - cc):
            pred, direction = cc, 1
        else:
            pred, direction = a, 0
        s = dc_scale(q, n < 4)
        return (pred + (s >> 1)) // s, direction

    def _ac_pred_values(self, n, x, y, q, direction):
        """The predicted first column (direction 0) or first row (1), quantised domain."""
        ok, p, r, c, mx, my = self._neighbours(n, x, y)[0 if direction == 0 else 2]
        out = np.zeros(8, np.int64)
        if not ok:
            return out
        src = self.ac[p][r, c][:8] if direction == 0 else self.ac[p][r, c][8:]
        qn = q if (mx, my) == (x, y) else int(self.mbq[my + 1, mx + 1])
        for i in range(1, 8):
            out[i] = src[i] if qn == q else _rdiv(src[i] * qn, q)
        return out

    def _store_intra(self, n, x, y, q, blk):
        p, r, c = self._pos(n, x, y)
        level = int(blk[0]) * dc_scale(q, n < 4)
        if level & ~2047:
            level = 0 if level < 0 else 2047
        self.dc[p][r, c] = level
        a = self.ac[p][r, c]
        a[:] = 0
        for i in range(1, 8):
            a[i] = blk[i * 8]
            a[8 + i] = blk[i]

    def _clear_intra(self, x, y):
        for n in range(6):
            p, r, c = self._pos(n, x, y)
            self.dc[p][r, c] = 1024
            self.ac[p][r, c] = 0

    # --- syntax
    def _time(self, bw):
        bw.put(0, 1)               # modulo_time_base
        bw.put(1, 1)
        bw.put(self.time, self.tb)
        bw.put(1, 1)

    def _header(self, bw, vtype, q, rounding=0, fcode=1, dc_thr=0):
        assert 0 <= dc_thr <= 7 and 1 <= q <= 31
        bw.start_code(0xB6)
        bw.put(vtype, 2)
        self.time = self.n % (1 << self.tb)
        self._time(bw)
        bw.put(1, 1)               # vop_coded
        if vtype == 1:
            bw.put(rounding, 1)
        bw.put(dc_thr, 3)          # intra_dc_vlc_thr
        bw.put(q, 5)
        if vtype == 1:
            bw.put(fcode, 3)
        self.n += 1
        self.vtype, self.fcode, self.dc_thr, self.q = vtype, fcode, dc_thr, q

    def _packet_starts(self, mbs, packets):
        starts = {}
        for e in packets or ():
            n, opt = (e, {}) if isinstance(e, (int, np.integer)) else e
            assert 0 < n < self.mw * self.mh and int(n) not in starts, n
            starts[int(n)] = opt
        flat = [mb for row in mbs for mb in row]
        assert flat[0] is not None and flat[-1] is not None, "lost macroblocks lie between two packets"
        for n in range(1, len(flat)):
            assert flat[n] is not None or n not in starts
            assert not (flat[n - 1] is None and flat[n] is not None) or n in starts, "a packet starts after a gap"
        return starts

    def _begin_mb(self, bw, mbs, x, y, starts):
        """The video packet header, when a packet starts at macroblock (x, y); False: the macroblock is lost."""
        if mbs[y][x] is None:
            return False
        n = y * self.mw + x
        if n in starts:
            opt = starts[n]
            self.stats["aligned_packets"] += len(bw.bits) % 8 == 0           # the stuffing is then a whole byte
            bw.stuff()                                                   # next_resync_marker
            bw.put(0, 16 + (self.fcode - 1 if self.vtype == 1 else 0))      # resync_marker: zeros, then a one
            bw.put(1, 1)
            bw.put(n, max(1, (self.mw * self.mh - 1).bit_length()))        # macroblock_number
            self.q = int(opt.get("q", self.q))
            bw.put(self.q, 5)                                              # quant_scale
            hec = bool(opt.get("hec", False))
            bw.put(int(hec), 1)                                            # header_extension_code
            if hec:
                self._time(bw)
                bw.put(self.vtype, 2)
                bw.put(self.dc_thr, 3)
                if self.vtype == 1:
                    bw.put(self.fcode, 3)
            self.cur_pkt += 1
            self.stats["packets"] += 1
            self.stats["hec"] += hec
        self.pkt[y, x] = self.cur_pkt
        return True

    def _tcoef(self, bw, coefs, intra):
        """coefs: (run, level) pairs in scan order, the last flagged implicitly."""
        ev = TCOEF[intra]
        for k, (run, level) in enumerate(coefs):
            last = int(k == len(coefs) - 1)
            a, s = abs(level), int(level < 0)
            if (last, run, a) in ev:
                bw.code(ev[(last, run, a)])
                bw.put(s, 1)
                continue
            lm = LMAX[intra].get((last, run), 0)
            if lm and (last, run, a - lm) in ev:              # escape type 1
                self.stats["esc1"] += 1
                bw.code(ESCAPE)
                bw.put(0, 1)
                bw.code(ev[(last, run, a - lm)])
                bw.put(s, 1)
                continue
            rm = RMAX[intra].get((last, a), None)
            if rm is not None and (last, run - rm - 1, a) in ev:  # escape type 2
                self.stats["esc2"] += 1
                bw.code(ESCAPE)
                bw.put(2, 2)
                bw.code(ev[(last, run - rm - 1, a)])
                bw.put(s, 1)
                continue
            assert -2048 < level < 2048, level
            self.stats["esc3"] += 1
            bw.code(ESCAPE)                                  # type 3
            bw.put(3, 2)
            bw.put(last, 1)
            bw.put(run, 6)
            bw.put(1, 1)
            bw.put(level & 0xFFF, 12)
            bw.put(1, 1)

    @staticmethod
    def _runs(blk, scan, start):
        out, run = [], 0
        for i in range(start, 64):
            v = int(blk[scan[i]])
            if v == 0:
                run += 1
            else:
                out.append((run, v))
                run = 0
        return out

    def _intra_mb(self, x, y, mb, q, use_dc_vlc):
        """mb: {"blocks": (6, 64) final quantised coefficients (raster), "ac_pred": bool}; q: the
        macroblock's QP (after its DQUANT).  Without the DC VLC the DC differential is the event
        at scan position 0 of the block's TCOEF list."""
        blocks = np.asarray(mb["blocks"], np.int64).reshape(6, 64)
        ac_pred = bool(mb.get("ac_pred", False))
        trans, dcs = [], []
        for n in range(6):
            pred, direction = self._pred_dc(n, x, y, q)
            blk = blocks[n].copy()
            t = blk.copy()
            if ac_pred:
                pv = self._ac_pred_values(n, x, y, q, direction)
                if direction == 0:
                    for i in range(1, 8):
                        t[i * 8] -= pv[i]
                else:
                    for i in range(1, 8):
                        t[i] -= pv[i]
            scan = (ALT_V if direction == 0 else ALT_H) if ac_pred else ZIGZAG
            t[0] = int(blk[0]) - pred
            dcs.append(int(t[0]))
            trans.append(self._runs(t, scan, 1 if use_dc_vlc else 0))
            self.stats["dc_vlc" if use_dc_vlc else "dc_ac"] += 1
            if not use_dc_vlc:
                self.stats["dc_ac_only"] += bool(t[0]) and len(trans[-1]) == 1
                self.stats["dc_ac_uncoded"] += not trans[-1]
            self._store_intra(n, x, y, q, blk)
        cbp = sum(1 << (5 - n) for n in range(6) if trans[n])
        return ac_pred, cbp, dcs, trans

    def _write_intra_blocks(self, bw, dcs, trans, use_dc_vlc=True):
        for n in range(6):
            if use_dc_vlc:
                d = dcs[n]
                size = abs(d).bit_length()
                assert size <= 12, d
                bw.code((DC_LUM if n < 4 else DC_CHROM)[size])
                if size:
                    bw.put(d if d > 0 else d + (1 << size) - 1, size)
                    if size > 8:
                        bw.put(1, 1)
            if trans[n]:
                self._tcoef(bw, trans[n], True)

    def _intra_syntax(self, bw, x, y, mb, p_vop):
        """One intra macroblock, header and blocks; the DC VLC switch looks at the QP in force
        before this macroblock's DQUANT."""
        q = self.q
        qn = mb.get("q", q)
        dq = qn - q
        assert dq in (0, -1, -2, 1, 2), (q, qn)
        use_dc_vlc = q < DC_VLC_QP[self.dc_thr]
        self.mbq[y + 1, x + 1] = qn
        ac_pred, cbp, dcs, trans = self._intra_mb(x, y, mb, qn, use_dc_vlc)
        if p_vop:
            bw.code(MCBPC_P[12 if dq else 4][cbp & 3])
        else:
            bw.code(MCBPC_I[(cbp & 3) + (4 if dq else 0)])
        bw.put(int(ac_pred), 1)
        bw.code(CBPY[cbp >> 2])
        if dq:
            bw.put({-1: 0, -2: 1, 1: 2, 2: 3}[dq], 2)
        self.q = qn
        self._write_intra_blocks(bw, dcs, trans, use_dc_vlc)

    def i_vop(self, mbs, q0, dc_thr=0, packets=None):
        """mbs[y][x] = {"q": QP (within 2 of the previous MB's), "blocks": (6, 64), "ac_pred": bool},
        or None for a lost macroblock."""
        self._reset()
        bw = BitWriter()
        self._header(bw, 0, q0, dc_thr=dc_thr)
        starts = self._packet_starts(mbs, packets)
        for y in range(self.mh):
            for x in range(self.mw):
                if self._begin_mb(bw, mbs, x, y, starts):
                    self._intra_syntax(bw, x, y, mbs[y][x], False)
        bw.stuff()
        return bw.tobytes()

    # --- motion vectors
    def _mvslot(self, x, y, k):
        return 2 * y + (k >> 1) + 1, 2 * x + (k & 1) + 1

    def _pred_mv(self, x, y, k):
        """Median of the candidates left, above and above-right (above-left for block 3) of luma
        block k.  With a picture one macroblock wide, a row below the first has two unusable
        candidates (left, above-right): the standard's rule above gives the third's value there,
        FFmpeg's border zeros give the median (0, B, 0) = 0; no test stream reaches that case."""
        off = {0: 2, 1: 1, 2: 1, 3: -1}[k]
        r, c = self._mvslot(x, y, k)
        cand = []
        for rr, cc in ((r, c - 1), (r - 1, c), (r - 1, c + off)):
            ok = self._usable((cc - 1) >> 1, (rr - 1) >> 1)
            cand.append((int(self.mv[rr, cc, 0]), int(self.mv[rr, cc, 1])) if ok else None)
        good = [v for v in cand if v is not None]
        if not good:
            return 0, 0
        if len(good) == 1:
            return good[0]
        cand = [v or (0, 0) for v in cand]
        return tuple(sorted(v[i] for v in cand)[1] for i in range(2))

    @staticmethod
    def _mvd(bw, diff, fcode):
        shift = fcode - 1
        rng = 32 << shift
        diff = ((diff + rng) % (2 * rng)) - rng    # wrap into the representable range
        if diff == 0:
            bw.code(MVD[0])
            return
        a = abs(diff) - 1
        code = (a >> shift) + 1
        bw.code(MVD[code])
        bw.put(int(diff < 0), 1)
        if shift:
            bw.put(a & ((1 << shift) - 1), shift)

    def p_vop(self, mbs, q0, rounding=0, fcode=1, dc_thr=0, packets=None):
        """mbs[y][x] = {"type": "skip"} | {"type": "inter", "mv": (x, y)} |
        {"type": "inter4v", "mvs": [(x, y)] * 4} | {"type": "intra", ...i_vop fields} | None (lost);
        inter types take "q" and "blocks" (6, 64) quantised residual coefficients (raster)."""
        self._reset()
        bw = BitWriter()
        self._header(bw, 1, q0, rounding, fcode, dc_thr)
        starts = self._packet_starts(mbs, packets)
        for y in range(self.mh):
            for x in range(self.mw):
                if not self._begin_mb(bw, mbs, x, y, starts):
                    continue
                mb = mbs[y][x]
                t = mb["type"]
                q = self.q
                if t == "skip":
                    bw.put(1, 1)
                    self._clear_intra(x, y)
                    for k in range(4):
                        self.mv[self._mvslot(x, y, k)] = 0
                    self.mbq[y + 1, x + 1] = q
                    continue
                bw.put(0, 1)
                if t == "intra":
                    for k in range(4):
                        self.mv[self._mvslot(x, y, k)] = 0
                    self._intra_syntax(bw, x, y, mb, True)
                    continue
                qn = mb.get("q", q)
                dq = qn - q
                assert dq in (0, -1, -2, 1, 2), (q, qn)
                self._clear_intra(x, y)
                blocks = np.asarray(mb.get("blocks", np.zeros((6, 64))), np.int64).reshape(6, 64)
                trans = [self._runs(blocks[n], ZIGZAG, 0) for n in range(6)]
                cbp = sum(1 << (5 - n) for n in range(6) if trans[n])
                four = t == "inter4v"
                assert not (four and dq), "inter4v + q is not Simple Profile"
                bw.code(MCBPC_P[(16 if four else 8 if dq else 0)][cbp & 3])
                bw.code(CBPY[15 - (cbp >> 2)])
                if dq:
                    bw.put({-1: 0, -2: 1, 1: 2, 2: 3}[dq], 2)
                self.q = qn
                self.mbq[y + 1, x + 1] = qn
                mvs = mb["mvs"] if four else [mb["mv"]] * 4
                for k in range(4 if four else 1):
                    px, py = self._pred_mv(x, y, k)
                    self._mvd(bw, mvs[k][0] - px, fcode)
                    self._mvd(bw, mvs[k][1] - py, fcode)
                    if four:
                        self.mv[self._mvslot(x, y, k)] = mvs[k]
                if not four:
                    for k in range(4):
                        self.mv[self._mvslot(x, y, k)] = mvs[0]
                for n in range(6):
                    if trans[n]:
                        self._tcoef(bw, trans[n], False)
        bw.stuff()
        return bw.tobytes()


def _rdiv(a, b):
    a, b = int(a), int(b)
    return int((a + (b >> 1)) // b) if a >= 0 else -int((-a + (b >> 1)) // b)


# ------------------------------------------------------------------ reconstruction restated
W1, W2, W3, W4, W5, W6, W7 = 22725, 21407, 19266, 16383, 12873, 8867, 4520


def _fits(values, bits, what):
    lim = 1 << (bits - 1)
    for v in values:
        assert -lim <= int(v) < lim, f"simple IDCT: {what} {int(v)} leaves int{bits}"


def simple_idct(blk, strict=False):
    """FFmpeg's simple IDCT (8-bit), restated in numpy int64: rows (DC-only shortcut x 8, else
    shift 11 with rounding), then columns (shift 20, W4 x (c0 + 32) rounding).  The C versions
    accumulate in int32 and store the row pass as int16; strict=True asserts that these inputs
    stay inside both (every running sum, every row-pass output), so that the int64 result is
    what any such implementation computes without relying on wrap-around."""
    b = np.asarray(blk, np.int64).reshape(8, 8).copy()
    for r in range(8):
        x = b[r]
        if not x[1:].any():
            if strict:
                _fits([int(x[0]) * 8], 16, "row DC")
            v = (int(x[0]) * 8) & 0xFFFF          # the DC-only shortcut, stored as int16
            b[r] = v - 65536 if v >= 32768 else v
            continue
        acc = []
        a0 = W4 * x[0] + (1 << 10)
        a1, a2, a3 = a0, a0, a0
        a0, a1, a2, a3 = a0 + W2 * x[2], a1 + W6 * x[2], a2 - W6 * x[2], a3 - W2 * x[2]
        b0 = W1 * x[1] + W3 * x[3]
        b1 = W3 * x[1] - W7 * x[3]
        b2 = W5 * x[1] - W1 * x[3]
        b3 = W7 * x[1] - W5 * x[3]
        acc += [a0, a1, a2, a3, b0, b1, b2, b3, W1 * x[1], W3 * x[1], W5 * x[1], W7 * x[1]]
        a0 += W4 * x[4]
        a1 += -W4 * x[4]
        a2 += -W4 * x[4]
        a3 += W4 * x[4]
        b0 += W5 * x[5]
        b1 += -W1 * x[5]
        b2 += W7 * x[5]
        b3 += W3 * x[5]
        acc += [a0, a1, a2, a3, b0, b1, b2, b3, W4 * x[4] + W6 * x[6], -W4 * x[4] - W2 * x[6], -W4 * x[4] + W2 * x[6],
                W4 * x[4] - W6 * x[6], W5 * x[5] + W7 * x[7], -W1 * x[5] - W5 * x[7], W7 * x[5] + W3 * x[7],
                W3 * x[5] - W1 * x[7]]
        a0 += W6 * x[6]
        a1 += -W2 * x[6]
        a2 += W2 * x[6]
        a3 += -W6 * x[6]
        b0 += W7 * x[7]
        b1 += -W5 * x[7]
        b2 += W3 * x[7]
        b3 += -W1 * x[7]
        full = np.array([a0 + b0, a1 + b1, a2 + b2, a3 + b3, a3 - b3, a2 - b2, a1 - b1, a0 - b0], np.int64)
        row = full >> 11
        if strict:
            _fits(acc + [a0, a1, a2, a3, b0, b1, b2, b3] + list(full), 32, "row accumulator")
            _fits(row, 16, "row output")
        b[r] = ((row + 32768) & 0xFFFF) - 32768   # int16 storage
    out = np.empty((8, 8), np.int64)
    for c in range(8):
        x = b[:, c]
        acc = []
        a0 = W4 * (x[0] + ((1 << 19) // W4))
        a1, a2, a3 = a0, a0, a0
        a0, a1, a2, a3 = a0 + W2 * x[2], a1 + W6 * x[2], a2 - W6 * x[2], a3 - W2 * x[2]
        b0 = W1 * x[1] + W3 * x[3]
        b1 = W3 * x[1] - W7 * x[3]
        b2 = W5 * x[1] - W1 * x[3]
        b3 = W7 * x[1] - W5 * x[3]
        acc += [a0, a1, a2, a3, b0, b1, b2, b3, W1 * x[1], W3 * x[1], W5 * x[1], W7 * x[1]]
        a0, a1, a2, a3 = a0 + W4 * x[4], a1 - W4 * x[4], a2 - W4 * x[4], a3 + W4 * x[4]
        b0, b1, b2, b3 = b0 + W5 * x[5], b1 - W1 * x[5], b2 + W7 * x[5], b3 + W3 * x[5]
        acc += [a0, a1, a2, a3, b0, b1, b2, b3]
        a0, a1, a2, a3 = a0 + W6 * x[6], a1 - W2 * x[6], a2 + W2 * x[6], a3 - W6 * x[6]
        b0, b1, b2, b3 = b0 + W7 * x[7], b1 - W5 * x[7], b2 + W3 * x[7], b3 - W1 * x[7]
        full = np.array([a0 + b0, a1 + b1, a2 + b2, a3 + b3, a3 - b3, a2 - b2, a1 - b1, a0 - b0])
        if strict:
            _fits(acc + [a0, a1, a2, a3, b0, b1, b2, b3] + list(full), 32, "column accumulator")
        out[:, c] = full >> 20
    return out


def float_idct(blk):
    """The separable 8x8 inverse DCT in float64 (IEEE 1180 reference)."""
    k = np.arange(8)
    cu = np.where(k == 0, np.sqrt(0.125), 0.5)
    basis = cu[:, None] * np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16)   # [u, x]
    return basis.T @ np.asarray(blk, np.float64).reshape(8, 8) @ basis


def dequant_h263(blk, q, intra, luma=True):
    b = np.asarray(blk, np.int64).reshape(64).copy()
    qmul, qadd = 2 * q, (q - 1) | 1
    start = 1 if intra else 0
    for i in range(start, 64):
        v = b[i]
        if v:
            b[i] = max(-2048, min(2047, v * qmul - qadd if v < 0 else v * qmul + qadd))
    if intra:
        b[0] = b[0] * dc_scale(q, luma)
    return b


def dequant_mpeg(blk, q, intra, luma, matrix, mismatch=True):
    """MPEG-type inverse quantisation (7.4.4.1) of the quantised raster block `blk` with the 64
    raster weights `matrix`: intra AC (2 |l| q W) // 16 and inter ((2 |l| + 1) q W) // 16 with the
    sign restored, saturated to [-2048, 2047]; the intra DC is level x dc_scaler; then mismatch
    control: an even sum of all 64 reconstructed coefficients toggles the LSB of coefficient 63."""
    b = np.asarray(blk, np.int64).reshape(64).copy()
    wgt = np.asarray(matrix, np.int64).reshape(64)
    for i in range(1 if intra else 0, 64):
        v = int(b[i])
        if v:
            a = (2 * abs(v) * q * int(wgt[i])) // 16 if intra else ((2 * abs(v) + 1) * q * int(wgt[i])) // 16
            b[i] = max(-2048, min(2047, -a if v < 0 else a))
    if intra:
        b[0] = b[0] * dc_scale(q, luma)
    if mismatch and int(b.sum()) % 2 == 0:
        b[63] ^= 1
    return b


def mc_plane(ref, x0, y0, w, h, mvx, mvy, rnd):
    """Half-pel prediction of a w x h block at (x0, y0) with edge clamping (unrestricted MVs)."""
    H, W = ref.shape
    sx, sy = x0 + (mvx >> 1), y0 + (mvy >> 1)
    ys = np.clip(np.arange(sy, sy + h + 1), 0, H - 1)
    xs = np.clip(np.arange(sx, sx + w + 1), 0, W - 1)
    p = ref[np.ix_(ys, xs)].astype(np.int64)
    a, b, c, d = p[:-1, :-1], p[:-1, 1:], p[1:, :-1], p[1:, 1:]
    hx, hy = mvx & 1, mvy & 1
    if not hx and not hy:
        return a
    if hx and not hy:
        return (a + b + 1 - rnd) >> 1
    if hy and not hx:
        return (a + c + 1 - rnd) >> 1
    return (a + b + c + d + 2 - rnd) >> 2


def chroma_mv(v):
    return (v >> 1) | (v & 1)


def chroma_mv4(s):
    tab = [0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2]
    return tab[s & 15] + ((s >> 3) & ~1)


def reconstruct(w, h, vops, fcode=1, quant_type=0, intra_matrix=None, inter_matrix=None, strict_idct=False):
    """The expected I420 planes of each VOP spec [(kind, mbs, q0, rounding)] (numpy).  quant_type 1:
    MPEG inverse quantisation with the matrices as given to vol_header (None: the defaults).

    A macroblock given as None is lost (no video packet holds it): a decoder that alternates
    between two pictures, writing each coded VOP over the picture of two coded VOPs earlier,
    leaves that older picture's pixels there, or Y = U = V = 128 where no such picture exists
    yet.  Every written macroblock of a stream with video packets carries its "q" (the packet
    header's quant_scale changes the running QP)."""
    mats = [expand_matrix(inter_matrix, DEFAULT_INTER_MATRIX), expand_matrix(intra_matrix, DEFAULT_INTRA_MATRIX)]
    pics = [[np.full((h, w), 128, np.int64), np.full((h // 2, w // 2), 128, np.int64),
             np.full((h // 2, w // 2), 128, np.int64)] for _ in range(2)]
    frames, cur_i = [], 0
    for kind, mbs, q0, rnd in vops:
        cur_i ^= 1
        planes, ref = pics[cur_i], pics[cur_i ^ 1]
        q = q0
        for y in range(h // 16):
            for x in range(w // 16):
                mb = mbs[y][x]
                if mb is None:
                    continue
                t = mb.get("type", "intra")
                q = mb.get("q", q)
                if t == "skip":
                    for pl, sz in ((0, 16), (1, 8), (2, 8)):
                        planes[pl][sz * y:sz * y + sz, sz * x:sz * x + sz] = ref[pl][sz * y:sz * y + sz, sz * x:sz * x + sz]
                    continue
                blocks = np.asarray(mb.get("blocks", np.zeros((6, 64))), np.int64).reshape(6, 64)
                pred = None
                if t in ("inter", "inter4v"):
                    mvs = mb["mvs"] if t == "inter4v" else [mb["mv"]] * 4
                    lp = np.zeros((16, 16), np.int64)
                    if t == "inter4v":
                        for k in range(4):
                            lp[8 * (k >> 1):8 * (k >> 1) + 8, 8 * (k & 1):8 * (k & 1) + 8] = mc_plane(
                                ref[0], 16 * x + 8 * (k & 1), 16 * y + 8 * (k >> 1), 8, 8, mvs[k][0], mvs[k][1], rnd)
                        cx = chroma_mv4(sum(m[0] for m in mvs))
                        cy = chroma_mv4(sum(m[1] for m in mvs))
                    else:
                        lp = mc_plane(ref[0], 16 * x, 16 * y, 16, 16, mvs[0][0], mvs[0][1], rnd)
                        cx, cy = chroma_mv(mvs[0][0]), chroma_mv(mvs[0][1])
                    pred = [lp] + [mc_plane(ref[c], 8 * x, 8 * y, 8, 8, cx, cy, rnd) for c in (1, 2)]
                for n in range(6):
                    intra = pred is None
                    if intra or blocks[n].any():
                        deq = (dequant_mpeg(blocks[n], q, intra, n < 4, mats[int(intra)]) if quant_type
                               else dequant_h263(blocks[n], q, intra, n < 4))
                        res = simple_idct(deq, strict_idct)
                    else:
                        res = np.zeros((8, 8), np.int64)   # a block without coded coefficients adds nothing
                    if n < 4:
                        pl, oy, ox = 0, 16 * y + 8 * (n >> 1), 16 * x + 8 * (n & 1)
                        base = None if intra else pred[0][8 * (n >> 1):8 * (n >> 1) + 8, 8 * (n & 1):8 * (n & 1) + 8]
                    else:
                        pl, oy, ox = n - 3, 8 * y, 8 * x
                        base = None if intra else pred[n - 3]
                    val = res if intra else base + res
                    planes[pl][oy:oy + 8, ox:ox + 8] = np.clip(val, 0, 255)
        frames.append([p.astype(np.uint8) for p in planes])
    return frames


# ------------------------------------------------------------------ containers
def _box(kind, body):
    import struct
    return struct.pack(">I4s", 8 + len(body), kind) + body


def _desc(tag, body):
    n = len(body)
    return bytes([tag, 0x80 | (n >> 21) & 0x7F, 0x80 | (n >> 14) & 0x7F, 0x80 | (n >> 7) & 0x7F, n & 0x7F]) + body


def mp4_file(config, samples, w, h, fps=30, chunk=3):
    """A minimal ISO BMFF file: ftyp, moov (one 'vide' track with an 'mp4v' sample entry whose
    esds carries `config`; samples grouped `chunk` per chunk through stsc / stco / stsz), mdat."""
    import struct
    esds = _box(b"esds", b"\0\0\0\0" + _desc(0x03, struct.pack(">HB", 1, 0) + _desc(
        0x04, bytes([0x20, 0x11]) + b"\0\0\0" + struct.pack(">II", 0, 0) + _desc(0x05, config)) + _desc(0x06, b"\x02")))
    entry = (b"\0" * 6 + struct.pack(">H", 1) + b"\0" * 16 + struct.pack(">HH", w, h) +
             struct.pack(">IIIH", 0x480000, 0x480000, 0, 1) + b"\0" * 32 + struct.pack(">Hh", 24, -1) + esds)
    stsd = _box(b"stsd", struct.pack(">II", 0, 1) + _box(b"mp4v", entry))
    stts = _box(b"stts", struct.pack(">III", 0, 1, len(samples)) + struct.pack(">I", 1000))
    n_chunks = (len(samples) + chunk - 1) // chunk
    stsc_rows = [(1, chunk, 1)]
    if len(samples) % chunk:
        stsc_rows.append((n_chunks, len(samples) % chunk, 1))
    stsc = _box(b"stsc", struct.pack(">II", 0, len(stsc_rows)) + b"".join(struct.pack(">III", *r) for r in stsc_rows))
    stsz = _box(b"stsz", struct.pack(">III", 0, 0, len(samples)) + b"".join(struct.pack(">I", len(s)) for s in samples))
    mdhd = _box(b"mdhd", struct.pack(">IIIIIHH", 0, 0, 0, int(fps * 1000), len(samples) * 1000, 0, 0))
    hdlr = _box(b"hdlr", struct.pack(">II4s", 0, 0, b"vide") + b"\0" * 12 + b"VideoHandler\0")

    def build(chunk_offsets):
        stco = _box(b"stco", struct.pack(">II", 0, len(chunk_offsets)) + b"".join(struct.pack(">I", o)
                                                                                  for o in chunk_offsets))
        stbl = _box(b"stbl", stsd + stts + stsc + stsz + stco)
        minf = _box(b"minf", _box(b"vmhd", struct.pack(">IHHHH", 1, 0, 0, 0, 0)) + stbl)
        mdia = _box(b"mdia", mdhd + hdlr + minf)
        trak = _box(b"trak", _box(b"tkhd", struct.pack(">II", 3, 0) + b"\0" * 76 + struct.pack(">II", w << 16, h << 16))
                    + mdia)
        return _box(b"moov", _box(b"mvhd", b"\0" * 100) + trak)

    ftyp = _box(b"ftyp", b"isom\0\0\x02\0isomiso2mp41")
    moov = build([0] * n_chunks)
    base = len(ftyp) + len(moov) + 8
    offs, o = [], base
    for i, s in enumerate(samples):
        if i % chunk == 0:
            offs.append(o)
        o += len(s)
    moov = build(offs)
    return ftyp + moov + _box(b"mdat", b"".join(samples))
