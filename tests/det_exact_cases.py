"""Exactly summable data for the person detector's kernels, and a float64 reference of every op.

The method is tests/exact_cases.py's (whose quantum, _seed, exact_input, normal_input and LIMIT are
used here, not copied): every weight and activation of a conv is a multiple of a power-of-two
quantum q and every partial sum stays below 2^24 q, so every f32 partial sum is exact in any order
and the conv's bf16 result is ONE array whatever the MFMA K order, tile shape, ring depth or fold.
A float64 conv on the CPU gives that array; tests/test_det_exact_gpu.py demands it of every kernel
variant of csrc/det_select.h bit for bit, each op alone in a one-op detector (build()), at planes
of a few dozen pixels where every tile is ragged.  tests/test_det_exact_cases.py holds this module
to its own claims on the CPU.

Data.  Ternary conv weights +-2^-shift at `nnz` seeded positions per output channel, integer
biases, integer inputs in [-3, 3] (exact_input).  The weights go through rtmdet.fold and
to_bf16_bits like any others (BN weight 1, mean 0, var 1: the scale 1 / sqrt(1 + 1e-5) vanishes in
the bf16 rounding; the depthwise and stem weights stay f32 on the device and get var 1 - 1e-5, so
that their scale rounds to 1 in f32), and check_blobs asserts what the blobs then hold.

Reference.  Each op is restated from its definition in float64 on the device's storage layout,
read from the DetOp and the blobs: channel views, padded couts (zero weights and bias), shared
concat buffers.  Every conv asserts that all values are multiples of q and that B / q <= LIMIT =
2^20, B = conv(|x|, |w|) + |bias| + |res|.  The largest B / q among the cases is 32,328 (a fold_ca
case: its scaled input has the finest quantum; 2,400 among the others).  On an MI355X every variant
(band_8w, band_4w, halo_2row, halo, halo_live3, halo_pers_lt2 / lt3 / lt4, fold_up, fold_ca,
pers_gemm, gemm on v_mfma_f32_16x16x32_bf16; stem, dw5, dwpw, the attention kernels, spp, up2, both
heads) is exact on every one of its cases, so nothing here says where below 2^20 exactness ends.
The expected output is canonicalised to +0.  The device cannot produce -0 on this data: every
accumulator starts at +0, and in round-to-nearest a sum is -0 only if every addend is, so no conv
sum is -0 whatever the signs of its zero products; the biases and residuals are written as +0;
fmaxf(v, +0) of a negative v is +0; SiLU of a non-zero multiple of q is far from underflow, and
silu(+0) = +0 * 0.5.  (The attention scale is the exception, and is not canonicalised: a negative
value times a scale of exactly 0 is -0 on the device and in the numpy restatement alike.)

Regimes, per conv family, as for HRNet: `small` (shift 0, few non-zeros: every value fits bf16's 8
bits) and `rounding` (shift 8 and biases in front: the value is its bias plus a sum of 1/256ths,
one or two bits more than bf16 has, ties included; exact_cases.ROUNDING explains it).  Behind a
ReLU the rounding cases draw their biases from exact_cases.ONE so that no channel dies.

Activations.  ACT_NONE and ACT_RELU are bit for bit.  A residual under ACT_RELU is added before
the ReLU, under ACT_SILU after the activation.  SiLU is v * rcp(1 + __expf(-v)) in f32 on the
device, which no CPU reproduces bit for bit: with z the exact pre-activation (|z| <= 26 asserted)
the expected value is bf16(silu_f64(z) + res), and an element is *undecidable* when the interval
r +- 2^-18 (|silu(z)| + |res|) holds a bf16 rounding boundary; there the device may give any bf16
value from the rounding of one end to that of the other, everywhere else the expected bits.  The
ends are the two bf16 neighbours (the CPU test asserts it) except at the few elements, under 0.2 %
of a case with a residual, where the residual cancels the SiLU (silu(3.125) - 3 = -0.0066) and the
interval, sized by the terms, spans two steps of their small sum.  2^-18 is from the accuracies det_common.h states:
-v log2(e) rounded once is |v| 2^-24 relative after the exponential, v_exp and v_rcp 1 ulp each,
two more roundings and the add: (|v| + 6) 2^-24 <= 2^-19 for |v| <= 26, and one bit of margin.
(The ISA guides at hand give no other accuracy for v_exp_f32 or v_rcp_f32.)  At most 2 % of a SiLU
case may be undecidable.  The fused depthwise + pointwise op has no SiLU case: its intermediate
would carry the activation's error into the pointwise sum, where it is no longer one rounding
boundary per element.

Untouched bytes.  Every output tensor starts as a NaN sentinel no result equals: inside the view
every stored channel is written (padding couts +0), outside it the sentinel survives.

Channel attention.  Expected scales are the kernels' arithmetic in numpy float32: the channel sums
(integers: exact in any order), / HW, the fmaf chain in k order, min(max(a + 3, 0), 6) / 6; the
tensor is bf16(f32(x) * s).  The fc weights are 0 or +-2^-shift, so w * mean is exact in f32 and
fmaf(w, mean, a) IS the f32 sum a + (w * mean): an fma that rounds once, also where the mean is
not dyadic (the 5x5 and 20x20 planes); the CPU test repeats one such chain with fractions.Fraction.

CASES is the one table both test files walk; Case.key names the data, which cases that differ only
in switches share (reference() is cached on it).
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from exact_cases import LIMIT, ONE, _seed, exact_input, normal_input, quantum
from mvpose import rtmdet as D

NONE, RELU, SILU = D.ACT_NONE, D.ACT_RELU, D.ACT_SILU
ACT_NAME = {NONE: "none", RELU: "relu", SILU: "silu"}
BIASES = (-2, -1, 0, 1, 2)
SILU_MAX = 26.0
SILU_WIDTH = 2.0 ** -18
SILU_CAP = 0.02
SENT16 = -57            # 0xFFC7: a bf16 NaN no kernel produces
SENT32 = -4194297       # 0xFFC00007: the same for the f32 candidates
CUS = 256               # the part the expected variants are stated for
SWITCHES = ("MVPOSE_DET_XCD", "MVPOSE_DET_BAND", "MVPOSE_DET_PERS", "MVPOSE_DET_PERS_OCC", "MVPOSE_DET_FOLD",
            "MVPOSE_DET_HALO_PERS", "MVPOSE_DET_HALO_ROWS", "MVPOSE_DET_LIVE", "MVPOSE_DET_HEAD_DIRECT",
            "MVPOSE_DET_DWPW")


# ------------------------------------------------------------------ bf16 --
def bf16_round(a):
    """float64 -> the nearest bf16 value (ties to even), as float64, in one rounding; -0 -> +0."""
    m, e = np.frexp(np.asarray(a, np.float64))
    return np.ldexp(np.rint(np.ldexp(m, 8)), e - 8) + 0.0


def bf16_bits(a):
    """Bit patterns (int16) of bf16-representable float64 values."""
    f = np.asarray(a, np.float64).astype(np.float32)
    assert np.array_equal(f.astype(np.float64), a), "not f32 values"
    u = np.ascontiguousarray(f).view(np.uint32)
    assert not np.any(u & 0xFFFF), "not bf16 values"
    return (u >> 16).astype(np.uint16).view(np.int16)


def bits_f64(bits):
    """float64 values of bf16 bit patterns (a torch int16 / bfloat16 tensor or an int16 array)."""
    if isinstance(bits, torch.Tensor):
        bits = (bits.view(torch.int16) if bits.dtype == torch.bfloat16 else bits).numpy()
    return (bits.view(np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def sentinel(shape):
    return torch.full(tuple(shape), SENT16, dtype=torch.int16).view(torch.bfloat16)


# ------------------------------------------------------------------ cases --
class Case:
    """One op in one detector under one set of switches.  op: conv | stem | dw | dwpw | ca | spp |
    up2 | head; family: the GPU test that walks it; variant: the kernel it must run on a 256-CU
    part; the other fields are the op's (see _DEFAULTS)."""
    _DEFAULTS = dict(env=(), n=3, act=NONE, res=False, regime="small", nnz=0, shift=0, biases=BIASES, ks=1, stride=1,
                     h=0, w=0, cin=0, cout=0, out_c=0, out_at=(0, 0), in_at=(0, 0), fold=None, up_c=0, size=32,
                     salt=0, direct=False, random=False)

    def __init__(self, family, op, variant, tag, **kw):
        bad = set(kw) - set(self._DEFAULTS)
        assert not bad, bad
        self.__dict__.update(self._DEFAULTS)
        self.__dict__.update(kw)
        self.family, self.op, self.variant = family, op, variant
        self.env = dict(self.env)
        for name, at in (("in", self.in_at), ("out", self.out_at)):   # a view at coff of a wider tensor
            if at[1]:
                tag += f"-{name}{at[0]}of{at[1]}"
        self.key = f"{op}-{tag}-{ACT_NAME[self.act]}-{self.regime}"
        sw = "".join(f"-{k[len('MVPOSE_DET_'):]}={v}" for k, v in sorted(self.env.items()))
        self.id = f"{variant}-{tag}-{ACT_NAME[self.act]}-{self.regime}{sw}"

    def __repr__(self):
        return self.id

    def ordinary(self):
        """The same op with ordinary random weights, biases and data (no exactness): what the
        reference is compared with the interpreter on."""
        c = Case.__new__(Case)
        c.__dict__.update(self.__dict__)
        c.random, c.nnz, c.biases, c.key = True, None, None, self.key + "-ordinary"
        return c


# weight seeds moved on until the case's conditions hold (test_det_exact_cases.py checks them)
SALT = {}

# (act, regime, nnz, shift): what every conv shape is run with.  none/small and relu/rounding give
# each family both regimes and both exact activations; silu has z in multiples of 2^-3.
MODES = ((NONE, "small", 6, 0), (RELU, "rounding", 144, 8), (SILU, "silu", 16, 3))
# behind the attention fold the input is bf16(x * s), 8 significant bits below 2^-2: rounding
# happens with unit weights, and shift 8 would pass 2^20
CA_MODES = ((NONE, "rounding", 8, 0), (RELU, "rounding", 8, 0), (SILU, "silu", 8, 3))


def _conv_cases(family, variant, tag, env=(), modes=MODES, only=None, **kw):
    out = []
    for act, regime, nnz, shift in modes:
        if only is not None and act != only:
            continue
        biases = ONE if (act == RELU and regime == "rounding") else BIASES
        c = Case(family, "conv", variant, tag, env=env, act=act, regime=regime, nnz=nnz, shift=shift, biases=biases, **kw)
        c.salt = SALT.get(c.key, 0)
        out.append(c)
    return out


def _tag(cin, cout, ks, stride, h, w, n, res=False, extra=""):
    return f"{cin}x{cout}-k{ks}s{stride}-{h}x{w}x{n}{'-res' if res else ''}{extra}"


def _cases():
    out = []
    # ---- the im2col GEMM and its persistent form: the same shapes, MVPOSE_DET_PERS = 0 | default | 3
    PW = [(32, 32), (64, 64), (96, 96), (128, 128), (192, 192), (96, 384)]
    for pers in ("0", None, "3"):
        for h in (5, 20):
            for cin, cout in PW:
                if pers == "3":
                    continue  # the 1x1 convs are persistent by default
                env = {"MVPOSE_DET_PERS": "0"} if pers == "0" else {}
                kw = {}
                extra = ""
                if (cin, cout, h) == (64, 64, 20):   # a view at coff > 0 of wider tensors, both sides
                    kw, extra = dict(out_at=(64, 192), in_at=(32, 128)), "-views"
                if (cin, cout, h) == (128, 128, 5):  # a residual on the 1x1 form
                    kw, extra = dict(res=True, out_at=(128, 256)), "-res-views"
                out += _conv_cases("gemm", "gemm" if pers == "0" else "pers_gemm",
                                   _tag(cin, cout, 1, 1, h, h, 3, extra=extra), env, cin=cin, cout=cout, h=h, w=h, **kw)
            if pers is None:
                continue
            env = {"MVPOSE_DET_PERS": pers}
            v = "gemm" if pers == "0" else "pers_gemm"
            out += _conv_cases("gemm", v, _tag(96, 96, 3, 1, h, h, 3), env, cin=96, cout=96, ks=3, h=h, w=h)
            for h2 in ((5, 10, 20) if h == 5 else ()):
                out += _conv_cases("gemm", v, _tag(96, 192, 3, 2, h2, h2, 3), env, cin=96, cout=192, ks=3, stride=2,
                                   h=h2, w=h2)
            if h == 20:
                out += _conv_cases("gemm", v, _tag(128, 64, 3, 1, h, h, 3, True), env, cin=128, cout=64, ks=3, h=h, w=h,
                                   res=True, out_at=(64, 128))
    # more (tile, cout block) items than workgroups: 88 tiles x 4 blocks over 256 workgroups
    out += _conv_cases("gemm", "pers_gemm", _tag(96, 768, 1, 1, 40, 40, 7), {"MVPOSE_DET_PERS_OCC": "1"}, only=RELU,
                       cin=96, cout=768, h=40, w=40, n=7)
    # ---- the folds: [up(x) | y] with the upsample never run, and attention + 1x1
    for cout in (192, 96):
        for h, cin, up_c in ((10, 128, 64), (40, 96, 32)):
            out += _conv_cases("fold", "fold_up", _tag(cin, cout, 1, 1, h, h, 3, extra=f"-up{up_c}"), cin=cin, cout=cout,
                               h=h, w=h, fold="up", up_c=up_c)
        for h, n in ((5, 7), (20, 3)):
            out += _conv_cases("fold", "fold_ca", _tag(64, cout, 1, 1, h, h, n, extra="-ca"), modes=CA_MODES, cin=64,
                               cout=cout, h=h, w=h, n=n, fold="ca")
    # ---- halo tiles (3x3/s1, 32 or 64 input channels, <= 64 couts)
    PLANES = ((5, 5), (9, 70), (20, 20))
    NOPERS = {"MVPOSE_DET_HALO_PERS": "0"}
    for h, w in PLANES:
        out += _conv_cases("halo", "halo", _tag(32, 32, 3, 1, h, w, 3, True), cin=32, cout=32, ks=3, h=h, w=w, res=True,
                           out_at=(32, 96))
        out += _conv_cases("halo", "halo", _tag(64, 64, 3, 1, h, w, 3, True), cin=64, cout=64, ks=3, h=h, w=w, res=True)
        out += _conv_cases("halo", "halo", _tag(64, 64, 3, 1, h, w, 3), NOPERS, cin=64, cout=64, ks=3, h=h, w=w,
                           in_at=(64, 128))
        out += _conv_cases("halo", "halo_live3", _tag(64, 48, 3, 1, h, w, 3), NOPERS, cin=64, cout=48, out_c=64, ks=3,
                           h=h, w=w, out_at=(64, 128))
    out += _conv_cases("halo", "halo_live3", _tag(32, 48, 3, 1, 9, 70, 3), NOPERS, cin=32, cout=48, out_c=64, ks=3,
                       h=9, w=70)
    ROWS2 = {"MVPOSE_DET_HALO_ROWS": "2"}
    for h, w in PLANES[:2]:
        out += _conv_cases("halo", "halo_2row", _tag(64, 64, 3, 1, h, w, 3, True), ROWS2, cin=64, cout=64, ks=3, h=h, w=w,
                           res=True)
        out += _conv_cases("halo", "halo_2row", _tag(32, 32, 3, 1, h, w, 3, True), ROWS2, cin=32, cout=32, ks=3, h=h, w=w,
                           res=True, out_at=(32, 96))
        out += _conv_cases("halo", "halo_2row", _tag(64, 64, 3, 1, h, w, 3), ROWS2, cin=64, cout=64, ks=3, h=h, w=w,
                           in_at=(64, 128))
    # ---- the persistent halo kernel: 2 / 3 / 4 live 16-cout tiles
    for h, w in PLANES[:2]:
        for cin, cout, lt in ((32, 24, 2), (32, 48, 3), (64, 48, 3), (32, 64, 4), (64, 64, 4)):
            at = (32, 96) if (cin, cout) == (32, 24) else (64, 128) if (cin, cout) == (64, 48) else (0, 0)
            out += _conv_cases("halo_pers", f"halo_pers_lt{lt}", _tag(cin, cout, 3, 1, h, w, 3), cin=cin, cout=cout,
                               out_c=D.pad32(cout), ks=3, h=h, w=w, out_at=at)
    # 300 8x64 tiles, two chunks each, over 256 workgroups: several steps per workgroup, the double buffer wraps
    out += _conv_cases("halo_pers", "halo_pers_lt3", _tag(64, 48, 3, 1, 160, 160, 5), only=RELU, cin=64, cout=48, out_c=64,
                       ks=3, h=160, w=160, n=5)
    # ---- the band kernel (80x80 / 40x40, >= 96 input channels), 8 and 4 waves; 3 frames: uneven XCD groups
    for band in (None, "4"):
        env = {"MVPOSE_DET_BAND": "4"} if band else {}
        v = "band_4w" if band else "band_8w"
        for cin, cout, h, res in ((96, 64, 40, False), (96, 96, 40, True), (192, 192, 40, False), (96, 64, 80, True),
                                  (96, 96, 80, False)):
            at = (64, 192) if (cout, h) == (64, 40) else (0, 0)
            out += _conv_cases("band", v, _tag(cin, cout, 3, 1, h, h, 3, res), env, cin=cin, cout=cout, ks=3, h=h, w=h,
                               res=res, out_at=at)
    # ---- the stem: 3x3/s2, 3 (of 4) -> 24 (of 32) channels, f32 weights; 96 / 2 = 48 is 6 16-pixel
    # tiles per row pair over 4 waves
    for size in (64, 96):
        for act, regime, nnz, shift in ((NONE, "small", 8, 0), (RELU, "rounding", 27, 8), (SILU, "silu", 16, 3)):
            out.append(Case("stem", "stem", "stem", f"{size}", size=size, act=act, regime=regime, nnz=nnz, shift=shift,
                            biases=ONE if act == RELU else BIASES, h=size, w=size, cin=4, cout=24))
    # ---- depthwise 5x5: all 25 taps, distinct magnitudes (t + 1) / 2^shift
    for c in (32, 64, 96, 192):
        for h in (3, 5, 20):
            for act, shift in ((NONE, 5), (RELU, 5), (SILU, 6)):
                if act == SILU and (c, h) not in ((32, 5), (96, 20), (192, 3)):
                    continue
                at = (32, 128) if c == 32 else (0, 0)
                out.append(Case("dw5", "dw", "dw5", f"{c}-{h}x{h}", act=act, regime="taps" if act != SILU else "silu",
                                shift=shift, h=h, w=h, cin=c, cout=c, in_at=at))
    # ---- depthwise 5x5 + pointwise 1x1 in one launch
    for c, cout in ((64, 48), (96, 96)):
        for h in (4, 5, 20, 33):
            for res in (False, True):
                modes = ((NONE, "small"), (RELU, "rounding")) if h in (5, 33) else ((RELU, "small"), (NONE, "rounding"))
                for act, regime in modes:
                    at = (c, 2 * c) if res else (0, 0)
                    out.append(Case("dwpw", "dwpw", "dwpw", f"{c}x{cout}-{h}x{h}{'-res' if res else ''}", act=act,
                                    regime=regime, nnz=6, h=h, w=h, cin=c, cout=cout, out_c=c, res=res, out_at=at,
                                    shift=0 if regime == "small" else 6))
    # ---- channel attention, unfolded: pool, fc, scale
    for c in (64, 192, 768):
        for h in (4, 8):
            for n in (2, 9):
                at = (64, 192) if c == 64 else (0, 0)
                out.append(Case("ca", "ca", "ca_pool", f"{c}-{h}x{h}x{n}", n=n, h=h, w=h, cin=c, cout=c, nnz=8, in_at=at,
                                regime="scale"))
    out.append(Case("ca", "ca", "ca_pool", "64-5x5x2", n=2, h=5, w=5, cin=64, cout=64, nnz=8, regime="scale"))
    # ---- SPP, upsample
    for c in (32, 192):
        for h, w in ((5, 5), (4, 7), (20, 20)):
            out.append(Case("spp", "spp", "spp", f"{c}-{h}x{w}", h=h, w=w, cin=c, cout=c, regime="copy"))
    for h in (5, 20):
        out.append(Case("up2", "up2", "up2", f"64-{h}x{h}", h=h, w=h, cin=64, cout=64, out_at=(32, 128), in_at=(64, 128),
                        regime="copy"))
    # ---- the head: F = 192, 5x5 at stride 32 and 20x20 at stride 8 of one size-160 detector
    for direct in (False, True):
        for h, stride in ((5, 32), (20, 8)):
            out.append(Case("head", "head", "head_direct" if direct else "head_staged", f"192-{h}x{h}-s{stride}",
                            env={"MVPOSE_DET_HEAD_DIRECT": "1"} if direct else {}, h=h, w=h, cin=384, stride=stride,
                            size=160, nnz=16, shift=4, regime="head", direct=direct))
    return out


# ------------------------------------------------------------- selection --
def switches(env):
    """DetSwitches as detnet.cpp's read_det_switches reads them from `env`."""
    first = lambda k: env.get(k, "")[:1]  # noqa: E731
    return dict(band=0 if first("MVPOSE_DET_BAND") == "0" else 4 if first("MVPOSE_DET_BAND") == "4" else 1,
                pers=0 if first("MVPOSE_DET_PERS") == "0" else 3 if first("MVPOSE_DET_PERS") == "3" else 1,
                fold=first("MVPOSE_DET_FOLD") != "0", halo_pers=first("MVPOSE_DET_HALO_PERS") != "0",
                halo_rows2=first("MVPOSE_DET_HALO_ROWS") == "2", live=first("MVPOSE_DET_LIVE") != "0",
                head_direct=first("MVPOSE_DET_HEAD_DIRECT") == "1")


def conv_bn(npad):
    return next((b for b in (192, 128, 96, 64) if npad % b == 0), 32)


def fold_shape_ok(h, w, cin, n, ks, ca):
    if ks != 1 or n > 1024 or cin % 32:
        return False
    if conv_bn(D.pad32(n)) not in (192, 96):
        return False
    return not ca or (127 + h * w - 1) // (h * w) + 1 <= 8


def select_conv(h, w, cin, cout, ks, stride, live, res, fold, sw, cus=CUS):
    """csrc/det_select.h select_det_conv, restated (h x w the input plane, cin / cout the views'
    stored channels): the name of the variant, "" for none.  The GPU test's launch_kernels
    assertion holds the restatement to the library."""
    npad = D.pad32(cout)
    live = cout if live <= 0 or live > cout else live
    if (ks, stride) not in ((1, 1), (3, 1), (3, 2)) or cin % 32 or cout % 4:
        return ""
    if fold and not fold_shape_ok(h, w, cin, cout, ks, fold == "ca"):
        return ""
    band_ok = ks == 3 and stride == 1 and h == w and w in (80, 40) and cin // 32 >= 3 and npad <= 32 * 64
    if band_ok and (npad + 63) // 64 <= max(8, cus // 8 * 8) // 8 and sw["band"]:
        return "band_4w" if sw["band"] == 4 else "band_8w"
    if ks == 3 and stride == 1 and cin in (32, 64) and npad <= 64:
        if sw["halo_rows2"]:
            return "halo_2row"
        pers = not res and sw["halo_pers"]
        if npad == 64:
            if live == 48 and pers:
                return "halo_pers_lt3"
            if live == 64 and pers:
                return "halo_pers_lt4"
            return "halo_live3" if 32 < live <= 48 and not res and sw["live"] else "halo"
        return "halo_pers_lt2" if cin == 32 and live > 16 and pers else "halo"
    if fold:
        return "fold_" + fold
    if cout <= 1024 and sw["pers"] and (ks == 1 or sw["pers"] == 3):
        return "pers_gemm"
    return "gemm"


def expected_variant(case):
    """The variant det_select.h gives the case's op on a 256-CU part under the case's switches."""
    sw = switches(case.env)
    if case.op == "conv":
        fold = case.fold if sw["fold"] and sw["pers"] else None
        return select_conv(case.h, case.w, case.cin, case.out_c or D.pad32(case.cout), case.ks, case.stride, case.cout,
                           case.res, fold, sw)
    if case.op == "head":
        return "head_staged" if (case.cin // 2) % 32 == 0 and not sw["head_direct"] else "head_direct"
    return {"stem": "stem", "dw": "dw5", "dwpw": "dwpw", "ca": "ca_pool", "spp": "spp", "up2": "up2"}[case.op]


# ------------------------------------------------------------------ data --
def _gen(case, what):
    return torch.Generator().manual_seed(_seed(case.key, what, case.salt))


def ternary(g, cout, fan, nnz, shift):
    """(cout, fan) float64: min(nnz, fan) values +-2^-shift per row at seeded positions (nnz None:
    ordinary N(0, 1 / fan) weights, for the comparison with the interpreter)."""
    if nnz is None:
        return torch.randn((cout, fan), generator=g, dtype=torch.float64) / fan ** 0.5
    w = torch.zeros((cout, fan), dtype=torch.float64)
    for o in range(cout):
        pos = torch.randperm(fan, generator=g)[:min(nnz, fan)]
        w[o, pos] = (torch.randint(0, 2, (pos.numel(),), generator=g) * 2.0 - 1.0).double() * 2.0 ** -shift
    return w


def draw(g, c, pool):
    if pool is None:
        return torch.randn(c, generator=g)
    return torch.tensor(pool, dtype=torch.float32)[torch.randint(0, len(pool), (c,), generator=g)]


def dw_taps(g, c, shift, taps=25):
    """(c, 1, 5, 5): per channel, `taps` non-zero taps at seeded positions; all 25 get the distinct
    magnitudes (t + 1) / 2^shift in a seeded order (a swapped tap changes bits), fewer get +-2^-shift."""
    if taps is None:
        return torch.randn((c, 1, 5, 5), generator=g, dtype=torch.float64) / 5
    w = torch.zeros((c, 25), dtype=torch.float64)
    for o in range(c):
        pos = torch.randperm(25, generator=g)[:taps]
        sign = (torch.randint(0, 2, (taps,), generator=g) * 2.0 - 1.0).double()
        mag = (torch.arange(25, dtype=torch.float64) + 1.0) if taps == 25 else torch.ones(taps, dtype=torch.float64)
        w[o, pos] = sign * mag * 2.0 ** -shift
    return w.reshape(c, 1, 5, 5)


def module_sd(name, w, bias, f32=False):
    """A ConvModule's entries: conv weight w (cout, cin / groups, k, k), BN weight 1, mean 0, var 1
    (1 - 1e-5 for weights that stay f32, exact_cases._plain_bn), bias `bias`."""
    c = w.shape[0]
    return {name + ".conv.weight": w.float(), name + ".bn.weight": torch.ones(c), name + ".bn.bias": bias.float(),
            name + ".bn.running_mean": torch.zeros(c),
            name + ".bn.running_var": torch.full((c,), 1.0 - 1e-5 if f32 else 1.0)}


def int_data(case, what, shape, real=None):
    """Integers in [-3, 3] as bf16 (n, h, w, c); stored channels past `real` are zero."""
    if case.random:
        x = torch.randn(tuple(shape), generator=_gen(case, what)).bfloat16()
        if shape[-1] == 4:
            x[..., 3] = 0
    else:
        x = exact_input(shape, _seed(case.key, what))
    if real is not None:
        x[..., real:] = 0
    return x


def placed(x, at):
    """x (n, h, w, c) as channels [coff, coff + c) of a sentinel tensor of `total` channels (at = (coff, total);
    (0, 0): x itself)."""
    coff, total = at
    if not total:
        return x.contiguous()
    t = sentinel(x.shape[:3] + (total,))
    t[..., coff:coff + x.shape[3]] = x
    return t


# ----------------------------------------------------------------- build --
class Built:
    """A case's one-op detector: spec, the ops [begin, end) to run, the tensors to set before the
    run ({tensor id: bf16 (n, h, w, c)}), the tensor to read back and the index of the op whose
    kernel the case names."""

    def __init__(self, spec, begin, end, inputs, out_t, op_index):
        self.spec, self.begin, self.end, self.inputs, self.out_t, self.op_index = spec, begin, end, inputs, out_t, op_index
        self.op = spec.ops[op_index]


def _base(size):
    """A DetSpec with what detnet.cpp's validation wants around the op under test: tensor 0 the
    size x size x 4 input, op 0 a filler (run_ops(0, ..) would start with the letterbox), and, by
    _finish, a small head level so that n_priors > 0."""
    g = D.DetSpec(size, fuse_dwpw=True)
    g.tensor(size, size, 4)
    g.up2(g.new(1, 1, 32), g.new(2, 2, 32))
    return g


def _finish(g):
    s = g.size // 32
    g.head("filler-head", np.zeros((5, 16)), np.zeros(5), g.new(s, s, 32), 32)
    return g


def _view(g, h, w, c, at, real=None):
    coff, total = at
    return D.View(g.tensor(h, w, total or c), coff, c, np.arange(real or c))


@functools.lru_cache(maxsize=None)
def _build(key, case):
    g = _base(case.size)
    n, h, w = case.n, case.h, case.w
    wg = _gen(case, "w")
    inputs = {}
    if case.op == "conv":
        k, st = case.ks, case.stride
        ho, wo = (h + 2 * (k // 2) - k) // st + 1, (w + 2 * (k // 2) - k) // st + 1
        out_c = case.out_c or D.pad32(case.cout)
        sd = module_sd("c", ternary(wg, case.cout, case.cin * k * k, case.nnz, case.shift).reshape(case.cout, k, k, case.cin)
                       .permute(0, 3, 1, 2), draw(wg, case.cout, case.biases))
        x = _view(g, h, w, case.cin, case.in_at)
        xd = int_data(case, "x", (n, h, w, case.cin))
        first = len(g.ops)
        if case.fold == "up":   # [up(src) | y]: the slice [0, up_c) is never written, the conv reads src
            src = _view(g, h // 2, w // 2, case.up_c, (32, case.up_c + 64))
            g.up2(src, D.View(x.t, 0, case.up_c, np.arange(case.up_c)))
            inputs[src.t] = placed(int_data(case, "up", (n, h // 2, w // 2, case.up_c)), (32, case.up_c + 64))
            xd[..., :case.up_c] = sentinel((n, h, w, case.up_c))
        elif case.fold == "ca":
            g.attention(_ca_sd(case, wg, case.cin), "a", x)
        inputs[x.t] = placed(xd, case.in_at)
        out = _view(g, ho, wo, out_c, case.out_at, case.cout)
        res = None
        if case.res:
            res = _view(g, ho, wo, out_c, (0, 0), case.cout)
            inputs[res.t] = int_data(case, "res", (n, ho, wo, out_c), case.cout)
        op_index = len(g.ops)
        g.conv(sd, "c", x, k, st, out=out, res=res, act=case.act)
        inputs[out.t] = sentinel((n,) + g.tensors[out.t][:3])
        return Built(_finish(g), first if case.fold == "ca" else op_index, op_index + 1, inputs, out.t, op_index)
    if case.op == "stem":
        sd = module_sd("c", ternary(wg, 24, 27, case.nnz, case.shift).reshape(24, 3, 3, 3).permute(0, 3, 1, 2),
                       draw(wg, 24, case.biases), f32=True)
        out = g.stem(sd, "c", D.View(0, 0, 4, np.arange(3)), act=case.act)
        inputs[0] = int_data(case, "x", (n, h, w, 4))
        inputs[out.t] = sentinel((n, h // 2, w // 2, 32))
        return Built(_finish(g), 1, 2, inputs, out.t, 1)
    if case.op == "dw":
        sd = module_sd("c", dw_taps(wg, case.cin, case.shift, None if case.random else 25),
                       draw(wg, case.cin, case.biases), f32=True)
        x = _view(g, h, w, case.cin, case.in_at)
        out = g.dw(sd, "c", x, act=case.act)
        inputs[x.t] = placed(int_data(case, "x", (n, h, w, case.cin)), case.in_at)
        inputs[out.t] = sentinel((n, h, w, case.cin))
        return Built(_finish(g), 1, 2, inputs, out.t, 1)
    if case.op == "dwpw":
        c = case.cin
        small = case.regime == "small"
        sd = module_sd("d", dw_taps(wg, c, case.shift, None if case.random else 9 if small else 25),
                       draw(wg, c, case.biases), f32=True)
        sd.update(module_sd("p", ternary(wg, case.cout, c, case.nnz, 0).reshape(case.cout, c, 1, 1),
                            draw(wg, case.cout, case.biases)))
        x = _view(g, h, w, c, (0, 0))
        out = _view(g, h, w, case.out_c, case.out_at, case.cout)
        res = None
        if case.res:
            res = _view(g, h, w, case.out_c, (0, 0), case.cout)
            inputs[res.t] = int_data(case, "res", (n, h, w, case.out_c), case.cout)
        g.dwpw(sd, "d", "p", x, out, res=res, act=case.act)
        inputs[x.t] = int_data(case, "x", (n, h, w, c))
        inputs[out.t] = sentinel((n,) + g.tensors[out.t][:3])
        return Built(_finish(g), 1, 2, inputs, out.t, 1)
    if case.op == "ca":
        x = _view(g, h, w, case.cin, case.in_at)
        g.attention(_ca_sd(case, wg, case.cin), "a", x)
        inputs[x.t] = placed(int_data(case, "x", (n, h, w, case.cin)), case.in_at)
        return Built(_finish(g), 1, 2, inputs, x.t, 1)
    if case.op == "spp":
        c = case.cin
        buf = D.View(g.tensor(h, w, 4 * c), 0, 4 * c, np.arange(4 * c))
        g.poolings("spp", buf.sub(0, c))
        xd = normal_input((n, h, w, c), _seed(case.key, "x"))
        assert bool((xd != 0).all())  # fmaxf(-0, +0) is either: no zeros in the data
        inputs[buf.t] = placed(xd, (0, 4 * c))
        return Built(_finish(g), 1, 2, inputs, buf.t, 1)
    if case.op == "up2":
        x = _view(g, h, w, case.cin, case.in_at)
        out = _view(g, 2 * h, 2 * w, case.cin, case.out_at)
        g.up2(x, out)
        inputs[x.t] = placed(normal_input((n, h, w, case.cin), _seed(case.key, "x")), case.in_at)
        inputs[out.t] = sentinel((n, 2 * h, 2 * w, case.out_at[1]))
        return Built(_finish(g), 1, 2, inputs, out.t, 1)
    if case.op == "head":
        return _build_head(case, g)
    raise ValueError(case.op)


def build(case):
    """The case's Built; cases that share their data share it (it is not modified)."""
    return _build(case.key, case if case.random else BY_KEY[case.key])


HEAD_LEVELS = ((5, 32), (20, 8))


def _build_head(case, g):
    """Both levels in one size-160 detector (each with its own seeded weights); the case runs one of
    them, and the other's candidate rows must keep the sentinel."""
    f = case.cin // 2
    inputs, ops = {}, {}
    for h, stride in HEAD_LEVELS:
        lg = torch.Generator().manual_seed(_seed("head", f, h, stride))
        w = torch.cat([ternary(lg, 1, f, case.nnz, case.shift - 2), ternary(lg, 4, f, case.nnz, case.shift)]).numpy()
        if case.random:
            w = w / 4
        b = np.array([-1.0, 1.0, 0.0, 2.0, 1.0])
        x = _view(g, h, h, 2 * f, (0, 0))
        ops[(h, stride)] = len(g.ops)
        g.head(f"level-{stride}", w, b, x, stride)
        if (h, stride) == (case.h, case.stride):
            inputs[x.t] = int_data(case, "x", (case.n, h, h, 2 * f))
    k = ops[(case.h, case.stride)]
    s = g.size // 32
    assert s * 32 == g.size
    return Built(g, k, k + 1, inputs, -1, k)


def _ca_sd(case, g, c):
    """fc weights 0 or +-1 (nnz per output) and integer biases in [-2, 2]: with channel means of a
    few tenths, a + 3 lies mostly strictly inside (0, 6)."""
    if case.op == "conv" and not case.random:
        # in front of a conv: a + 3 >= 0.6 or so, so that no scale is tiny and bf16(x * s), whose
        # quantum is 2^-7 of its magnitude, keeps the conv's B / q below 2^20
        return {"a.fc.weight": ternary(g, c, c, 4, 0).reshape(c, c, 1, 1).float(), "a.fc.bias": draw(g, c, (0, 1))}
    bias = 1.0 + draw(g, c, None) if case.random else draw(g, c, BIASES)
    return {"a.fc.weight": ternary(g, c, c, case.nnz, 0).reshape(c, c, 1, 1).float(), "a.fc.bias": bias}


# ------------------------------------------------------------- reference --
class Expect:
    """What the device must hold.  want: bit patterns of the whole output tensor (int16 (n, h, w,
    c), the sentinel outside the view); lo / hi: for SiLU cases the bf16 values (float64) a got
    value may lie between where `und` is set (None otherwise).  stats: the CPU tests' figures.
    For head cases want is the f32 candidates' bit patterns (int32 (n, priors, 6)), with `rows`
    the level's rows, `score` / `box` float64."""

    def __init__(self, want, und=None, lo=None, hi=None, **stats):
        self.want, self.und, self.lo, self.hi, self.stats = want, und, lo, hi, stats


def blob_values(spec):
    wbits, fblob = spec.blobs()
    return (wbits.astype(np.uint32) << 16).view(np.float32).astype(np.float64), fblob.astype(np.float64)


def check_blobs(case, B):
    """After fold, to_bf16_bits and the f32 cast, every conv weight of the blobs is 0 or a dyadic
    value of the case (+-2^-shift; the depthwise taps' (t + 1) / 2^shift) and every bias an integer."""
    wf, fb = blob_values(B.spec)
    op = B.op
    if case.op == "conv":
        k, cp = op.ks, D.cout_pad(op.out.c)
        w = np.abs(wf[op.w_off:op.w_off + cp * k * k * op.in_.c])
        assert np.all((w == 0) | (w == 2.0 ** -case.shift)), (case.id, np.unique(w)[:8])
        b = fb[op.b_off:op.b_off + cp]
        assert np.array_equal(b, np.round(b)) and not np.any(np.signbit(b)[b == 0]), case.id
    elif case.op in ("stem", "dw", "dwpw"):
        nw = 32 * 36 if case.op == "stem" else op.in_.c * 25
        w = np.abs(fb[op.w_off:op.w_off + nw]) * 2.0 ** case.shift
        ok = (w == 0) | (w == 1) if case.op == "stem" or (case.op == "dwpw" and case.regime == "small") else \
            (w == np.round(w)) & (w <= 25)
        assert np.all(ok), (case.id, np.unique(w)[:8])
        nb = 32 if case.op == "stem" else op.in_.c * (2 if case.op == "dwpw" else 1)
        b = fb[op.b_off:op.b_off + nb]
        assert np.array_equal(b, np.round(b)), case.id
        if case.op == "dwpw":
            w = np.abs(wf[op.aux:op.aux + op.in_.c * op.in_.c])
            assert np.all((w == 0) | (w == 1)), case.id


def view_of(t, v):
    return t[..., v.coff:v.coff + v.c]


def conv_f64(x, w, stride, pad, groups=1):
    """x (n, h, w, c), w (cout, kh, kw, cin / groups) float64 -> (n, ho, wo, cout)."""
    y = F.conv2d(torch.from_numpy(np.ascontiguousarray(x)).permute(0, 3, 1, 2), torch.from_numpy(np.ascontiguousarray(w))
                 .permute(0, 3, 1, 2), stride=stride, padding=pad, groups=groups)
    return y.permute(0, 2, 3, 1).contiguous().numpy()


def exact_sum(name, x, w, b, res, stride, pad, groups=1, exact=True):
    """z = conv(x, w) + b (the residual is added by finish()), with the precondition asserted:
    every value a multiple of q, and B / q <= 2^20.  Returns (z, q, B / q).  exact=False: z alone."""
    if not exact:
        return conv_f64(x, w, stride, pad, groups) + b, None, None
    q = min(quantum(x) * quantum(w), quantum(b), quantum(res) if res is not None else float("inf"))
    z = conv_f64(x, w, stride, pad, groups) + b
    bound = conv_f64(np.abs(x), np.abs(w), stride, pad, groups) + np.abs(b) + (np.abs(res) if res is not None else 0.0)
    assert np.array_equal(np.round(z / q) * q, z), f"{name}: values are not multiples of {q}"
    if res is not None:
        assert np.array_equal(np.round(res / q) * q, res), f"{name}: residual is not a multiple of {q}"
    ratio = float(bound.max()) / q
    assert ratio <= LIMIT, f"{name}: B / q = {ratio:.3g} > 2^20"
    return z, q, ratio


def rounding_stats(r, want):
    changed = want != r
    r32 = r.astype(np.float32)
    assert np.array_equal(r32.astype(np.float64), r)
    ties = changed & ((np.ascontiguousarray(r32).view(np.uint32) & 0xFFFF) == 0x8000)
    return dict(numel=int(r.size), changed=int(changed.sum()), ties=int(ties.sum()))


def finish(z, res, act, relu_first=False, exact=True):
    """The epilogue on the exact pre-activation z: SiLU before the residual, ReLU after it.
    Returns (want values, und, lo, hi, stats).  relu_first: the wrong order (the CPU test's
    perturbation).  exact=False: the unrounded float64 result alone."""
    r0 = res if res is not None else 0.0
    if not exact:
        if act == SILU:
            return z / (1.0 + np.exp(-z)) + r0, None, None, None, {}
        return (np.maximum(z + r0, 0.0) if act == RELU else z + r0), None, None, None, {}
    if act == SILU:
        assert float(np.abs(z).max()) <= SILU_MAX, float(np.abs(z).max())
        s = z / (1.0 + np.exp(-z))
        r = s + r0
        wd = SILU_WIDTH * (np.abs(s) + np.abs(r0))
        lo, hi = bf16_round(r - wd), bf16_round(r + wd)
        und = lo != hi
        return bf16_round(r), und, lo, hi, dict(numel=int(r.size), undecidable=int(und.sum()))
    if act == RELU:
        r = np.maximum(z, 0.0) + r0 if relu_first else np.maximum(z + r0, 0.0)
    else:
        r = z + r0
    want = bf16_round(r)
    st = rounding_stats(r, want)
    if act == RELU and res is not None:
        st["relu_order"] = int((np.maximum(z, 0.0) + r0 != np.maximum(z + r0, 0.0)).sum())
    return want, None, None, None, st


def ca_scales(x, wt, b):
    """The attention kernels' arithmetic in numpy float32 on x (n, h, w, C) bf16 values: channel sums
    (integers, exact in any order), / HW, a = b[c], a = fmaf(wt[k][c], mean[k], a) for k = 0 .. C-1
    (wt[k][c] is 0 or a power of two, so the product is exact and the f32 add is the fma's one
    rounding), min(max(a + 3, 0), 6) / 6 -> (n, C) float32."""
    n, h, w, c = x.shape
    sums = x.reshape(n, h * w, c).sum(axis=1)
    assert np.array_equal(sums, np.round(sums)) and float(np.abs(sums).max()) < 2 ** 24
    mean = sums.astype(np.float32) / np.float32(h * w)
    wt = wt.astype(np.float32)
    m, e = np.frexp(np.abs(wt[wt != 0]))
    assert np.all(m == 0.5), "attention weights must be powers of two"
    a = np.broadcast_to(b.astype(np.float32), (n, c)).copy()
    for k in range(c):
        a = a + wt[k][None, :] * mean[:, k:k + 1]
        assert a.dtype == np.float32
    return np.minimum(np.maximum(a + np.float32(3), np.float32(0)), np.float32(6)) / np.float32(6), a


def ca_plain(x, wt, b):
    """The attention's definition in float64: hardsigmoid(W mean + b) -> (n, C)."""
    a = x.mean(axis=(1, 2)) @ wt + b
    return np.clip(a + 3.0, 0.0, 6.0) / 6.0


def ca_apply(x, s):
    """bf16(f32(x) * s) as float64 (n, h, w, C); signed zeros kept."""
    p = x.astype(np.float32) * s[:, None, None, :]
    return torch.from_numpy(p).bfloat16().double().numpy()


def _ca_params(spec, op):
    _, fb = blob_values(spec)
    c = op.in_.c
    return fb[op.w_off:op.w_off + c * c].reshape(c, c), fb[op.b_off:op.b_off + c]


@functools.lru_cache(maxsize=None)
def _reference(key, case, perturb=None):
    B = build(case)
    spec, op = B.spec, B.op
    exact = not case.random
    if exact:
        check_blobs(case, B)
    wf, fb = blob_values(spec)
    T = {t: bits_f64(x) for t, x in B.inputs.items()}
    stats = {}
    if case.op == "head":
        return _head_reference(case, B, T, fb, exact)
    out_v = op.out if op.out.t >= 0 else op.in_
    full = B.inputs[B.out_t].view(torch.int16).numpy().copy()
    und = lo = hi = None
    if case.op in ("conv", "stem"):
        k, cout = op.ks, op.out.c
        if case.op == "stem":
            x = T[op.in_.t]
            w = fb[op.w_off:op.w_off + 32 * 36].reshape(32, 3, 3, 4)
            b = fb[op.b_off:op.b_off + 32]
        else:
            x = view_of(T[op.in_.t], op.in_).copy()
            cp = D.cout_pad(cout)
            w = wf[op.w_off:op.w_off + cp * k * k * op.in_.c].reshape(cp, k, k, op.in_.c)[:cout]
            b = fb[op.b_off:op.b_off + cout]
            if case.fold == "up":
                u = spec.ops[B.op_index - 1]
                src = view_of(T[u.in_.t], u.in_)
                x[..., :u.out.c] = src.repeat(2, axis=1).repeat(2, axis=2)
            elif case.fold == "ca":
                a_op = spec.ops[B.begin]
                if exact:
                    s, pre = ca_scales(x, *_ca_params(spec, a_op))
                    stats.update(scales_inside=int(((s > 0) & (s < 1)).sum()), scales=int(s.size))
                    x = ca_apply(x, s)
                else:
                    x = x * ca_plain(x, *_ca_params(spec, a_op))[:, None, None, :]
        assert not np.isnan(x).any(), "the op reads a sentinel"
        if perturb == "tap":      # one tap of one cout dropped
            w = w.copy()
            co, kh, kw, ci = np.argwhere(w != 0)[0]
            w[co, kh, kw, ci] = 0
        if perturb == "halo":     # one input column taken from its neighbour
            x = x.copy()
            x[:, :, 0] = x[:, :, 1]
        res = view_of(T[op.res.t], op.res) if op.res.t >= 0 else None
        z, q, ratio = exact_sum(case.id, x, w, b, res, op.stride, k // 2, exact=exact)
        stats.update(q=q, ratio=ratio)
        want, und, lo, hi, st = finish(z, res, op.act, relu_first=perturb == "relu", exact=exact)
        if not exact:
            return want, None
        stats.update(st)
        real = np.zeros(cout, bool)
        real[:case.cout] = True
        stats["padding_zero"] = bool(np.all(want[..., ~real] == 0))
        stats["constant"] = [int(c) for c in np.flatnonzero(real) if want[..., c].min() == want[..., c].max()]
    elif case.op == "dw":
        c = op.in_.c
        x = view_of(T[op.in_.t], op.in_)
        w = fb[op.w_off:op.w_off + c * 25].reshape(c // 8, 25, 8).transpose(0, 2, 1).reshape(c, 5, 5, 1)
        if perturb == "tap":      # two taps swapped
            w = w.copy()
            w[0, 0, 0], w[0, 0, 1] = w[0, 0, 1].copy(), w[0, 0, 0].copy()
        z, q, ratio = exact_sum(case.id, x, w, fb[op.b_off:op.b_off + c], None, 1, 2, groups=c, exact=exact)
        if not exact:
            return finish(z, None, op.act, exact=False)[0], None
        stats.update(q=q, ratio=ratio, taps=int((w != 0).reshape(c, 25).sum(axis=1).min()),
                     magnitudes=int(min(len(np.unique(np.abs(w[ch]))) for ch in range(c))))
        want, und, lo, hi, st = finish(z, None, op.act)
        stats.update(st)
    elif case.op == "dwpw":
        c, cout = op.in_.c, op.out.c
        x = view_of(T[op.in_.t], op.in_)
        wd = fb[op.w_off:op.w_off + c * 25].reshape(c // 8, 25, 8).transpose(0, 2, 1).reshape(c, 5, 5, 1)
        z, q, ratio = exact_sum(case.id + " dw", x, wd, fb[op.b_off:op.b_off + c], None, 1, 2, groups=c, exact=exact)
        assert op.act != SILU
        # the intermediate, rounded to bf16 as the unfused pair stores it
        t, _, _, _, st = finish(z, None, op.act, exact=exact)
        wp = wf[op.aux:op.aux + D.cout_pad(cout) * c].reshape(-1, 1, 1, c)[:cout]
        res = view_of(T[op.res.t], op.res) if op.res.t >= 0 else None
        z2, q2, ratio2 = exact_sum(case.id + " pw", t, wp, fb[op.b_off + c:op.b_off + c + cout], res, 1, 0, exact=exact)
        if not exact:
            return finish(z2, res, op.act, exact=False)[0], None
        stats.update(mid_changed=st["changed"], mid_numel=st["numel"])
        stats.update(q=q2, ratio=max(ratio, ratio2))
        want, und, lo, hi, st = finish(z2, res, op.act, relu_first=perturb == "relu")
        stats.update(st)
        stats["padding_zero"] = bool(np.all(want[..., case.cout:] == 0))
    elif case.op == "ca":
        x = view_of(T[op.in_.t], op.in_)
        if not exact:
            return x * ca_plain(x, *_ca_params(spec, op))[:, None, None, :], None
        s, pre = ca_scales(x, *_ca_params(spec, op))
        stats.update(scales_inside=int(((s > 0) & (s < 1)).sum()), scales=int(s.size), scales_zero=int((s == 0).sum()))
        y = ca_apply(x, s)
        view_of(full, out_v)[...] = torch.from_numpy(y).bfloat16().view(torch.int16).numpy()
        return Expect(full, **stats), s
    elif case.op == "spp":
        c = op.in_.c
        x = torch.from_numpy(T[op.in_.t][..., :c].copy()).permute(0, 3, 1, 2)
        for j in range(1, 4):     # max pools of 5, 9, 13 = the 5x5 max applied 1, 2, 3 times (-inf padding)
            x = F.max_pool2d(x, 5, 1, 2)
            full[..., j * c:(j + 1) * c] = bf16_bits(x.permute(0, 2, 3, 1).numpy())
        return Expect(full, **stats), None
    elif case.op == "up2":
        src = view_of(B.inputs[op.in_.t].view(torch.int16).numpy(), op.in_)
        view_of(full, out_v)[...] = src.repeat(2, axis=1).repeat(2, axis=2)
        return Expect(full, **stats), None
    view_of(full, out_v)[...] = bf16_bits(want)
    if und is not None:
        U = np.zeros(full.shape, bool)
        L, H = np.zeros(full.shape), np.zeros(full.shape)
        view_of(U, out_v)[...] = und
        view_of(L, out_v)[...] = lo
        view_of(H, out_v)[...] = hi
        und, lo, hi = U, L, H
    return Expect(full, und, lo, hi, **stats), None


def _head_reference(case, B, T, fb, exact=True):
    """Logits exact (integer features, dyadic weights: any order gives the same f32 number);
    scores and boxes in float64 from the definition (sigmoid; distance2bbox of exp(reg) * stride
    around the prior (x, y) * stride, clipped to [0, size])."""
    spec, op = B.spec, B.op
    x = T[op.in_.t]
    n, h, w, c2 = x.shape
    f = c2 // 2
    wt, b = fb[op.w_off:op.w_off + 5 * f].reshape(5, f), fb[op.b_off:op.b_off + 5]
    q = quantum(wt) * quantum(x)
    cls = x[..., :f] @ wt[0] + b[0]
    reg = x[..., f:] @ wt[1:].T + b[1:]
    bound = max(float((np.abs(x[..., :f]) @ np.abs(wt[0])).max()), float((np.abs(x[..., f:]) @ np.abs(wt[1:]).T).max())) + 2
    if exact:
        assert bound / q <= LIMIT
        assert np.array_equal(cls.astype(np.float32).astype(np.float64), cls)
    s = float(op.stride)
    ys, xs = np.meshgrid(np.arange(h) * s, np.arange(w) * s, indexing="ij")
    d = np.exp(reg) * s
    raw = np.stack([xs - d[..., 0], ys - d[..., 1], xs + d[..., 2], ys + d[..., 3]], -1)
    box = np.clip(raw, 0.0, float(spec.size))
    want = np.full((n, spec.n_priors, 6), SENT32, np.int32)
    rows = slice(int(op.aux), int(op.aux) + h * w)
    want[:, rows, 5] = np.ascontiguousarray(cls.astype(np.float32).reshape(n, -1)).view(np.int32)
    e = Expect(want, ratio=bound / q, q=q, clamped=int((box != raw).sum()), unclamped=int((box == raw).sum()),
               boxes=int(box.size))
    e.logit = cls.reshape(n, -1)
    e.rows, e.score, e.box = rows, (1.0 / (1.0 + np.exp(-cls))).reshape(n, -1), box.reshape(n, -1, 4)
    return e, None


def reference(case, perturb=None):
    """The case's Expect, computed once per data key and shared; do not modify.  perturb: "tap" |
    "halo" | "relu", a deliberately wrong reference (the CPU test shows that it differs)."""
    return _reference(case.key, case if case.random else BY_KEY[case.key], perturb)[0]


def scales(case):
    """The (n, C) float32 attention scales of a ca case."""
    return _reference(case.key, BY_KEY[case.key])[1]


def mismatches(got_bits, e):
    """Boolean array: where the device's bit patterns are not what `e` allows."""
    bad = got_bits != e.want
    if e.und is not None:
        g = bits_f64(np.ascontiguousarray(got_bits))
        with np.errstate(invalid="ignore"):
            bad &= ~(e.und & (g >= e.lo) & (g <= e.hi))
    return bad


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
BY_KEY = {}
_DATA = [k for k in Case._DEFAULTS if k not in ("env", "direct")]
for _c in CASES:   # cases that share a key share their data: they differ in switches alone
    _o = BY_KEY.setdefault(_c.key, _c)
    assert all(getattr(_o, k) == getattr(_c, k) for k in _DATA), (_o, _c)
FAMILIES = sorted({c.family for c in CASES})
CONV_VARIANTS = ("band_8w", "band_4w", "halo_2row", "halo", "halo_live3", "halo_pers_lt2", "halo_pers_lt3",
                 "halo_pers_lt4", "fold_up", "fold_ca", "pers_gemm", "gemm")
OTHER_VARIANTS = ("stem", "dw5", "dwpw", "ca_pool", "spp", "up2", "head_staged", "head_direct")
