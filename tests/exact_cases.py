"""Exactly summable data for the HRNet conv kernels, and a float64 reference of every spec helper.

If every weight and activation of a conv is a multiple of a power-of-two quantum q and every
partial sum stays below 2^24 q, every f32 partial sum is exact in any order, so the conv's bf16
result is ONE array whatever the MFMA K order, split, tile shape or fusion: a float64 conv on
the CPU gives it and the device must match it bit for bit (tests/test_exact_conv_gpu.py;
tests/test_exact_cases.py checks this module's own claims on the CPU).

The reference asserts the precondition at every conv and fuse sum: all values are multiples of
q, and B / q <= LIMIT = 2^20, where q = input quantum x weight quantum (bias and residual
included; never refined by the bf16 rounding) and B = max(conv2d(|x|, |w|) + |bias| + |res|)
bounds every partial sum in every order.  2^24 is what f32's significand holds; the factor 16
below it is margin for alignment inside the MFMA, which nobody had measured.  Measured with these
cases on an MI355X: every kernel family is exact on every case, the largest B / q among them being
317,406 (block-64x64x48-rounding, b1.conv2), so the bound stands as set.

Two regimes, chosen per case through (nnz, shift):
  small     shift = 0 and few non-zeros: every activation is an integer with |v| <= 256, which
            bf16 holds exactly, so the reference is the plain float64 forward whichever fusion ran
  rounding  denser weights of +-2^-shift: bf16 rounding, ties included, really happens, at the
            tensor boundaries of the device graph (a cat-fused downsample stays unrounded)
and, for the fuse layers, selection weights: one +-1 on the centre tap per output channel, so a
conv output is a signed copy of input values for ANY finite input and the only arithmetic left
is the fuse sum's f32 adds in term order.

Biases are integers in [-2, 2], drawn uniformly except behind the ReLU of the bias-carried
rounding cases (see ROUNDING).  A few cases move their weight seed on (SALT) until no output
channel is constant; test_exact_cases.py holds every case to the conditions, so a changed table
that breaks one fails there, on the CPU.

CASES is the one table both test files walk.
"""
import collections
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

LIMIT = 2.0 ** 20
SMALL_MAX = 256
FUSE_CHANNELS = (32, 64, 128, 256)


# ------------------------------------------------------------------ data --
def _seed(*parts):
    return zlib.crc32(repr(parts).encode())


def _conv_keys(sd):
    return [k[:-len(".weight")] for k, v in sd.items() if k.endswith(".weight") and v.dim() == 4]


def _bn_keys(sd):
    return [k[:-len(".running_mean")] for k in sd if k.endswith(".running_mean")]


def _plain_bn(out, bn, bias, f32):
    """weight 1, mean 0, var 1 (or 1 - eps, so that an f32 weight folds to itself exactly)."""
    c = out[bn + ".weight"].shape[0]
    out[bn + ".weight"] = torch.ones(c)
    out[bn + ".running_mean"] = torch.zeros(c)
    out[bn + ".running_var"] = torch.full((c,), 1.0 - 1e-5 if f32 else 1.0)
    out[bn + ".bias"] = bias


BIASES = (-2, -1, 0, 1, 2)


def exact_state_dict(sd, seed, nnz, shift, f32_bn=(), biases=BIASES):
    """A copy of a spec helper's state dict with every conv weight ternary — nnz non-zeros per
    output channel (all of them where the fan-in is smaller) at seeded (ci, tap) positions,
    values +-2^-shift — every BatchNorm weight 1, mean 0, var 1 and a seeded integer bias in
    [-2, 2], and every conv bias such an integer.  fold_bn's scale 1 / sqrt(1 + 1e-5) vanishes
    when the weight is rounded to bf16; the BatchNorms named in f32_bn (the stem's, whose conv
    keeps f32 weights) get var 1 - 1e-5 instead, so that their scale rounds to 1 in f32.
    biases: the integers a bias is drawn from (uniformly, with repetition as listed)."""
    g = torch.Generator().manual_seed(seed)
    pool = torch.tensor(biases, dtype=torch.float32)

    def draw(c):
        return pool[torch.randint(0, len(biases), (c,), generator=g)]

    out = {k: v.clone() for k, v in sd.items()}
    for conv in _conv_keys(sd):
        w = sd[conv + ".weight"]
        co, fan = w.shape[0], w[0].numel()
        new = torch.zeros((co, fan))
        for o in range(co):
            pos = torch.randperm(fan, generator=g)[:min(nnz, fan)]
            sign = torch.randint(0, 2, (pos.numel(),), generator=g) * 2.0 - 1.0
            new[o, pos] = sign * 2.0 ** -shift
        out[conv + ".weight"] = new.reshape(w.shape)
        if conv + ".bias" in sd:
            out[conv + ".bias"] = draw(co)
    for bn in _bn_keys(sd):
        c = sd[bn + ".weight"].shape[0]
        _plain_bn(out, bn, draw(c), bn in f32_bn)
    return out


def selection_state_dict(sd, seed):
    """Every conv gets exactly one non-zero weight per output channel: +-1 on the centre tap at
    a seeded input channel, bias 0 — each conv output is then an exact signed copy of input
    values, for any finite input."""
    g = torch.Generator().manual_seed(seed)
    out = {k: v.clone() for k, v in sd.items()}
    for conv in _conv_keys(sd):
        w = sd[conv + ".weight"]
        co, ci, k, _ = w.shape
        new = torch.zeros(w.shape)
        src = torch.randint(0, ci, (co,), generator=g)
        sign = torch.randint(0, 2, (co,), generator=g) * 2.0 - 1.0
        new[torch.arange(co), src, k // 2, k // 2] = sign
        out[conv + ".weight"] = new
        if conv + ".bias" in sd:
            out[conv + ".bias"] = torch.zeros(co)
    for bn in _bn_keys(sd):
        _plain_bn(out, bn, torch.zeros(sd[bn + ".weight"].shape[0]), False)
    return out


def exact_input(shape, seed):
    """Integers in [-3, 3] as bf16 NHWC; a 4-channel (stem) input has its 4th channel zero."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-3, 4, tuple(shape), generator=g).float()
    if shape[-1] == 4:
        x[..., 3] = 0
    return x.bfloat16()


def normal_input(shape, seed):
    """Random normal bf16 NHWC, each element times a seeded power of two in 2^-16 .. 2^16:
    ordinary non-integer data.  Plain N(0, 1) values would not do: three or four bf16 numbers
    within 16 binades of each other add exactly in f32 (8-bit significands), so every order of
    a fuse sum would give the same bits and the test could not pin the order.  With the spread,
    f32 adds round, and a small term decides a bf16 tie in one order and is lost in another."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(tuple(shape), generator=g) * 2.0 ** torch.randint(-16, 17, tuple(shape), generator=g)
    return x.bfloat16()


def quantum(a):
    """The largest power of two that divides every value of a (inf if all are zero)."""
    v = np.abs(np.asarray(a, np.float64).ravel())
    v = v[v != 0]
    if v.size == 0:
        return float("inf")
    m, e = np.frexp(v)
    mi = (m * 2.0 ** 53).astype(np.int64)
    low = mi & -mi  # lowest set bit of the 53-bit significand
    return float(np.min(np.ldexp(low.astype(np.float64), e - 53)))


# ------------------------------------------------------------- reference --
T = collections.namedtuple("T", "v q")  # NCHW values and their quantum


class Ref:
    """Float64 reference ops over a state dict, recording what the CPU tests check.

    exact=True asserts the precondition at every conv and fuse sum.  dtype=torch.float32 with
    permute_seed runs the same forward in f32 with every conv's input channels permuted (the
    order-independence demonstration).  rounding=False, bf16_weights=False: the unrounded
    forward on ordinary weights that is compared with the oracle."""

    def __init__(self, sd, dtype=torch.float64, exact=True, rounding=True, bf16_weights=True, permute_seed=None):
        self.sd, self.dtype, self.exact, self.rounding, self.bf16_weights = sd, dtype, exact, rounding, bf16_weights
        self.gen = None if permute_seed is None else torch.Generator().manual_seed(permute_seed)
        self.convs = []     # (name, q, B)
        self.tensors = []   # (name, values, relu)
        self.rounded = []   # (name, elements, changed, ties)

    def input(self, x_nhwc):
        v = x_nhwc.to(self.dtype).permute(0, 3, 1, 2).contiguous()
        return T(v, quantum(v.numpy()) if self.exact else 1.0)

    def _weights(self, conv, bn, f32_weights):
        from mvpose import hrnet
        w, b = hrnet.fold_bn(self.sd, conv, bn)  # (cout, k, k, cin) f64
        if f32_weights:
            w = np.ascontiguousarray(w, dtype=np.float32).astype(np.float64)
        elif self.bf16_weights:
            w = hrnet.to_bf16_bits(w).astype(np.uint32) << 16
            w = w.view(np.float32).astype(np.float64)
        if self.bf16_weights:
            b = np.asarray(b, np.float32).astype(np.float64)
        return torch.from_numpy(np.ascontiguousarray(w.transpose(0, 3, 1, 2))), torch.from_numpy(b)

    def _finish(self, name, z, q, bound, relu, rounding):
        if self.exact:
            assert torch.equal(torch.round(z / q) * q, z), f"{name}: values are not multiples of {q}"
            assert bound / q <= LIMIT, f"{name}: B / q = {bound / q:.3g} > 2^20"
            self.convs.append((name, q, bound))
        if relu:
            z = torch.relu(z)
        if rounding and self.rounding:
            z32 = z.float()
            r = z32.bfloat16().float()
            changed = r != z32
            ties = changed & ((z32.view(torch.int32) & 0xFFFF) == 0x8000)
            self.rounded.append((name, z.numel(), int(changed.sum()), int(ties.sum())))
            z = r.to(self.dtype)
        z = z + 0.0  # no negative zero: every accumulator starts at +0, so no sum can be one
        self.tensors.append((name, z, bool(relu)))
        return T(z, q)

    def conv(self, x, conv, bn, stride=1, relu=False, res=None, rounding=True, f32_weights=False):
        """conv2d + folded-BN bias (+ residual) (+ ReLU), then bf16 rounding unless rounding=False."""
        w, b = self._weights(conv, bn, f32_weights)
        k = w.shape[-1]
        xv = x.v[:, :w.shape[1]]  # the stem reads 3 of its input's 4 channels
        q = bound = None
        if self.exact:
            q = min(x.q * quantum(w.numpy()), quantum(b.numpy()), res.q if res is not None else float("inf"))
            bound = F.conv2d(xv.abs(), w.abs(), stride=stride, padding=k // 2) + b.abs()[None, :, None, None]
            bound = float((bound + (res.v.abs() if res is not None else 0)).max())
        w, b = w.to(self.dtype), b.to(self.dtype)
        if self.gen is not None:
            perm = torch.randperm(w.shape[1], generator=self.gen)
            xv, w = xv[:, perm].contiguous(), w[:, perm].contiguous()
        z = F.conv2d(xv, w, stride=stride, padding=k // 2) + b[None, :, None, None]
        if res is not None:
            z = z + res.v
        return self._finish(conv, z, q, bound, relu, rounding)

    def fuse(self, terms, relu=True, reverse=False, name="fuse"):
        """act(((0 + up(t0)) + up(t1)) + ...) in self.dtype, in term order, then bf16 rounding."""
        ups = [upsample(t.v, u) for t, u in terms]
        z = torch.zeros_like(ups[0])
        for u in (reversed(ups) if reverse else ups):
            z = z + u
        q = bound = None
        if self.exact:
            q = min(t.q for t, _ in terms)
            bound = float(sum(u.abs() for u in ups).max())
        return self._finish(name, z, q, bound, relu, True)


def upsample(v, factor):
    """Nearest upsample of NCHW by an integer factor."""
    return v if factor == 1 else v.repeat_interleave(factor, dim=2).repeat_interleave(factor, dim=3)


def fuse_layer_ref(R, xs, i, relu=True, reverse=False, p="mod"):
    """Fuse layer i of an HRModule on branch tensors xs, restated from mmpose's definition:
    relu(sum_j f_ij(x_j)) in order j = 0..n-1, f_ii the identity, f_ij (j > i) a 1x1 conv + BN
    then nearest upsampling by 2^(j-i), f_ij (j < i) i - j 3x3/s2 conv + BN, ReLU between."""
    terms = []
    for j, x in enumerate(xs):
        q = f"{p}.fuse_layers.{i}.{j}"
        if j > i:
            terms.append((R.conv(x, q + ".0", q + ".1"), 2 ** (j - i)))
        elif j == i:
            terms.append((x, 1))
        else:
            for k in range(i - j):
                x = R.conv(x, f"{q}.{k}.0", f"{q}.{k}.1", stride=2, relu=k < i - j - 1)
            terms.append((x, 1))
    return R.fuse(terms, relu, reverse)


def lead_in(R, x, n, lead_relu):
    xs = [x]
    for j in range(1, n):
        xs.append(R.conv(xs[-1], f"lead.{j}.0", f"lead.{j}.1", stride=2, relu=lead_relu))
    return xs


def cat_fused(cin, k):
    """Whether the graph folds projection_spec's conv_a into conv_b (cat-fusion: 1x1 convs whose
    concatenated K is 64, 128 or 256); conv_a's output is then never rounded to bf16."""
    return k == 1 and 2 * cin // 32 in (2, 4, 8)


def forward(case, R, x, reverse=False):
    """The case's graph on NHWC input x through R; returns the output T (NCHW)."""
    a = case.args
    x = R.input(x)
    if case.kind == "block":
        for k in range(2):
            t = R.conv(x, f"b{k}.conv1", f"b{k}.bn1", relu=True)
            x = R.conv(t, f"b{k}.conv2", f"b{k}.bn2", relu=True, res=x)
        return x
    if case.kind == "s2":
        return R.conv(x, "c", "bn", stride=2, relu=a[4])
    if case.kind == "sibling":
        name, relu = (("s1", False), ("s2", True), ("s3", True))[a[1]]
        return R.conv(x, name, name + "bn", stride=2, relu=relu)
    if case.kind == "projection":
        t = R.conv(x, "a", "abn", rounding=not cat_fused(a[0], a[4]))
        return R.conv(x, "b", "bbn", relu=True, res=t)
    if case.kind == "join":
        r = R.conv(x, "r", "rbn", relu=not a[0], rounding=not a[0])
        y = R.conv(x, "a", "abn", relu=True, res=r)
        return R.conv(y, "b", "bbn", relu=True)
    if case.kind == "bottleneck":
        n_blocks, lead = a
        for b in range(n_blocks):
            first = lead and b == 0
            idn = R.conv(x, f"b{b}.ds", f"b{b}.dsbn", rounding=False) if first else x
            y = R.conv(x, f"b{b}.conv1", f"b{b}.conv1bn", relu=True)
            y = R.conv(y, f"b{b}.conv2", f"b{b}.conv2bn", relu=True)
            x = R.conv(y, f"b{b}.conv3", f"b{b}.conv3bn", relu=True, res=idn)
        return x
    if case.kind == "stem":
        y = R.conv(x, "backbone.conv1", "backbone.bn1", stride=2, relu=True, f32_weights=True)
        return R.conv(y, "backbone.conv2", "backbone.bn2", stride=2, relu=True)
    if case.kind == "transition":
        name = ("t0", "t1")[a[0]]
        return R.conv(x, name, name + "bn", stride=1 + a[0], relu=True)
    if case.kind in ("fuse", "fusesel", "head"):
        n, i = a[0], a[1]
        relu = a[2] if case.kind == "fuse" else True
        y = fuse_layer_ref(R, lead_in(R, x, n, case.kind == "fuse" or case.regime != "selection"), i, relu, reverse)
        if case.kind == "head" and case.regime != "selection":
            y = R.conv(y, "head.final_layer", None, rounding=False)
        return y
    raise ValueError(case.kind)


def head_chain(fused_nhwc, w, bias):
    """The heatmap head as its kernels compute it: per pixel and joint, acc = bias, then
    acc = f32(acc + f32(w[c] * x[c])) for c = 0..31 (the product of two bf16 values is exact
    in f32, so an fma rounds once, like this).  fused_nhwc (n, h, w, 32) bf16-valued, w (17, 32)
    bf16-valued, bias (17,) -> (n, 17, h, w) float32."""
    x = np.ascontiguousarray(fused_nhwc, dtype=np.float32)
    n, h, ww, c = x.shape
    x = x.reshape(n, 1, h * ww, c)
    w = np.asarray(w, np.float32).reshape(1, -1, 1, c)
    acc = np.broadcast_to(np.asarray(bias, np.float32).reshape(1, -1, 1), (n, w.shape[1], h * ww)).copy()
    for k in range(c):
        prod = (w[..., k] * x[..., k]).astype(np.float32)
        acc = (acc + prod).astype(np.float32)
    return acc.reshape(n, -1, h, ww)


# ----------------------------------------------------------------- cases --
# kind       args
# block      (c, h, w): two BasicBlocks                     basic_block_spec
# s2         (cin, cout, h, w, relu): one 3x3/s2 conv        conv_spec
# sibling    (n, output)                                     sibling_spec
# projection (cin, cout, h, w, k)                            projection_spec
# join       (cat,)                                          join_spec
# bottleneck (n_blocks, lead)                                bottleneck_spec
# stem       ()                                              stem_spec
# transition (output,)                                       transition_spec
# fuse       (n_branches, output, relu)                      fuse_layer_spec
# fusesel    (n_branches, output): selection weights, lead_relu=False, random normal input
# head       (n_branches, 0): fuse_layer_spec(head=True); regime "selection" = selection fuse
#            weights, ordinary head weights, random normal input (head_chain)
Case = collections.namedtuple("Case", "id kind args regime nnz shift biases batch")

BLOCK_PLANES = [(32, 64, 48), (64, 32, 24), (128, 16, 12), (256, 8, 6), (64, 64, 48)]
S2_PLANES = [(64, 64, 128, 96, True), (256, 64, 64, 48, True), (32, 64, 64, 48, False),
             (32, 128, 32, 24, False), (64, 128, 32, 24, True), (64, 64, 32, 24, True),
             (32, 256, 16, 12, False), (64, 256, 16, 12, False), (128, 256, 16, 12, True)]
PROJECTIONS = [(64, 256, 64, 48, 1), (256, 64, 64, 48, 1), (64, 64, 64, 48, 1), (64, 32, 32, 24, 1),
               (128, 64, 16, 12, 1), (256, 128, 8, 6, 1), (256, 32, 64, 48, 3)]
FUSE_LAYERS = [(n, i) for n in (2, 3, 4) for i in range(n)]

# (nnz, shift) per regime; see test_exact_cases.py for what each must satisfy
SMALL = {"block": (4, 0), "s2": (8, 0), "sibling": (8, 0), "projection": (6, 0), "join": (6, 0),
         "bottleneck": (2, 0), "stem": (8, 0), "transition": (8, 0), "fuse": (6, 0), "head": (6, 0)}
# A single conv of integers in [-3, 3] cannot reach 256 quanta through its taps: the sum of N such
# terms has a standard deviation of 2 sqrt(N) quanta, 34 for a 3x3 conv of 32 channels.  There the
# bias carries the value past bf16's 8 bits: with shift = 8 a bias of 1 is 256 quanta and one of 2
# is 512, so bias + sum needs one or two bits more than bf16 has, ties and non-ties both.  Such a
# value is its bias +- 0.6 at the most, so behind a ReLU a negative bias would leave a channel
# constant zero whatever nnz and shift are (the sum would have to reach 256 quanta again); those
# cases draw their biases from ONE (a single BatchNorm in front of the ReLU) or TWO (the sum of two),
# which keep every channel alive and 20-80 % of the outputs positive.
ONE, TWO = (0, 0, 0, 1, 2), (0, 0, 0, 1)
ROUNDING = {"block": (144, 3), "s2": (144, 8), "sibling": (144, 8), "projection": (48, 8, TWO), "join": (48, 3),
            "bottleneck": (48, 3), "stem": (144, 3), "transition": (144, 8, ONE), "fuse": (144, 3)}
OVERRIDE = {"fuse-2x1x1-rounding": (144, 8, TWO), "bottleneck-4x0-small": (3, 0)}
# weight seeds moved on until no output channel is constant (test_exact_cases.py checks it)
SALT = {"block-256x8x6-small": 5, "join-1-small": 2, "bottleneck-4x1-small": 2, "bottleneck-4x0-small": 47, "stem-small": 1,
        "bottleneck-1x0-rounding": 1, "stem-rounding": 2, "fuse-4x3x1-rounding": 17, "fusesel-3x2-selection": 4,
        "fusesel-4x3-selection": 12}


def _mk(kind, args, regime, batch, tag=""):
    par = {"small": SMALL, "rounding": ROUNDING}.get(regime, {}).get(kind, (0, 0))
    name = f"{kind}-{'x'.join(str(int(v)) for v in args)}{tag}-{regime}".replace("--", "-")
    par = OVERRIDE.get(name, par)
    if regime == "rounding" and len(par) == 2 and (kind == "s2" and args[4] or kind == "sibling" and args[1] > 0):
        par += (ONE,)  # the single convs with a ReLU
    nnz, shift, biases = par if len(par) == 3 else par + (BIASES,)
    return Case(name, kind, tuple(args), regime, nnz, shift, biases, batch)


def _cases():
    out = []
    for regime in ("small", "rounding"):
        out += [_mk("block", p, regime, 5) for p in BLOCK_PLANES]
        out += [_mk("s2", p, regime, 5) for p in S2_PLANES]
        out += [_mk("sibling", (n, o), regime, 3) for n in (3, 2) for o in range(n)]
        out += [_mk("projection", p, regime, 3) for p in PROJECTIONS]
        out += [_mk("join", (cat,), regime, 3) for cat in (False, True)]
        out += [_mk("bottleneck", (4 if regime == "small" else 1, lead), regime, 3) for lead in (True, False)]
        out += [_mk("stem", (), regime, 3)]
        out += [_mk("transition", (o,), regime, 3) for o in (0, 1)]
        out += [_mk("fuse", (n, i, True), regime, 3) for n, i in FUSE_LAYERS]
        out += [_mk("fuse", (4, i, False), regime, 3) for i in (0, 3)]
    out += [_mk("fusesel", (n, i), "selection", 3) for n, i in FUSE_LAYERS]
    out += [_mk("head", (n, 0), "selection", 3) for n in (4, 2)]
    out += [_mk("head", (n, 0), "small", 3) for n in (4, 2)]
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
# the crop-streaming kernels also run one batch of CU count + 3 crops, 8 distinct crops tiled
TILED = {"tblock32s": "block-32x64x48-rounding", "stem2": "stem-rounding"}
TILE_CROPS = 8


def in_shape(case):
    a = case.args
    return {"block": lambda: (a[1], a[2], a[0]), "s2": lambda: (a[2], a[3], a[0]), "sibling": lambda: (64, 48, 32),
            "projection": lambda: (a[2], a[3], a[0]), "join": lambda: (64, 48, 64),
            "bottleneck": lambda: (64, 48, 64 if a[1] else 256), "stem": lambda: (256, 192, 4),
            "transition": lambda: (64, 48, 256)}.get(case.kind, lambda: (64, 48, 32))()


def spec(case, sd=None):
    """The case's (GraphSpec, input id, output id, state dict) from its spec helper."""
    from mvpose import hrnet
    a = case.args
    if case.kind == "block":
        return hrnet.basic_block_spec(*a, n_blocks=2, sd=sd)
    if case.kind == "s2":
        return hrnet.conv_spec(a[0], a[1], a[2], a[3], k=3, stride=2, relu=a[4], sd=sd)
    if case.kind == "sibling":
        return hrnet.sibling_spec(output=a[1], n=a[0], sd=sd)
    if case.kind == "projection":
        return hrnet.projection_spec(*a[:4], k=a[4], sd=sd)
    if case.kind == "join":
        return hrnet.join_spec(64, 48, cat=a[0], sd=sd)
    if case.kind == "bottleneck":
        return hrnet.bottleneck_spec(n_blocks=a[0], lead=a[1], sd=sd)
    if case.kind == "stem":
        return hrnet.stem_spec(sd=sd)
    if case.kind == "transition":
        return hrnet.transition_spec(output=a[0], sd=sd)
    if case.kind == "fuse":
        return hrnet.fuse_layer_spec(a[0], a[1], relu=a[2], sd=sd)
    if case.kind == "fusesel":
        return hrnet.fuse_layer_spec(a[0], a[1], lead_relu=False, sd=sd)
    if case.kind == "head":
        return hrnet.fuse_layer_spec(a[0], 0, head=True, lead_relu=case.regime != "selection", sd=sd)
    raise ValueError(case.kind)


def check_folded(case, sd):
    """After folding (fold_bn, then bf16 for the conv blob, f32 for the stem's weights and the
    biases) every weight is exactly 0 or +-2^-shift and every bias an integer."""
    w, f = spec(case, sd)[0].blobs()
    unit = 2.0 ** -case.shift
    wv = np.abs((w.astype(np.uint32) << 16).view(np.float32))
    assert np.all((wv == 0) | (wv == unit)), f"{case.id}: folded bf16 weights {np.unique(wv)[:8]}"
    fv = np.abs(f)
    assert np.all((fv == unit) | (fv == np.round(fv))), f"{case.id}: folded f32 values {np.unique(fv)[:8]}"


@functools.lru_cache(maxsize=None)
def weights(case):
    """The case's state dict: the helper's template, rewritten for the case's regime."""
    template = spec(case)[3]
    if case.regime == "selection":
        sd = selection_state_dict(template, _seed(case.id, "w", SALT.get(case.id, 0)))
        if case.kind == "head":  # ordinary head weights (bf16-valued), f32 bias
            sd["head.final_layer.weight"] = template["head.final_layer.weight"].bfloat16().float()
            sd["head.final_layer.bias"] = template["head.final_layer.bias"].clone()
        else:
            check_folded(case, sd)
        return sd
    sd = exact_state_dict(template, _seed(case.id, "w", SALT.get(case.id, 0)), case.nnz, case.shift,
                          f32_bn=("backbone.bn1",) if case.kind == "stem" else (), biases=case.biases)
    check_folded(case, sd)
    return sd


@functools.lru_cache(maxsize=None)
def inputs(case, n=None):
    shape = (n or case.batch,) + in_shape(case)
    make = normal_input if case.regime == "selection" else exact_input
    return make(shape, _seed(case.id, "x"))


@functools.lru_cache(maxsize=None)
def reference(case, n=None):
    """(expected output, Ref).  The output is what the device must hold bit for bit: bf16 NHWC,
    or for a head case float32 NCHW.  Computed once per case and shared; do not modify."""
    sd, x = weights(case), inputs(case, n)
    if case.regime == "selection":
        # a float32 forward: convs copy values exactly, the fuse sum adds in f32 in term order
        R = Ref(sd, dtype=torch.float32, exact=False)
    else:
        R = Ref(sd)
    y = forward(case, R, x.float())
    if case.kind != "head":
        return y.v.permute(0, 2, 3, 1).contiguous().bfloat16(), R
    if case.regime == "selection":
        w = sd["head.final_layer.weight"].numpy().reshape(17, 32)
        out = head_chain(y.v.permute(0, 2, 3, 1).numpy(), w, sd["head.final_layer.bias"].numpy())
        return torch.from_numpy(out), R
    return y.v.float().contiguous(), R
