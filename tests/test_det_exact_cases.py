"""CPU checks of tests/det_exact_cases.py: every case the GPU file runs (one shared table) meets the
exactness precondition and its regime's and activation's conditions, names the variant
det_select.h gives it, and the float64 restatement of every op agrees with tests/det_interp.py
(which tests/test_rtmdet_cpu.py pins to oracle/rtmdet_ref.py) on ordinary weights.  A changed
table that breaks a condition fails here.  No GPU."""
import fractions

import numpy as np
import pytest
import torch

import det_exact_cases as dc
import det_interp
from mvpose import rtmdet as D

DATA = list(dc.BY_KEY.values())   # one case per data key: the cases that differ in switches alone share it
ids = lambda cases: [c.key for c in cases]  # noqa: E731
RES_EXEMPT = {"halo_live3", "halo_pers_lt2", "halo_pers_lt3", "halo_pers_lt4", "fold_up", "fold_ca"}


def test_table_covers_every_variant():
    """Every conv variant of det_select.h under each activation, with a residual where it takes
    one, in both regimes per family; every other op; per conv family a view at coff > 0 of a wider
    output tensor, and one read through such a view."""
    convs = [c for c in dc.CASES if c.op == "conv"]
    for v in dc.CONV_VARIANTS:
        mine = [c for c in convs if c.variant == v]
        assert {c.act for c in mine} == {dc.NONE, dc.RELU, dc.SILU}, v
        if v not in RES_EXEMPT:
            assert {c.act for c in mine if c.res} == {dc.NONE, dc.RELU, dc.SILU}, v
    for f in ("gemm", "fold", "halo", "halo_pers", "band"):
        mine = [c for c in convs if c.family == f]
        assert {"rounding"} <= {c.regime for c in mine} and (f == "fold" or "small" in {c.regime for c in mine}), f
        assert any(c.out_at[0] > 0 or c.fold for c in mine), f
    assert any(c.in_at[0] > 0 for c in convs)
    assert any(c.res and c.act == dc.SILU for c in convs)
    for f in ("gemm", "halo", "band"):
        assert any(c.res and c.act == dc.RELU for c in convs if c.family == f), f
    assert {c.variant for c in dc.CASES} == set(dc.CONV_VARIANTS) | set(dc.OTHER_VARIANTS)


@pytest.mark.parametrize("case", dc.CASES, ids=[c.id for c in dc.CASES])
def test_expected_variant(case):
    """The variant the case names is select_det_conv's (restated in det_exact_cases.select_conv,
    which the GPU test's launch_kernels assertion holds to the library) for a 256-CU part."""
    assert dc.expected_variant(case) == case.variant


def test_persistent_items():
    """The two persistent-GEMM cases about items and workgroups (2 per CU by default, 1 with
    MVPOSE_DET_PERS_OCC=1, on 256 CUs), and the persistent halo case with more tiles than CUs."""
    items = lambda c: -(-c.n * c.h * c.w // 128) * -(-D.pad32(c.cout) // dc.conv_bn(D.pad32(c.cout)))  # noqa: E731
    small = [c for c in dc.CASES if c.variant == "pers_gemm" and c.h == 5 and c.ks == 1]
    assert small and all(items(c) < 512 for c in small)
    big = [c for c in dc.CASES if c.env.get("MVPOSE_DET_PERS_OCC") == "1"]
    assert big and all(c.variant == "pers_gemm" and items(c) > dc.CUS for c in big)
    halo = [c for c in dc.CASES if c.family == "halo_pers" and c.n * -(-c.h // 8) * -(-c.w // 64) > dc.CUS]
    assert halo and all(c.cin == 64 for c in halo)   # two chunks per tile: the double buffer wraps


@pytest.mark.parametrize("case", DATA, ids=ids(DATA))
def test_conditions(case):
    """The reference asserts per op that all values are multiples of q and that B / q <= 2^20, and
    that the folded blobs hold only the case's dyadic values; here the recorded figures are
    checked again, then the case's regime and activation."""
    e = dc.reference(case)
    st = e.stats
    if "ratio" in st:
        print(f"{case.key}: largest B / q = {st['ratio']:.0f}")
        assert st["ratio"] <= dc.LIMIT
    if case.op in ("conv", "stem", "dwpw"):
        assert st["padding_zero"]
    if case.op in ("conv", "stem"):
        assert not st["constant"], st["constant"]
    if case.regime == "small":       # every value fits bf16's 8 bits
        assert st["changed"] == 0
    if case.regime == "rounding":    # bf16 rounding really happens, ties included
        assert st["changed"] >= 0.01 * st["numel"] and st["ties"] >= 1, st
    if case.op == "dwpw" and case.regime == "rounding":
        assert st["mid_changed"] >= 0.01 * st["mid_numel"], st   # the intermediate is rounded too
    if case.act == dc.RELU and case.res:
        assert st["relu_order"] >= 1    # relu(z) + r != relu(z + r) somewhere: the device must show the order
    if case.act == dc.SILU:
        share = st["undecidable"] / st["numel"]
        print(f"{case.key}: {st['undecidable']} of {st['numel']} undecidable ({100 * share:.2f} %)")
        assert share <= dc.SILU_CAP
        # the ends of an undecidable interval are bf16 neighbours ("between the ends" is "either
        # neighbour"), but for the few elements where the residual cancels the SiLU (2.9934 - 3: the
        # error is 2^-18 of the terms, the bf16 step 2^-8 of their small sum), where they are two apart
        lo, hi = e.lo[e.und], e.hi[e.und]
        lb, hb = (dc.bf16_bits(v).astype(np.int32) & 0xFFFF for v in (lo, hi))
        steps = np.where(lo >= 0, hb - lb, lb - hb)
        assert np.all((steps == 1) | (steps == 2)) and np.all((lo >= 0) | (hi < 0)), np.unique(steps)
        assert (steps == 2).sum() <= 0.002 * st["numel"] and (case.res or np.all(steps == 1))
    if case.op == "dw" and case.act != dc.SILU:
        assert st["taps"] == 25 and st["magnitudes"] == 25
        assert case.h < 20 or st["changed"] >= 0.01 * st["numel"]
    if case.op == "ca" or case.fold == "ca":
        assert 0 < st["scales_inside"] <= st["scales"]
    if case.op == "head":
        assert st["clamped"] >= 0.05 * st["boxes"] and st["unclamped"] >= 0.05 * st["boxes"], st


def test_bf16_round():
    """bf16_round is torch's float32 -> bfloat16 rounding where both apply, and rounds a float64
    once (a value just above a tie, which a detour through float32 would round down to it)."""
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(100000, generator=g) * 2.0 ** torch.randint(-20, 20, (100000,), generator=g)).float()
    x = torch.cat([x, torch.tensor([1.00390625, 1.01171875, -3.0078125, 0.0, 255.5, 256.5])])  # ties
    assert np.array_equal(dc.bf16_round(x.double().numpy()), x.bfloat16().double().numpy())
    assert dc.bf16_round(1.00390625 + 2.0 ** -40) == 1.0078125 and dc.bf16_round(1.00390625) == 1.0


ORDINARY = [dc.BY_ID[i] for i in (
    "gemm-64x64-k1s1-20x20x3-views-in32of128-out64of192-silu-silu-PERS=0",
    "gemm-128x64-k3s1-20x20x3-res-out64of128-relu-rounding-PERS=0",
    "gemm-128x64-k3s1-20x20x3-res-out64of128-silu-silu-PERS=0", "gemm-96x192-k3s2-5x5x3-none-small-PERS=0",
    "fold_up-128x192-k1s1-10x10x3-up64-silu-silu", "fold_ca-64x96-k1s1-5x5x7-ca-silu-silu",
    "halo_live3-64x48-k3s1-9x70x3-out64of128-relu-rounding-HALO_PERS=0", "stem-64-silu-silu",
    "dw5-32-5x5-in32of128-silu-silu",
    "dwpw-64x48-5x5-res-out64of128-relu-rounding", "dwpw-96x96-4x4-none-rounding", "ca_pool-64-5x5x2-none-scale",
    "spp-32-4x7-none-copy", "up2-64-5x5-in64of128-out32of128-none-copy", "head_staged-192-5x5-s32-none-head")]


@pytest.mark.parametrize("case", ORDINARY, ids=[c.id for c in ORDINARY])
def test_reference_matches_interpreter(case):
    """On ordinary random weights, biases and data the float64 restatement (no rounding) equals
    det_interp.apply_op's float32 execution of the same ops to f32 accuracy: the views, channel
    padding, weight layouts, fold sources and the activation / residual order are the builder's."""
    c = case.ordinary()
    B = dc.build(c)
    want = dc.reference(c)
    n = c.n
    T = [torch.zeros((n,) + tuple(t[:3])) for t in B.spec.tensors]
    for t, x in B.inputs.items():
        T[t] = torch.nan_to_num(x.float(), nan=0.0)
    cand = torch.zeros((n, B.spec.n_priors, 6))
    first = B.op_index - 1 if c.fold == "up" else B.begin
    for op in B.spec.ops[first:B.end]:
        det_interp.apply_op(B.spec, T, op, cand)
    if c.op == "head":
        got = cand[:, want.rows].double().numpy()
        ref = np.concatenate([want.score[..., None], want.box, want.logit[..., None]], -1)
    elif c.op in ("spp", "up2"):
        got = T[B.out_t].bfloat16().view(torch.int16).numpy()
        keep = want.want != dc.SENT16
        assert np.array_equal(got[keep], want.want[keep])
        return
    else:
        v = B.op.out if B.op.out.t >= 0 else B.op.in_
        got = T[v.t][..., v.coff:v.coff + v.c].double().numpy()
        ref = want
    assert got.shape == ref.shape
    err = float(np.abs(got - ref).max())
    assert err <= 2e-5 * max(1.0, float(np.abs(ref).max())), err


PERTURB = [("gemm-96x96-k3s1-5x5x3-none-small-PERS=0", "tap"), ("halo-64x64-k3s1-9x70x3-res-none-small", "tap"),
           ("dw5-64-5x5-none-taps", "tap"), ("halo-64x64-k3s1-9x70x3-res-none-small", "halo"),
           ("band_8w-96x64-k3s1-40x40x3-out64of192-none-small", "halo"),
           ("gemm-128x64-k3s1-20x20x3-res-out64of128-relu-rounding-PERS=0", "relu"),
           ("dwpw-64x48-5x5-res-out64of128-relu-rounding", "relu")]


@pytest.mark.parametrize("cid,what", PERTURB, ids=[f"{w}-{c}" for c, w in PERTURB])
def test_perturbed_reference_differs(cid, what):
    """A subtly wrong conv changes bits on this data: one tap of one cout dropped (two depthwise
    taps swapped), one input column taken from its neighbour, the ReLU in front of the residual."""
    case = dc.BY_ID[cid]
    good, wrong = dc.reference(case), dc.reference(case, what)
    differ = int((good.want != wrong.want).sum())
    print(f"{cid} / {what}: {differ} of {good.want.size} elements differ")
    assert differ >= 1


def test_blob_check_bites():
    """check_blobs passes on every case (reference() runs it); the depthwise weights fold to their
    dyadic values only with the variance that cancels BatchNorm's eps in f32."""
    case = dc.BY_ID["dw5-64-5x5-none-taps"]
    B = dc.build(case)
    dc.check_blobs(case, B)
    g = dc._base(32)
    w = dc.dw_taps(dc._gen(case, "w"), 64, case.shift)
    g.dw(dc.module_sd("c", w, torch.zeros(64)), "c", g.new(5, 5, 64), act=dc.NONE)   # var 1, not 1 - 1e-5
    with pytest.raises(AssertionError):
        dc.check_blobs(case, dc.Built(g, 1, 2, {}, 0, 1))


def test_attention_chain_in_fractions():
    """The 5x5 attention case (means k / 25, not dyadic): the f32 chain of ca_scales, whose adds
    are the fmaf's one rounding because the weights are powers of two, equals the chain computed
    exactly with fractions.Fraction and rounded to f32 once per step."""
    case = dc.BY_ID["ca_pool-64-5x5x2-none-scale"]
    B = dc.build(case)
    x = dc.view_of(dc.bits_f64(B.inputs[B.op.in_.t]), B.op.in_)
    wt, b = dc._ca_params(B.spec, B.op)
    s, pre = dc.ca_scales(x, wt, b)

    def f32(fr):   # a Fraction to the nearest f32 (ties to even), as a Fraction
        if fr == 0:
            return fr
        e = 0
        while abs(fr) / fractions.Fraction(2) ** e >= 2 ** 24:
            e += 1
        while abs(fr) / fractions.Fraction(2) ** e < 2 ** 23:
            e -= 1
        return round(fr / fractions.Fraction(2) ** e) * fractions.Fraction(2) ** e

    n, c = pre.shape
    for i in range(n):
        mean = [fractions.Fraction(float(np.float32(x[i, :, :, k].sum()) / np.float32(25))) for k in range(c)]
        for o in range(0, c, 7):
            a = fractions.Fraction(float(b[o]))
            for k in range(c):
                a = f32(a + fractions.Fraction(float(wt[k, o])) * mean[k])
            assert a == fractions.Fraction(float(pre[i, o])), (i, o)
    assert ((s > 0) & (s < 1)).any()
