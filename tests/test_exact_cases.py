"""CPU checks of tests/exact_cases.py: every case the GPU file runs (one shared table) meets the
exactness precondition and its regime's conditions, is not degenerate, is demonstrably
independent of the summation order, and the fuse-layer restatement is wired as the oracle's
HRModule is.  No GPU."""
import numpy as np
import pytest
import torch

import exact_cases as ec

EXACT = [c for c in ec.CASES if c.regime != "selection"]
FUSESEL = [c for c in ec.CASES if c.kind == "fusesel"]
ids = lambda cases: [c.id for c in cases]  # noqa: E731


def _tiled(case):
    return [ec.TILE_CROPS] if case.id in ec.TILED.values() else []


@pytest.mark.parametrize("case", EXACT, ids=ids(EXACT))
def test_precondition_and_regime(case):
    """B / q <= 2^20 at every conv and fuse sum (the reference asserts it and that all values
    are multiples of q; here the recorded figures are checked again), then the regime: small
    = every tensor integer-valued within 256 and untouched by bf16 rounding; rounding = bf16
    rounding changes >= 1 % of some tensor, an exact tie among the changed elements."""
    for n in [None] + _tiled(case):
        _, R = ec.reference(case, n)
        assert R.convs
        worst = max(b / q for _, q, b in R.convs)
        print(f"{case.id}: largest B / q = {worst:.0f}")
        assert worst <= ec.LIMIT
        if case.regime == "small":
            for name, v, _ in R.tensors:
                assert float(v.abs().max()) <= ec.SMALL_MAX, (name, float(v.abs().max()))
                assert torch.equal(v, torch.round(v)), name
            assert all(changed == 0 for _, _, changed, _ in R.rounded)
        else:
            assert max(changed / numel for _, numel, changed, _ in R.rounded) >= 0.01, R.rounded
            assert sum(ties for *_, ties in R.rounded) >= 1, R.rounded


@pytest.mark.parametrize("case", ec.CASES, ids=ids(ec.CASES))
def test_not_degenerate(case):
    """20-80 % of every ReLU output positive; the output has >= 16 distinct values and no
    constant channel."""
    y, R = ec.reference(case)
    for name, v, relu in R.tensors:
        if relu:
            pos = float((v > 0).double().mean())
            assert 0.2 <= pos <= 0.8, (name, pos)
    y = y.float()
    assert y.unique().numel() >= 16
    cdim = 1 if case.kind == "head" else 3  # f32 NCHW heatmaps, bf16 NHWC otherwise
    flat = y.movedim(cdim, 0).reshape(y.shape[cdim], -1)
    constant = (flat.min(dim=1).values == flat.max(dim=1).values).nonzero().flatten().tolist()
    assert not constant, constant


@pytest.mark.parametrize("case", EXACT, ids=ids(EXACT))
def test_order_independent(case):
    """The same forward in float32, with the input channels of every conv permuted (another
    summation order, f32 partial sums), equals the float64 forward bit for bit."""
    want, _ = ec.reference(case)
    R = ec.Ref(ec.weights(case), dtype=torch.float32, exact=False, permute_seed=5)
    got = ec.forward(case, R, ec.inputs(case).float()).v
    if case.kind == "head":
        assert torch.equal(got.contiguous().view(torch.int32), want.view(torch.int32))
    else:
        got = got.permute(0, 2, 3, 1).contiguous().bfloat16()
        assert torch.equal(got.view(torch.int16), want.view(torch.int16))


def test_weights_fold_exactly():
    """exact_cases.weights asserts it for every case; here that the assertion bites: the stem's
    f32 weights fold to +-2^-shift only with the variance that cancels BatchNorm's eps."""
    case = ec.BY_ID["stem-rounding"]
    ec.check_folded(case, ec.weights(case))
    sd = ec.exact_state_dict(ec.spec(case)[3], 1, case.nnz, case.shift)  # f32_bn not given
    with pytest.raises(AssertionError):
        ec.check_folded(case, sd)


@pytest.mark.parametrize("n,i", ec.FUSE_LAYERS)
def test_fuse_restatement_matches_oracle(n, i):
    """With ordinary random weights and no bf16 rounding, fuse_layer_ref equals row i of the
    oracle's HRModule.fuse_layers on the same branch tensors (relu of the sum in order
    j = 0..n-1) to 1e-12 relative: the restatement's wiring is the oracle's, whatever hrnet.py does."""
    from mvpose import hrnet
    from oracle import hrnet_ref
    sd = hrnet.fuse_layer_spec(n, i, seed=40 + 4 * n + i)[3]
    R = ec.Ref(sd, exact=False, rounding=False, bf16_weights=False)
    x = torch.randn((2, 64, 48, 32), generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    xs = ec.lead_in(R, R.input(x), n, True)
    got = ec.fuse_layer_ref(R, xs, i).v
    mod = hrnet_ref.HRModule(ec.FUSE_CHANNELS[:n]).double().eval()
    own = {k[len("mod."):]: v.double() for k, v in sd.items() if k.startswith("mod.")}
    res = mod.load_state_dict(own, strict=False)
    assert not res.unexpected_keys and own
    row = mod.fuse_layers[i]
    with torch.no_grad():
        y = 0
        for j in range(n):
            y = y + (xs[j].v if i == j else row[j](xs[j].v))
        want = torch.relu(y)
    assert got.shape == want.shape
    err = float((got - want).abs().max() / want.abs().max())
    assert err <= 1e-12, err


@pytest.mark.parametrize("case", FUSESEL, ids=ids(FUSESEL))
def test_fuse_sum_order_is_observable(case):
    """On the selection-weight cases, summing the terms in reversed order changes the output:
    the bit-exact GPU test therefore pins "sums in input order" (head_fuse_kernel's contract).
    Three and four terms only: (0 + a) + b and (0 + b) + a are the same f32 number, so a
    two-term layer has no order to pin, which is asserted too."""
    want, _ = ec.reference(case)
    R = ec.Ref(ec.weights(case), dtype=torch.float32, exact=False)
    rev = ec.forward(case, R, ec.inputs(case).float(), reverse=True).v.permute(0, 2, 3, 1).contiguous().bfloat16()
    differ = int((rev.view(torch.int16) != want.view(torch.int16)).sum())
    print(f"{case.id}: {differ} of {want.numel()} elements differ with the sum reversed")
    assert differ >= 1 if case.args[0] >= 3 else differ == 0


def test_selection_convs_copy_values():
    """A selection-weight conv output is a signed copy of input values for non-integer data:
    every |output| of the lead-in and projections occurs among the |inputs|."""
    case = ec.BY_ID["fusesel-4x1-selection"]
    _, R = ec.reference(case)
    src = set(ec.inputs(case).float().abs().flatten().tolist()) | {0.0}
    for name, v, _ in R.tensors:
        if name != "fuse":
            assert set(v.abs().flatten().tolist()) <= src, name


def test_head_chain_data_is_normal():
    """The head-chain cases keep |w| and |x| away from the subnormal range, so that the f32
    chain of exact products means the same on the device (which may flush subnormals)."""
    for case in (c for c in ec.CASES if c.kind == "head" and c.regime == "selection"):
        w = ec.weights(case)["head.final_layer.weight"].abs()
        x = ec.inputs(case).float().abs()
        out, _ = ec.reference(case)
        for t in (w[w > 0], x[x > 0], out.abs()[out != 0]):
            assert float(t.min()) > 2.0 ** -60
        assert np.isfinite(out.numpy()).all()
