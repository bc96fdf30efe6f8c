"""GPU: the label-swap kernels (mvp_label_swap_costs / _solve / _apply) against the numpy
restatement tests/label_swap_ref.py.

Tables: n must be equal exactly.  The sums: both sides are fp64 on the same f32 undistorted and
raw pixels; the bound and its reasoning are those of tests/test_frame_sync_gpu.py (a term's relative
error is about eps · (coordinate scale / d) ≈ 1e-13 at d ≈ 1 px, so rtol 1e-9 leaves three orders
of margin without hiding a wrong term).  The measured maximum is printed: 5.9e-11 over the shapes
below, at nv = 8, where an entry can be the sum of two terms far below one pixel.

Solver: on the restatement's tables the answer must be array_equal, with no margin condition: the
solver only adds and compares, in the stated order."""
import numpy as np
import pytest
import torch

import label_swap_cases as cases
import label_swap_ref as ref
from mvpose import synthetic as syn

pytestmark = pytest.mark.gpu
RTOL = 1e-9
TABLES = ("same", "cross", "keep", "change", "prior")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mvpose import ops as _ops
    return _ops


def _cams_dev(ops, cams):
    return torch.tensor(ops.pack_cameras(syn.reference_camera_params(cams)), device="cuda")


def _compare_tables(ops, k, cams, ci, pairs, units, **kw):
    want = ref.cost_tables(k, cams, list(ci), pairs, units, **kw)
    got = ops.label_swap_costs(torch.tensor(k, device="cuda"), _cams_dev(ops, cams), ci, pairs, units, return_n=True, **kw)
    assert got[5].dtype == torch.int32 and np.array_equal(got[5].cpu().numpy(), want["n"])
    worst = 0.0
    for name, g in zip(TABLES, got):
        g, w = g.cpu().numpy(), want[name]
        assert g.dtype == np.float64 and g.shape == w.shape, name
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = max(worst, float(np.where(w != 0, np.abs(g - w) / np.abs(w), np.abs(g)).max()))
    print(f"T={k.shape[0]} J={k.shape[1]} nv={len(ci)}: max rel |table - ref| = {worst:.3g}")
    for name, g in zip(TABLES, got):
        np.testing.assert_allclose(g.cpu().numpy(), want[name], rtol=RTOL, atol=0, err_msg=name)
    return want


@pytest.mark.parametrize("nv", [2, 4, 8])
def test_tables_match_restatement(ops, nv):
    """T = 48 with 10 % of the x coordinates dropped and injected swaps; non-default parameters
    so that every product shows; with 4 views cam_idx out of order and skipping a column."""
    sc = cases.scene(nv if nv != 4 else 5, 48, 11, "limbs", drops=True)
    ci = {2: (0, 1), 4: (3, 0, 4, 1), 8: tuple(range(8))}[nv]
    k = sc["kpts"].copy()
    k[5:9, :, 2, ci[1]] = 0.05                      # below min_conf
    k[20, :, 1, :] = np.inf                         # a frame without usable keypoints
    want = _compare_tables(ops, k, sc["cams"], ci, sc["pairs"], sc["units"], min_conf=0.1, trunc_px=3.0,
                           motion_trunc_px=6.0, motion_weight=0.75, swap_prior_px=1.5)
    assert (want["n"][20] == 0).all() and (want["n"][5:9, :, 1] == 0).all() and want["n"].max() == 3
    assert (want["same"] < want["cross"]).mean() > 0.25 and (want["cross"] == 2 * 3 * 9.0).any()   # all six at τ²


def test_tables_other_joint_count_single_pair(ops):
    """J = 5, NS = 1, U = 1: the pair is (right, left) = (4, 1) of a body cut to five joints."""
    sc = cases.scene(3, 48, 12, "limbs", drops=True)
    k = np.ascontiguousarray(sc["kpts"][:, [0, 5, 7, 9, 6]])
    want = _compare_tables(ops, k, sc["cams"], (2, 0, 1), [(4, 1)], [0])
    assert want["n"].max() == 1 and want["same"].shape == (48, 1, 3)


def _random_tables(rng, T, U, nv, zero=False):
    n_vp = nv * (nv - 1) // 2
    shapes = dict(same=n_vp, cross=n_vp, keep=nv, change=nv, prior=nv)
    if zero:
        return {k: np.zeros((T, U, n)) for k, n in shapes.items()}
    t = {k: rng.uniform(0.0, 10.0, (T, U, n)) for k, n in shapes.items()}
    # values on a coarse grid in a third of the frames: exact ties between different paths
    coarse = rng.uniform(size=T) < 0.33
    for k in t:
        t[k][coarse] = np.round(t[k][coarse])
    t["keep"][0] = t["change"][0] = 0.0
    return t


@pytest.mark.parametrize("nv", [2, 5, 6, 7, 8])
@pytest.mark.parametrize("T", [1, 2, 300])
def test_solver_alone(ops, nv, T):
    """nv = 2, 5: partly filled wavefront; 6: full; 7, 8: two and four registers per lane.
    T = 300 is no multiple of the backtrack chunk (256, 128 or 64 frames).  Random tables with
    exact ties, and all-zero tables, where every comparison is a tie: everything stays 0."""
    rng = np.random.default_rng(100 * nv + T)
    for zero in (False, True):
        t = _random_tables(rng, T, 3, nv, zero)
        want, want_cost = ref.solve(*(t[k] for k in TABLES))
        swap, cost = ops.label_swap_solve(*(torch.tensor(t[k], device="cuda") for k in TABLES))
        assert swap.dtype == torch.uint8 and tuple(swap.shape) == (T, 3)
        assert np.array_equal(swap.cpu().numpy(), want)
        assert np.array_equal(cost.cpu().numpy(), want_cost)          # the same additions: the same bits
        if zero:
            assert not want.any()
        elif T == 300:
            assert len(np.unique(want)) > min(4, (1 << nv) - 1)     # the path moves through the states


@pytest.mark.parametrize("nv,units", [(2, "limbs"), (4, "limbs"), (4, "body"), (7, "limbs"), (8, "body")])
def test_solver_alone_on_scene_tables(ops, nv, units):
    """The restatement's tables of a scene with dropped keypoints and a frame without data: keep
    and change zero at t = 0, entries saturated at τ², empty rows.  One, two and four registers
    per lane."""
    sc = cases.scene(nv, 120 if nv >= 7 else 240, 4, units, drops=True)
    k = sc["kpts"].copy()
    k[50:53] = np.nan
    t = ref.cost_tables(k, sc["cams"], sc["cam_idx"], sc["pairs"], sc["units"], trunc_px=5.0)
    assert (t["cross"] == t["cross"].max()).sum() > 1 and not t["n"][50:53].any()
    want, want_cost = ref.solve(*(t[name] for name in TABLES))
    swap, cost = ops.label_swap_solve(*(torch.tensor(t[name], device="cuda") for name in TABLES))
    assert want.any() and np.array_equal(swap.cpu().numpy(), want)
    assert np.array_equal(cost.cpu().numpy(), want_cost)


def test_two_views_without_a_prior(ops):
    """swap_prior_px = 0, nv = 2: a state and its complement cost the same in every frame, on the
    kernel's tables as on the restatement's (both read the same table entries), so the tie rules
    alone decide between the truth and its complement: the answer is the restatement's."""
    sc = cases.scene(2, 240, 6, "limbs")
    kd, cd = torch.tensor(sc["kpts"], device="cuda"), _cams_dev(ops, sc["cams"])
    _, _, swap = ops.fix_label_swaps(kd, cd, sc["cam_idx"], sc["pairs"], sc["units"], swap_prior_px=0.0)
    swap = swap.cpu().numpy()
    assert (swap[-1] < 2).all()
    for u in range(2):
        assert np.array_equal(swap[:, u], sc["truth"][:, u]) or np.array_equal(swap[:, u], sc["truth"][:, u] ^ 3)
    _, _, want = ref.fix(sc["kpts"], sc["cams"], sc["cam_idx"], sc["pairs"], sc["units"], swap_prior_px=0.0)
    assert np.array_equal(swap, want)


@pytest.mark.parametrize("nv,T,seed,units", cases.NO_DROP)
def test_fix_label_swaps_end_to_end(ops, nv, T, seed, units):
    sc = cases.scene(nv, T, seed, units)
    kd, gd, cd = torch.tensor(sc["kpts"], device="cuda"), torch.tensor(sc["gauss"], device="cuda"), _cams_dev(ops, sc["cams"])
    fixed, gfixed, swap = ops.fix_label_swaps(kd, cd, sc["cam_idx"], sc["pairs"], sc["units"], gauss=gd)
    assert np.array_equal(swap.cpu().numpy(), sc["truth"])
    assert cases.same_bits(fixed.cpu().numpy(), sc["clean"]) and cases.same_bits(gfixed.cpu().numpy(), sc["gauss_clean"])
    again = ops.fix_label_swaps(kd, cd, sc["cam_idx"], sc["pairs"], sc["units"], gauss=gd)
    assert torch.equal(again[2], swap) and torch.equal(again[0].view(torch.int32), fixed.view(torch.int32))
    assert torch.equal(again[1].view(torch.int64), gfixed.view(torch.int64))
    # the mask applied to the fixed arrays gives the input back
    back, gback = ops.label_swap_apply(fixed, swap, sc["cam_idx"], sc["pairs"], sc["units"], gauss=gfixed)
    assert cases.same_bits(back.cpu().numpy(), sc["kpts"]) and cases.same_bits(gback.cpu().numpy(), sc["gauss"])
    assert kd.cpu().numpy().tobytes() == sc["kpts"].tobytes()          # the input is not written


def test_apply_leaves_unlisted_columns_and_nan_bits(ops):
    """cam_idx out of order and skipping a column; NaN keypoints keep their bits; without gauss."""
    sc = cases.scene(5, 48, 11, "limbs", drops=True)
    ci = (3, 0, 4, 1)
    truth = cases.inject(48, 2, 4, 5)
    want, _ = ref.apply(sc["kpts"], truth, ci, sc["pairs"], sc["units"])
    got, none = ops.label_swap_apply(torch.tensor(sc["kpts"], device="cuda"), torch.tensor(truth, device="cuda"), ci,
                                     sc["pairs"], sc["units"])
    assert none is None and cases.same_bits(got.cpu().numpy(), want)
    assert cases.same_bits(got.cpu().numpy()[..., 2], sc["kpts"][..., 2]) and truth.any()


def test_argument_errors(ops):
    from mvpose import _lib
    sc = cases.scene(2, 48, 11, "limbs")
    kd, cd = torch.tensor(sc["kpts"], device="cuda"), _cams_dev(ops, sc["cams"])
    ok = dict(cam_idx=(0, 1), pairs=sc["pairs"], units=sc["units"])
    for kw, what in ((dict(cam_idx=(0,)), "n_cam_idx"), (dict(trunc_px=0.0), "trunc_px"),
                     (dict(motion_trunc_px=float("inf")), "motion_trunc_px"), (dict(motion_weight=-1.0), "motion_weight"),
                     (dict(swap_prior_px=float("nan")), "swap_prior_px"), (dict(units=[0, 0, 0, 2, 2, 2]), "unit 1"),
                     (dict(pairs=[(5, 6)] * 6), "repeats")):
        with pytest.raises(_lib.MvposeError, match=what):
            ops.label_swap_costs(kd, cd, **{**ok, **kw})
    with pytest.raises(ValueError):
        ops.label_swap_costs(kd[0], cd, **ok)
    with pytest.raises(TypeError):
        ops.label_swap_costs(kd.double(), cd, **ok)
    with pytest.raises(ValueError):
        ops.label_swap_apply(kd, torch.zeros((48, 3), dtype=torch.uint8, device="cuda"), (0, 1), sc["pairs"], sc["units"])
    with pytest.raises(ValueError, match="disagree"):
        z = torch.zeros((4, 1, 3), dtype=torch.float64, device="cuda")
        ops.label_swap_solve(z, z, z, z, z[:, :, :2].contiguous())
    assert ops.label_swap_solve_plan(1000, 2, 8) == 2 * 1000 * 256
    assert ops.label_swap_solve_plan(3, 5, 2) == 5 * 256          # a unit's bytes are rounded up to 256
    with pytest.raises(_lib.MvposeError, match="n_cam_idx"):
        ops.label_swap_solve_plan(10, 2, 9)
