"""CPU: the left/right label-swap decision — the restatement tests/label_swap_ref.py against the
injected truth on the scenes of tests/label_swap_cases.py, its edge cases, and the argument
checks of the C-ABI (which come before any device work).

Without dropped keypoints the answer must equal the truth; with 10 % of the x coordinates NaN at
most 2 % of the (frame, unit) entries may differ.  Applying the answer restores the keypoints
from before the injection bit for bit wherever the answer is the truth."""
import ctypes

import numpy as np
import pytest

import label_swap_cases as cases
import label_swap_ref as ref
from mvpose import swaps, synthetic as syn


def _fix(sc, **kw):
    return ref.fix(sc["kpts"], sc["cams"], sc["cam_idx"], sc["pairs"], sc["units"], gauss=sc["gauss"], **kw)


@pytest.mark.parametrize("nv,T,seed,units", cases.NO_DROP)
def test_reference_finds_the_injected_swaps(nv, T, seed, units):
    sc = cases.scene(nv, T, seed, units)
    assert sc["truth"].any()
    fixed, gfixed, swap = _fix(sc)
    assert swap.dtype == np.uint8 and np.array_equal(swap, sc["truth"])
    assert cases.same_bits(fixed, sc["clean"]) and cases.same_bits(gfixed, sc["gauss_clean"])


@pytest.mark.parametrize("nv,T,seed,units", cases.NO_DROP)
def test_reference_with_dropped_keypoints(nv, T, seed, units):
    sc = cases.scene(nv, T, seed, units, drops=True)
    fixed, _, swap = _fix(sc)
    wrong = int((swap != sc["truth"]).sum())
    print(f"nv={nv} T={T} seed={seed} {units}: {wrong} of {swap.size} entries wrong")
    assert wrong <= 0.02 * swap.size
    good = np.flatnonzero((swap == sc["truth"]).all(axis=1))
    assert cases.same_bits(fixed[good], sc["clean"][good])


def test_apply_twice_restores_the_bits():
    sc = cases.scene(4, 240, 3, "limbs", drops=True)
    args = (sc["cam_idx"], sc["pairs"], sc["units"])
    once, gonce = ref.apply(sc["kpts"], sc["truth"], *args, gauss=sc["gauss"])
    twice, gtwice = ref.apply(once, sc["truth"], *args, gauss=gonce)
    assert not cases.same_bits(once, sc["kpts"])
    assert cases.same_bits(twice, sc["kpts"]) and cases.same_bits(gtwice, sc["gauss"])
    # the injection is the same exchange
    assert cases.same_bits(once, sc["clean"]) and cases.same_bits(gonce, sc["gauss_clean"])


def test_single_frame():
    """T = 1: no motion term; the prior decides, so nothing is exchanged in a consistent frame,
    and a view mirrored against three others is found."""
    sc = cases.scene(4, 240, 3, "body")
    k = sc["clean"][:1]
    _, _, swap = ref.fix(k, sc["cams"], sc["cam_idx"], sc["pairs"], sc["units"])
    assert swap.shape == (1, 1) and swap[0, 0] == 0
    truth = np.array([[4]], np.uint8)
    bad, _ = cases.exchange(k, truth, sc["cam_idx"], sc["pairs"], sc["units"])
    _, _, swap = ref.fix(bad, sc["cams"], sc["cam_idx"], sc["pairs"], sc["units"])
    assert np.array_equal(swap, truth)


def test_view_without_data():
    """A view that is all NaN has empty tables; its bit stays 0 by the tie rules and the other
    views are solved as before."""
    sc = cases.scene(4, 240, 4, "limbs")
    k = sc["kpts"].copy()
    k[:, :, :, 2] = np.nan
    t = ref.cost_tables(k, sc["cams"], sc["cam_idx"], sc["pairs"], sc["units"])
    assert (t["n"][:, :, 2] == 0).all() and (t["keep"][:, :, 2] == 0).all() and (t["prior"][:, :, 2] == 0).all()
    assert (t["same"][:, :, [1, 3, 5]] == 0).all() and (t["cross"][:, :, [1, 3, 5]] == 0).all()
    swap, _ = ref.solve(t["same"], t["cross"], t["keep"], t["change"], t["prior"])
    assert np.array_equal(swap, sc["truth"] & np.uint8(0b1011))


def test_unit_without_a_complete_pair():
    """Unit 1 (the legs) never has both keypoints of a pair: all its tables are zero, every
    comparison ties, and its state stays 0 throughout; unit 0 is unaffected."""
    sc = cases.scene(3, 240, 5, "limbs")
    k = sc["kpts"].copy()
    k[:, [11, 13, 15], 0, :] = np.nan
    t = ref.cost_tables(k, sc["cams"], sc["cam_idx"], sc["pairs"], sc["units"])
    for name in ("n", "same", "cross", "keep", "change", "prior"):
        assert (t[name][:, 1] == 0).all(), name
    swap, cost = ref.solve(t["same"], t["cross"], t["keep"], t["change"], t["prior"])
    assert (swap[:, 1] == 0).all() and cost[1] == 0.0
    assert np.array_equal(swap[:, 0], sc["truth"][:, 0])


def test_two_views_without_a_prior():
    """swap_prior_px = 0, nv = 2: states s and its complement cost the same in every frame, so
    the tie rules decide: the smallest final state, and a flip only when strictly cheaper.  The
    answer is the truth or its complement in both views, fixed by the last frame's tie (the GPU
    test compares the kernels' answer with this one)."""
    sc = cases.scene(2, 240, 6, "limbs")
    _, _, a = _fix(sc, swap_prior_px=0.0)
    assert (a[-1] < 2).all()                      # of {s, s xor 3} the smaller one ends the path
    for u in range(2):
        assert np.array_equal(a[:, u], sc["truth"][:, u]) or np.array_equal(a[:, u], sc["truth"][:, u] ^ 3)
    _, _, c = _fix(sc)                             # the prior removes the ambiguity
    assert np.array_equal(c, sc["truth"])


def test_presets():
    assert swaps.COCO_PAIRS == ((1, 2), (3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14), (15, 16))
    p, u = swaps.preset("limbs")
    assert p.tolist() == [[5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]] and u.tolist() == [0, 0, 0, 1, 1, 1]
    p, u = swaps.preset("body")
    assert len(p) == 6 and u.tolist() == [0] * 6
    with pytest.raises(ValueError, match="preset"):
        swaps.preset("face")


def test_reference_argument_rules():
    ok = dict(T=10, J=17, nv=2, pairs=[(5, 6), (7, 8)], units=[0, 1])
    assert ref.check_args(**ok) == 2
    for bad in (dict(T=0), dict(nv=1), dict(nv=9), dict(pairs=[(5, 6), (6, 8)]), dict(pairs=[(5, 17), (7, 8)]),
                dict(units=[0, 2]), dict(units=[1, 1]), dict(trunc_px=0.0), dict(motion_trunc_px=np.inf),
                dict(motion_weight=-1.0), dict(swap_prior_px=np.nan), dict(min_conf=np.nan)):
        with pytest.raises(ValueError):
            ref.check_args(**{**ok, **bad})


def _ints(v):
    return (ctypes.c_int * len(v))(*v)


def test_library_argument_checks():
    """Every rule is enforced before any device work: the calls below fail with MVP_ERR_ARG on
    a machine without a GPU, with pointers that are never followed."""
    from mvpose import _lib
    for name in ("mvp_label_swap_plan", "mvp_label_swap_solve_plan", "mvp_label_swap_costs", "mvp_label_swap_solve",
                 "mvp_label_swap_apply"):
        assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES
    nbytes = ctypes.c_int64(0)
    assert _lib.lib.mvp_label_swap_plan(100, 17, 4, 6, 2, ctypes.byref(nbytes)) == 0
    assert nbytes.value >= max(4 * 100 * 17 * 8 + 6 * 72, 2 * 100 * 16)
    assert _lib.lib.mvp_label_swap_plan(1000, 17, 8, 6, 2, ctypes.byref(nbytes)) == 0
    assert nbytes.value >= 2 * 1000 * 256                      # the solver's back pointers
    for args, what in (((0, 17, 2, 6, 2), "T="), ((2 ** 27, 17, 2, 6, 2), "T\\*J"), ((10, 17, 1, 6, 2), "n_cam_idx"),
                       ((10, 17, 9, 6, 2), "n_cam_idx"), ((10, 17, 2, 0, 1), "n_pairs"), ((10, 200, 2, 65, 1), "n_pairs"),
                       ((10, 17, 2, 9, 1), "n_pairs"), ((10, 17, 2, 6, 0), "n_units"), ((10, 17, 2, 6, 7), "n_units")):
        assert _lib.lib.mvp_label_swap_plan(*args, None) == -1, args
        assert __import__("re").search(what, _lib.last_error()), (args, _lib.last_error())

    ci, pairs, units = _ints([0, 1]), _ints([5, 6, 7, 8]), _ints([0, 1])
    p = ctypes.c_void_p(64)                                     # never followed

    def costs(T=10, J=17, V=2, ci=ci, nv=2, pairs=pairs, ns=2, units=units, U=2, min_conf=0.0, trunc=20.0, mtrunc=40.0,
              w=1.0, prior=2.0, nbytes=1 << 20):
        return _lib.lib.mvp_label_swap_costs(p, T, J, V, p, 2, ci, nv, pairs, ns, units, U, min_conf, trunc, mtrunc, w,
                                             prior, p, nbytes, p, p, p, p, p, None, None)

    nan, inf = float("nan"), float("inf")
    for kw, what in ((dict(T=0), "T="), (dict(ci=_ints([0, 2])), "cam_idx"), (dict(pairs=_ints([5, 6, 6, 8])), "repeats"),
                     (dict(pairs=_ints([5, 5, 7, 8])), "twice"), (dict(pairs=_ints([5, 17, 7, 8])), "out of range"),
                     (dict(units=_ints([0, 2])), "unit"), (dict(units=_ints([1, 1])), "unit 0"),
                     (dict(min_conf=nan), "min_conf"), (dict(trunc=0.0), "trunc_px"), (dict(trunc=inf), "trunc_px"),
                     (dict(mtrunc=-1.0), "motion_trunc_px"), (dict(mtrunc=nan), "motion_trunc_px"),
                     (dict(w=-0.5), "motion_weight"), (dict(w=inf), "motion_weight"), (dict(prior=-1.0), "swap_prior_px"),
                     (dict(prior=nan), "swap_prior_px"), (dict(nbytes=64), "workspace_bytes")):
        assert costs(**kw) == -1, kw
        assert what in _lib.last_error() and "mvp_label_swap_costs" in _lib.last_error(), (kw, _lib.last_error())

    assert _lib.lib.mvp_label_swap_solve_plan(1000, 2, 8, ctypes.byref(nbytes)) == 0 and nbytes.value == 512000
    for args, what in (((0, 2, 2), "T="), ((10, 0, 2), "n_units"), ((10, 65, 2), "n_units"), ((10, 2, 1), "n_cam_idx")):
        assert _lib.lib.mvp_label_swap_solve_plan(*args, None) == -1 and what in _lib.last_error(), args

    def solve(T=10, U=2, nv=2, nbytes=1 << 20, tables=p):
        return _lib.lib.mvp_label_swap_solve(tables, p, p, p, p, T, U, nv, p, nbytes, p, None, None)

    for kw, what in ((dict(T=0), "T="), (dict(nv=9), "n_cam_idx"), (dict(U=0), "n_units"),
                     (dict(T=1000, nv=8, nbytes=2 * 255999), "workspace_bytes"), (dict(tables=None), "null")):
        assert solve(**kw) == -1, kw
        assert what in _lib.last_error(), (kw, _lib.last_error())

    q = ctypes.c_void_p(128)

    def apply(ci=ci, gauss=None, gout=None, out=q, C=6, pairs=pairs):
        return _lib.lib.mvp_label_swap_apply(p, gauss, 10, 17, 2, C, ci, 2, pairs, 2, units, 2, p, out, gout, None)

    for kw, what in ((dict(ci=_ints([1, 1])), "twice"), (dict(ci=_ints([0, 2])), "cam_idx"), (dict(gauss=p), "go together"),
                     (dict(out=p), "must not be"), (dict(gauss=p, gout=q, C=0), "C="),
                     (dict(pairs=_ints([5, 6, 6, 8])), "repeats")):
        assert apply(**kw) == -1, kw
        assert what in _lib.last_error(), (kw, _lib.last_error())


def test_eye_and_ear_pairs_carry_no_evidence():
    """The eye and ear pairs as a unit of their own (the presets leave them out: they lie a few
    pixels apart) do not disturb the decision of the limbs' units; how many of the head unit's
    entries are wrong is printed, not asserted."""
    sc = cases.scene(3, 240, 3, "limbs")
    pairs = [(1, 2), (3, 4)] + sc["pairs"]
    units = [2, 2] + sc["units"]
    truth = np.concatenate([sc["truth"], cases.inject(240, 1, 3, 77)], axis=1)
    bad, _ = cases.exchange(sc["clean"], truth, sc["cam_idx"], pairs, units)
    _, _, swap = ref.fix(bad, sc["cams"], sc["cam_idx"], pairs, units)
    assert np.array_equal(swap[:, :2], sc["truth"])
    print("head unit wrong:", int((swap[:, 2] != truth[:, 2]).sum()), "of 240")
