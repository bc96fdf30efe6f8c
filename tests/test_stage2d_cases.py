"""CPU: the inputs of tests/test_stage2d_shapes_gpu.py reach what they are meant to reach,
checked with the oracle alone (oracle/heatmap_ref.py) — so that a GPU test there cannot pass
by comparing nothing with nothing, or judge rounding luck at the moments threshold."""
import numpy as np
import pytest

import stage2d_cases as sc
from oracle import heatmap_ref

MOMENT_IDS = [(name, kind) for name in sc.MOMENT_CASES for kind in sc.MOMENT_KINDS]


@pytest.mark.parametrize("name,kind", MOMENT_IDS)
def test_moment_case_clear_of_threshold_and_no_empty_joint(name, kind):
    """The separable path evaluates a reverted pixel within 2 float32 ulps of OpenCV's
    operation order (documented in moments_kernel), so a pixel within 4 ulps of the 0.01
    threshold could be counted on one side and not the other; and an all-zero joint
    compares 0 with 0.  Neither may occur in any case (the general-path-only case included)."""
    c = sc.moment_case(name, kind)
    print(f"{name} {kind}: nearest pixel {c['gap_ulps']:.0f} ulps from thr, least joint sum {c['sums'].min():.4g}")
    assert c["gap_ulps"] > 4
    assert (c["sums"] > 0).all()
    assert np.isfinite(c["ref"]).all() and (c["ref"][:, [2, 5]] > 0).all()


def test_moment_cases_reach_their_paths():
    """LDS formula of mvp_heatmap_moments: the portrait frame is past the budget of the
    mixed-column closed forms (mixcf off), every other case inside it; the frame widths cover
    a second trip of the 1280-column loop, a partly filled column group and a width below one
    workgroup's 320 lanes; by mvp_warp_is_separable's fixed-point rule every case is separable
    but the rotated one."""
    for name, c in sc.MOMENT_CASES.items():
        lds0 = sc.moments_lds0(*c["map_hw"], *c["hw"])
        assert lds0 <= sc.MOM_LDS, name
        assert (lds0 + c["hw"][0] * 48 > sc.MOM_LDS_CF) == (name == "1600x360"), name
        assert sc.fixed_point_separable(sc.moment_geometry(name)[3], c["hw"]) == (c["geom"] != "rot12"), name
    widths = {c["hw"][1] for c in sc.MOMENT_CASES.values()}
    assert any(w > 1280 for w in widths) and any(w < 320 for w in widths) and any(w % 4 for w in widths)
    assert sc.moments_lds0(64, 48, 480, 8000) > sc.MOM_LDS  # the refusal case


@pytest.mark.parametrize("K,H,W,N,seed", [c + (1,) for c in sc.DECODE_CASES]
                         + [c + (sc.DECODE_VARIANT_SEED,) for c in sc.DECODE_VARIANT_BASES])
def test_decode_case_not_hollow(K, H, W, N, seed):
    """Each decode case holds a map whose peak qualifies for the +-0.25 refinement and one
    whose peak does not — except 3x3, where 1 < px < W - 1 has no solution: there no peak
    qualifies by construction, and the case is about exactly that."""
    hm, hmf, flip, cs = sc.decode_inputs(K, H, W, N, seed)
    for a, b, shift in ((hm, hmf, 1), (hm, hmf, 0), (hm, None, 1)):
        avg, am, scores, kp = sc.decode_oracle(a, b, flip, shift, cs)
        q = sc.refinement_mask(avg)
        assert (~q).any()
        assert q.any() == ((H, W) != (3, 3))
        flat = avg.reshape(N * K, H * W)
        assert (flat[0] == flat[0, 0]).all() and am.ravel()[0] == 0       # all-equal map: first occurrence
        assert (flat[1] == flat[1].max()).sum() == 2                      # exact tie
        assert scores.ravel()[2] <= 0 and (scores.ravel() > 0).any()      # the (-1, -1) rule and the usual one
    if K != 17:
        assert flip != list(range(K)) or K == 1
        assert sorted(flip) == list(range(K))
    # the one-column shift, the mirror and the joint permutation each change the expected average
    want = heatmap_ref.flip_test_average(hm, hmf, flip, True)
    assert not np.array_equal(want, heatmap_ref.flip_test_average(hm, hmf, flip, False))
    assert not np.array_equal(want, heatmap_ref.flip_test_average(hm, hmf[..., ::-1], flip, True))
    if K > 1:
        assert not np.array_equal(want, heatmap_ref.flip_test_average(hm, hmf, list(range(K)), True))
        inverse = [flip.index(k) for k in range(K)]
        assert inverse == flip or not np.array_equal(want, heatmap_ref.flip_test_average(hm, hmf, inverse, True))


def test_planted_maps_is_planted_heatmaps_where_it_fits():
    from test_stage2d_gpu import _planted_heatmaps
    a = sc.planted_maps(np.random.default_rng(4), 2, 17, 64, 48)
    b = _planted_heatmaps(np.random.default_rng(4), 2)
    np.testing.assert_array_equal(a, b)
    small = sc.planted_maps(np.random.default_rng(4), 3, 1, 3, 3)
    assert (small[0, 0] == 0.25).all() and (small[2, 0] == -0.5).all()
    assert small[1, 0, 0, 0] == small[1, 0, 2, 2] == 5.0


@pytest.mark.parametrize("hw", [(480, 854), (1080, 1920)])
def test_preprocess_boxes_reach_the_edges(hw):
    """The boxes overhang the side they are named for; the tiny one repeats sx between
    neighbouring outputs; the last one puts every source column W-5 .. W-1 (both sides of
    the kernel's `sx + 3 < W` switch, which matters where W % 4 == 0) under some output
    whose source rows are inside the frame."""
    H, W = hw
    boxes = sc.preprocess_boxes(hw)
    src = [sc.crop_sources(sc.box_geometry(b)[2]) for b in boxes]
    assert src[0][0].min() < -1 and src[1][0].max() > W and src[2][1].min() < -1 and src[3][1].max() > H
    sx_tiny = src[4][0]
    assert (sx_tiny[:, 1:] == sx_tiny[:, :-1]).mean() > 0.9
    sx, sy = src[5]
    inside = (sy >= 0) & (sy + 1 < H)
    assert set(range(W - 6, W + 1)) <= set(sx[inside].tolist())


@pytest.mark.parametrize("hw", [(479, 641), (720, 1280)])
@pytest.mark.parametrize("rot", [12.0, 90.0])
def test_rotated_crop_is_not_axis_aligned(hw, rot):
    Minv = heatmap_ref.invert_affine(sc.rotated_geometry(hw, rot)[2])
    assert Minv[1] != 0 and Minv[3] != 0
    sx, sy = sc.crop_sources(sc.rotated_geometry(hw, rot)[2])
    inside = (sx >= 0) & (sx + 1 < hw[1]) & (sy >= 0) & (sy + 1 < hw[0])
    assert inside.any() and (~inside).any()


@pytest.mark.parametrize("hw", [(479, 641), (240, 318)])
def test_revert_maps_leave_pixels_outside(hw):
    """The box leaves part of the frame outside the map (exact zeros to check) and part
    inside; the whole-image maps, rotated or not, are larger than the frame."""
    _, mats = sc.revert_inputs(hw)
    assert not sc.outside_map(mats["whole"], hw).any() and not sc.outside_map(mats["rot12"], hw).any()
    out = sc.outside_map(mats["box"], hw)
    assert out.any() and (~out).any()
