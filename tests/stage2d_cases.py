"""Inputs and oracle-side references of the 2D-stage shape tests
(tests/test_stage2d_shapes_gpu.py runs the kernels on them, tests/test_stage2d_cases.py
checks on the CPU, with the oracle alone, that the inputs reach what they are meant to).

Everything here is numpy + oracle/heatmap_ref.py: no GPU, no libmvpose.  Frame sizes are
(H, W) throughout; map sizes are (h, w).  References are computed once per case
(functools.lru_cache) and handed out read-only.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from oracle import heatmap_ref
from test_stage2d_gpu import _planted_heatmaps

INPUT_WH = (192, 256)          # crop (w, h)
THR = np.float32(0.01)         # get_heatmap_means_cov threshold
THR_ULP = 2.0 ** -30           # one float32 ulp at 0.01 (2^-7 <= 0.01 < 2^-6)
FRAME_SIZES = [(1080, 1920), (480, 854), (479, 641), (240, 318), (1600, 360)]


def bf16(x):
    """float32 array rounded to bf16 (round to nearest even), back as float32."""
    return torch.tensor(np.ascontiguousarray(x, np.float32)).bfloat16().float().numpy()


# ------------------------------------------------------------------ geometry --
def box_geometry(box, map_wh=(48, 64)):
    """Oracle side of one person box (tests/test_bbox_gpu.py::_oracle_geometry, for any
    map size): center, scale, crop matrix M (image -> crop), revert matrix Mh (map -> image)."""
    center, scale = heatmap_ref.bbox_xyxy2cs(box)
    scale = heatmap_ref.fix_aspect_ratio(scale, INPUT_WH[0] / INPUT_WH[1])
    M = heatmap_ref.get_warp_matrix(center, scale, 0.0, INPUT_WH)
    Mh = heatmap_ref.get_warp_matrix(center, scale, 0.0, map_wh, inv=True)
    return center, scale, M, Mh


def whole_box(hw):
    return np.array([0.0, 0.0, hw[1], hw[0]])


def rotated_geometry(hw, rot, map_wh=(48, 64)):
    """Whole-image center/scale with a rotated warp: crop matrix M and revert matrix Mh."""
    center, scale, _, _ = box_geometry(whole_box(hw))
    M = heatmap_ref.get_warp_matrix(center, scale, rot, INPUT_WH)
    Mh = heatmap_ref.get_warp_matrix(center, scale, rot, map_wh, inv=True)
    return center, scale, M, Mh


def preprocess_boxes(hw):
    """Boxes of the preprocess test: overhanging each side of the frame, a tiny one
    (~0.05 source px per crop px, so neighbouring outputs share sx), and one narrow enough
    (< 1 source px per crop px) and ending on the frame's last column, so that every
    source column W-5 .. W-1 is some output's sx (test_stage2d_cases.py asserts it)."""
    H, W = hw
    return np.array([[-0.1 * W, 0.2 * H, 0.3 * W, 0.9 * H],
                     [0.7 * W, 0.1 * H, 1.15 * W, 0.8 * H],
                     [0.3 * W, -0.2 * H, 0.6 * W, 0.5 * H],
                     [0.4 * W, 0.6 * H, 0.7 * W, 1.25 * H],
                     [W / 2, H / 2, W / 2 + 10, H / 2 + 11],
                     [W - 121.0, 0.4 * H, W - 1.0, 0.4 * H + 150]])


OVERHANG_BOX = 0  # index into preprocess_boxes: the box the moments / revert cases reuse


def crop_sources(M, out_hw=(INPUT_WH[1], INPUT_WH[0])):
    """(sx, sy) source cell of every crop pixel under crop matrix M (image -> crop)."""
    sx, sy, _, _ = heatmap_ref.warp_coords(heatmap_ref.invert_affine(M), *out_hw)
    return sx, sy


def frames_u8(n, hw, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, hw[0], hw[1], 3), dtype=np.uint8)


def oracle_crop(frame, M, swap_rb=True, mean=None, std=None):
    """heatmap_ref.preprocess rounded to bf16, as (256, 192, 3) float32 (the kernel's NHWC).
    A non-default mean/std restates preprocess's last line with them."""
    if mean is None and std is None:
        ref = heatmap_ref.preprocess(frame, M, swap_rb=swap_rb)
    else:
        crop = heatmap_ref.warp_affine_linear_u8(frame, M, INPUT_WH[1], INPUT_WH[0])
        x = np.moveaxis(crop, -1, 0).astype(np.float32)
        if swap_rb:
            x = x[[2, 1, 0]]
        mean, std = np.asarray(mean, np.float32), np.asarray(std, np.float32)
        ref = ((x - mean[:, None, None]) / std[:, None, None]).astype(np.float32)
    return np.moveaxis(bf16(ref), 0, -1)


# -------------------------------------------------------------------- decode --
# (K, H, W, N): 17 maps with a last workgroup of one; the 16-byte branch at another width;
# the one-cell branch at K's maximum; odd sizes; the smallest map; W % 4 != 0 on a large map
DECODE_CASES = [(17, 64, 48, 1), (5, 32, 24, 3), (32, 16, 12, 3), (2, 65, 47, 3), (1, 3, 3, 3), (17, 64, 50, 3)]
# bases of the variant tests (NULL arguments, shift off, V): N = 6, so that V = 3 divides it and V = 4 does not
DECODE_VARIANT_BASES = [(17, 64, 48, 6), (2, 65, 47, 6)]
DECODE_VARIANT_SEED = 2


def flip_permutation(K):
    """COCO's table at K = 17, otherwise the rotation k -> k + 1: not an involution, so
    reading flip_idx in the wrong direction (which COCO's pair swaps cannot show) fails."""
    if K == 17:
        return list(heatmap_ref.COCO_FLIP_INDICES)
    return [(k + 1) % K for k in range(K)]


def tie_cells(H, W):
    """The two cells of the planted exact tie: _planted_heatmaps' (10, 10) and (20, 5),
    scaled into a map smaller than 21x11; two opposite corners where those coincide (3x3)."""
    if H > 20 and W > 10:
        return (10, 10), (20, 5)
    a, b = (10 * H // 64, 10 * W // 48), (20 * H // 64, 5 * W // 48)
    return (a, b) if a != b else (a, (H - 1, W - 1))


def planted_maps(rng, N, K, H, W):
    """_planted_heatmaps for any allowed (K, H, W): its own result where its fixed
    positions fit (K >= 4 maps per crop, H > 20, W > 10); otherwise the same recipe with
    the four specials on the first maps in (crop, joint) order and their cells scaled into
    the map (y·H/64, x·W/48 when it is smaller than 21x11).  With fewer than four maps
    (K = 1, N = 3) the tie's two cells already lie on the border."""
    if K >= 4 and H > 20 and W > 10:
        return _planted_heatmaps(rng, N, K, H, W)
    hm = rng.normal(0, 0.05, (N, K, H, W)).astype(np.float32)
    for i in range(N):
        for k in range(K):
            y, x = rng.integers(0, H), rng.integers(0, W)
            hm[i, k, y, x] += rng.uniform(0.5, 1.0)
    a, b = tie_cells(H, W)
    flat = hm.reshape(N * K, H, W)
    flat[0] = 0.25                 # all-equal map -> first occurrence
    if N * K > 1:
        flat[1][a] = flat[1][b] = 5.0  # exact tie
    if N * K > 2:
        flat[2] = -0.5             # max <= 0 -> (-1, -1)
    if N * K > 3:
        flat[3][0, 0] = 9.0        # max on the border -> no refinement
    return hm


def decode_center_scale(N):
    """(N, 4) float32 center x, y, scale w, h: a different box per crop."""
    cs = np.zeros((N, 4), np.float32)
    for i in range(N):
        c, s, _, _ = box_geometry([40.0 + 30 * i, 20.5 + 10 * i, 400.0 + 50 * i, 500.0 - 20 * i])
        cs[i, :2], cs[i, 2:] = c, s
    return cs


def decode_inputs(K, H, W, N, seed=1):
    """hm, hm_flip (planted_maps each), flip_idx, center_scale.  Averaged with an arbitrary
    partner, an all-equal map, an exact tie or a map <= 0 is none of these any more
    (tests/test_stage2d_gpu.py::test_decode_vs_oracle meets them in no averaged map), so
    the flipped-input partner hm_flip[n, flip_idx[k]] of the first three maps is shaped to
    keep them: constant 0.25 (all-equal); noise that is 0 in the cells that fall on the
    tie's two cells with or without the one-column shift (5.0 / 2 twice); noise - 0.5
    (<= 0).  The last two stay non-constant, so that the mirror and the shift show in every
    case, the three-map 3x3 one included."""
    rng = np.random.default_rng(seed)
    hm, hmf, flip = planted_maps(rng, N, K, H, W), planted_maps(rng, N, K, H, W), flip_permutation(K)
    noise = rng.normal(0, 0.05, (2, H, W)).astype(np.float32)
    for y, x in tie_cells(H, W):
        for c in (W - 1 - x, W - x):
            if 0 <= c < W:
                noise[0, y, c] = 0.0
    for m, partner in enumerate((np.float32(0.25), noise[0], noise[1] - np.float32(0.5))[:N * K]):
        hmf[m // K, flip[m % K]] = partner
    return hm, hmf, flip, decode_center_scale(N)


def decode_oracle(hm, hmf, flip_idx, shift, cs):
    """avg (N,K,H,W), argmax (N,K), scores (N,K), image keypoints (N,K,2) of the oracle."""
    avg = hm if hmf is None else heatmap_ref.flip_test_average(hm, hmf, flip_idx, bool(shift))
    am, sc, kp = [], [], []
    for i in range(hm.shape[0]):
        rk, rs, ri = heatmap_ref.msra_decode(avg[i])
        am.append(ri)
        sc.append(rs)
        kp.append(heatmap_ref.keypoints_to_image(rk, cs[i, :2], cs[i, 2:]))
    return avg, np.stack(am), np.stack(sc), np.stack(kp)


def refinement_mask(avg):
    """Per map: does its peak qualify for MSRA's +-0.25 refinement (1 < px < W-1, 1 < py < H-1)?"""
    N, K, H, W = avg.shape
    locs, _, _ = heatmap_ref.get_heatmap_maximum(avg.reshape(N * K, H, W))
    px, py = locs[:, 0].astype(int), locs[:, 1].astype(int)
    return ((1 < px) & (px < W - 1) & (1 < py) & (py < H - 1)).reshape(N, K)


# ------------------------------------------------------------------- moments --
def moments_lds0(h, w, img_h, img_w):
    """mvp_heatmap_moments' LDS bytes without the mixed-column prefix table (its lds0);
    the table adds img_h * 48 and is dropped (mixcf off) above MOM_LDS_CF."""
    return (((h * w + 3) & ~3) * 4 + img_w * 8 + ((img_h + 2) & ~1) * 4 + ((h + 2) & ~1) * 8 + (h + 1) * 48)


MOM_LDS, MOM_LDS_CF = 64 * 1024, 96 * 1024

# name -> frame (H, W), K, map (h, w), geometry ("whole", "box", "rot12"), kernel paths
# (the `separable` argument) compared with the oracle
MOMENT_CASES = {
    "1080x1920": dict(hw=(1080, 1920), K=5, map_hw=(64, 48), geom="whole", paths=(1, 2, 0)),
    "480x854": dict(hw=(480, 854), K=17, map_hw=(64, 48), geom="whole", paths=(1, 2, 0)),
    "479x641": dict(hw=(479, 641), K=5, map_hw=(64, 48), geom="whole", paths=(1, 0)),
    "240x318": dict(hw=(240, 318), K=17, map_hw=(64, 48), geom="whole", paths=(1, 0)),
    "1600x360": dict(hw=(1600, 360), K=5, map_hw=(64, 48), geom="whole", paths=(1, 2)),
    "480x854-box": dict(hw=(480, 854), K=5, map_hw=(64, 48), geom="box", paths=(1, 0)),
    "1080x1920-box": dict(hw=(1080, 1920), K=5, map_hw=(64, 48), geom="box", paths=(1, 0)),
    "480x854-K20": dict(hw=(480, 854), K=20, map_hw=(64, 48), geom="whole", paths=(1, 0)),
    "480x854-K1": dict(hw=(480, 854), K=1, map_hw=(64, 48), geom="whole", paths=(1, 0)),
    "480x854-map32x24": dict(hw=(480, 854), K=5, map_hw=(32, 24), geom="whole", paths=(1, 2, 0)),
    "479x641-rot12": dict(hw=(479, 641), K=5, map_hw=(64, 48), geom="rot12", paths=(0,)),
}
MOMENT_KINDS = ("dense", "peaked")
# test_moments_full_frame_vs_oracle's seed: with it no oracle-reverted pixel of any case lies
# within 4 ulps of the threshold and no joint is empty (asserted in test_stage2d_cases.py)
MOMENT_SEED = 3


def moment_geometry(name):
    """Oracle side of a moments case: (box or None, center, scale, Mh (map -> image))."""
    c = MOMENT_CASES[name]
    map_wh = (c["map_hw"][1], c["map_hw"][0])
    if c["geom"] == "rot12":
        center, scale, _, Mh = rotated_geometry(c["hw"], 12.0, map_wh)
        return None, center, scale, Mh
    box = whole_box(c["hw"]) if c["geom"] == "whole" else preprocess_boxes(c["hw"])[OVERHANG_BOX]
    center, scale, _, Mh = box_geometry(box, map_wh)
    return box, center, scale, Mh


def fixed_point_separable(Mh, hw):
    """mvp_warp_is_separable's rule on the oracle's inverted map: in WarpAffineInvoker's
    fixed point the source column does not depend on y nor the source row on x."""
    M = heatmap_ref.invert_affine(Mh)
    ys, xs = np.arange(hw[0], dtype=np.float64), np.arange(hw[1], dtype=np.float64)
    X0 = np.rint((M[1] * ys + M[2]) * 1024.0)
    bd = np.rint(M[3] * xs * 1024.0)
    return bool((X0 == X0[0]).all() and (bd == bd[0]).all())


def visible_cells(Mh, hw, map_hw):
    """Range of map cells the frame's pixels read under revert matrix Mh, clipped to the
    5-cell margin of test_moments_full_frame_vs_oracle's peaks: ((y0, y1), (x0, x1))."""
    sx, sy, _, _ = heatmap_ref.warp_coords(heatmap_ref.invert_affine(Mh), *hw)
    h, w = map_hw
    return ((max(5.0, float(sy.min())), min(h - 5.0, float(sy.max()))),
            (max(5.0, float(sx.min())), min(w - 5.0, float(sx.max()))))


def moment_maps(kind, seed, K, map_hw, cells):
    """The "dense" and "peaked" maps of test_moments_full_frame_vs_oracle, (1, K, h, w).
    That test draws a peak's centre anywhere in the map, 5 cells from its border; a frame
    shows only part of the map (a 16:9 whole-image crop rows 21 .. 43 of 64, a 360-wide
    portrait columns 18 .. 30 of 48), and a peak outside it is an empty joint that
    compares 0 with 0.  The centres are therefore drawn from the cells the frame reads
    (`cells`, visible_cells): peaks cut by the frame's edge are kept, empty joints are not."""
    h, w = map_hw
    rng = np.random.default_rng(seed)
    hm = planted_maps(rng, 1, K, h, w)
    if kind == "dense":
        return (np.abs(hm) + np.float32(0.02)).astype(np.float32)
    assert kind == "peaked"
    (y0, y1), (x0, x1) = cells
    yy, xx = np.mgrid[0:h, 0:w]
    for k in range(K):
        cy, cx = rng.uniform(y0, y1), rng.uniform(x0, x1)
        hm[0, k] = np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * 2.0 ** 2)) - 0.005
    return hm


def moments_oracle(hm_khw, Mh, hw):
    """warp_affine_linear_f32 + heatmap_means_cov_f64 of one crop's maps: the (K, 6)
    reference, the least distance of a reverted pixel to the threshold in float32 ulps at
    0.01, and the per-joint thresholded sums."""
    rev = heatmap_ref.warp_affine_linear_f32(hm_khw, Mh, hw[0], hw[1])
    ref = heatmap_ref.heatmap_means_cov_f64(rev)
    gap = float(np.abs(rev.astype(np.float64) - float(THR)).min() / THR_ULP)
    sums = np.where(rev < THR, 0.0, rev.astype(np.float64)).sum(axis=(1, 2))
    return ref, gap, sums


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def moment_case(name, kind):
    """dict(hm (1,K,h,w) f32, Mh, ref (K,6) f64, gap_ulps, sums (K,)) of a registered case."""
    c = MOMENT_CASES[name]
    _, _, _, Mh = moment_geometry(name)
    hm = moment_maps(kind, MOMENT_SEED, c["K"], c["map_hw"], visible_cells(Mh, c["hw"], c["map_hw"]))
    ref, gap, sums = moments_oracle(hm[0], Mh, c["hw"])
    return dict(hm=_frozen(hm), Mh=_frozen(Mh), ref=_frozen(ref), gap_ulps=gap, sums=_frozen(sums))


def moments_errors(got, ref):
    """Measured figures of a (K, 6) result against the oracle, and whether they meet
    test_moments_full_frame_vs_oracle's bound (relative to the frame, so it carries to
    other sizes): means rtol 2e-6, atol 1e-6; covariances 2e-6·|ref| + 1e-9·(mx² + my²) + 1e-9.
    Returns (max |d mean|, max |d cov|, max of error / bound, ok)."""
    dm = np.abs(got[:, :2] - ref[:, :2])
    bm = 1e-6 + 2e-6 * np.abs(ref[:, :2])
    scale = (ref[:, 0] ** 2 + ref[:, 1] ** 2)[:, None]
    dc = np.abs(got[:, 2:] - ref[:, 2:])
    bc = 2e-6 * np.abs(ref[:, 2:]) + 1e-9 * scale + 1e-9
    ok = bool(np.isfinite(got).all() and (dm <= bm).all() and (dc <= bc).all())
    return float(dm.max()), float(dc.max()), float(max((dm / bm).max(), (dc / bc).max())), ok


# -------------------------------------------------------------------- revert --
def revert_inputs(hw, seed=5, N=2, K=3, map_hw=(64, 48)):
    """Random (N, K, h, w) maps and the three revert matrices (map -> image) the test
    pairs up: whole image, overhanging box, 12° rotation."""
    rng = np.random.default_rng(seed)
    hm = rng.standard_normal((N, K) + map_hw).astype(np.float32)
    mats = {"whole": box_geometry(whole_box(hw))[3],
            "box": box_geometry(preprocess_boxes(hw)[OVERHANG_BOX])[3],
            "rot12": rotated_geometry(hw, 12.0)[3]}
    return hm, mats


def outside_map(Mh, hw, map_hw=(64, 48)):
    """Frame pixels none of whose four taps lies in the map (border value 0)."""
    sx, sy, _, _ = heatmap_ref.warp_coords(heatmap_ref.invert_affine(Mh), *hw)
    h, w = map_hw
    return (sx >= w) | (sx + 1 < 0) | (sy >= h) | (sy + 1 < 0)
