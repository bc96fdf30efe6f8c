"""GPU: the 2D-stage kernels of csrc/heatmap.hip (preprocess, decode, moments, revert) and
the estimator that drives them, against the oracle at other frame sizes than 720x1280 and
on the branches that size never takes: widths that are no multiple of 4 (every pixel on
preprocess's six-byte-load path), boxes and rotated maps, swap_rb / flip off, decode's
one-cell-per-lane branch and other map sizes, a second trip and a partly filled group in the
moments column loop, the separable path without the mixed-column closed forms, per-crop
separability flags, K other than 17, and revert with N > 1.

Inputs and oracle-side references come from tests/stage2d_cases.py; that they reach those
branches (and are clear of the moments threshold) is checked on the CPU in
tests/test_stage2d_cases.py.  Frame sizes are (H, W)."""
import ctypes

import numpy as np
import pytest
import torch

import stage2d_cases as cases
from oracle import heatmap_ref
from test_bbox_gpu import BOXES, _oracle_geometry
from test_stage2d_gpu import _p, _s

pytestmark = pytest.mark.gpu

# sentinel bit patterns (quiet NaNs with a payload no kernel produces)
SENT16, SENT32, SENT64 = 0x7FC1, 0x7FC12345, 0x7FF8123456789ABC


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mvpose import _lib, geometry
    return _lib, geometry


def _sent(shape, dtype):
    return torch.full(shape, {torch.int16: SENT16, torch.int32: SENT32, torch.int64: SENT64}[dtype], dtype=dtype,
                      device="cuda")


def _f3(v):
    return (ctypes.c_float * 3)(*[float(x) for x in v])


# ---------------------------------------------------------------- preprocess --
def _preprocess(_lib, frames, minv, n=None, swap_rb=1, with_flip=1, mean=heatmap_ref.MEAN_RGB,
                std=heatmap_ref.STD_RGB):
    """mvp_preprocess of `n` (default all) frames into 2·len(frames) sentinel-filled crops:
    the raw 16-bit patterns (2N, 256, 192, 4) and the same as float32 values."""
    N, H, W, _ = frames.shape
    fd = torch.tensor(frames, device="cuda")
    md = torch.tensor(np.ascontiguousarray(minv, np.float64).reshape(N, 6), device="cuda")
    out = _sent((2 * N, 256, 192, 4), torch.int16)
    _lib.call("mvp_preprocess", _p(fd), N if n is None else n, H, W, _p(md), 256, 192, _f3(mean), _f3(std),
              swap_rb, with_flip, _p(out), _s())
    torch.cuda.synchronize()
    raw = out.cpu()
    return raw.numpy(), raw.view(torch.bfloat16).float().numpy()


def _check_crops(vals, refs, flipped=True):
    n = len(refs)
    for i, ref in enumerate(refs):
        np.testing.assert_array_equal(vals[i, :, :, :3], ref, err_msg=f"crop {i}")
        assert (vals[i, :, :, 3] == 0).all()
        if flipped:
            np.testing.assert_array_equal(vals[n + i, :, :, :3], ref[:, ::-1], err_msg=f"crop {i} flipped")
            assert (vals[n + i, :, :, 3] == 0).all()


@pytest.mark.parametrize("hw", cases.FRAME_SIZES)
def test_preprocess_whole_image_sizes(lib, hw):
    """Whole-image crop, bit-exact bf16: 1920 wide takes the three-dword path like 1280;
    854, 641, 318 (W % 4 != 0) send every pixel through the byte loads; 1600x360 is a
    portrait frame (the crop's width, not its height, is padded)."""
    _lib, geometry = lib
    frames = cases.frames_u8(2, hw, seed=hw[0])
    g = geometry.CropGeometry.whole_image(hw[1], hw[0])
    _, vals = _preprocess(_lib, frames, np.tile(g.crop_minv, (2, 1)))
    M = cases.box_geometry(cases.whole_box(hw))[2]
    _check_crops(vals, [cases.oracle_crop(f, M) for f in frames])


@pytest.mark.parametrize("hw", [(480, 854), (1080, 1920)])
def test_preprocess_boxes(lib, hw):
    """Boxes overhanging each side, a tiny box, and a box on the frame's last column
    (cases.preprocess_boxes), one per frame: crop + flipped copy bit-exact."""
    _lib, geometry = lib
    boxes = cases.preprocess_boxes(hw)
    frames = cases.frames_u8(len(boxes), hw, seed=7)
    minv = np.stack([geometry.CropGeometry(b).crop_minv for b in boxes])
    _, vals = _preprocess(_lib, frames, minv)
    _check_crops(vals, [cases.oracle_crop(f, cases.box_geometry(b)[2]) for f, b in zip(frames, boxes)])


@pytest.mark.parametrize("hw", [(479, 641), (720, 1280)])
def test_preprocess_rotated(lib, hw):
    """12° and 90° rotated crop maps (M[1], M[3] != 0: the source column changes with the
    crop row); minv = geometry.inverse_map(M)."""
    _lib, geometry = lib
    frames = cases.frames_u8(2, hw, seed=11)
    Ms = [cases.rotated_geometry(hw, rot)[2] for rot in (12.0, 90.0)]
    _, vals = _preprocess(_lib, frames, np.stack([geometry.inverse_map(M) for M in Ms]))
    _check_crops(vals, [cases.oracle_crop(f, M) for f, M in zip(frames, Ms)])


@pytest.fixture(scope="module")
def small_frames(lib):
    _, geometry = lib
    hw = (480, 854)
    frames = cases.frames_u8(2, hw, seed=13)
    minv = np.tile(geometry.CropGeometry.whole_image(hw[1], hw[0]).crop_minv, (2, 1))
    return frames, minv, cases.box_geometry(cases.whole_box(hw))[2]


def test_preprocess_no_swap(lib, small_frames):
    frames, minv, M = small_frames
    _, vals = _preprocess(lib[0], frames, minv, swap_rb=0)
    _check_crops(vals, [cases.oracle_crop(f, M, swap_rb=False) for f in frames])


def test_preprocess_other_mean_std(lib, small_frames):
    frames, minv, M = small_frames
    mean, std = np.array([101.3, 57.9, 140.2], np.float32), np.array([31.7, 64.9, 12.3], np.float32)
    _, vals = _preprocess(lib[0], frames, minv, mean=mean, std=std)
    _check_crops(vals, [cases.oracle_crop(f, M, mean=mean, std=std) for f in frames])


def test_preprocess_without_flip_leaves_second_half(lib, small_frames):
    frames, minv, M = small_frames
    raw, vals = _preprocess(lib[0], frames, minv, with_flip=0)
    _check_crops(vals, [cases.oracle_crop(f, M) for f in frames], flipped=False)
    assert (raw[2:] == SENT16).all()


def test_preprocess_zero_frames_writes_nothing(lib, small_frames):
    frames, minv, _ = small_frames
    raw, _ = _preprocess(lib[0], frames, minv, n=0)
    assert (raw == SENT16).all()


# -------------------------------------------------------------------- decode --
def _decode_buffers(N, K, H, W, V):
    return dict(avg=_sent((N, K, H, W), torch.int32), kpts=_sent((N, K, 2), torch.int32),
                scores=_sent((N, K), torch.int32), argmax=_sent((N, K), torch.int32),
                tkv=_sent(((N + V - 1) // V, K, 3, V), torch.int32))


def _decode_call(_lib, bufs, hm, hmf, flip, shift, cs, V, null=()):
    """mvp_heatmap_decode into `bufs` (the optional outputs named in `null` passed as NULL);
    returns the buffers' bit patterns as int32 numpy arrays."""
    N, K, H, W = hm.shape
    hd = torch.tensor(hm, device="cuda")
    hfd = torch.tensor(hmf, device="cuda") if hmf is not None else None
    csd = torch.tensor(cs, device="cuda")
    ptr = {k: (None if k in null else _p(v)) for k, v in bufs.items()}
    try:
        _lib.call("mvp_heatmap_decode", _p(hd), _p(hfd), N, K, H, W, (ctypes.c_int * K)(*flip), shift, _p(csd), 192,
                  256, ptr["avg"], ptr["kpts"], ptr["scores"], ptr["argmax"], ptr["tkv"], V, _s())
    finally:
        torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in bufs.items()}


def _f(a):
    return a.view(np.float32)


def _check_decode(out, hm, hmf, flip, shift, cs, V, null=()):
    N, K = hm.shape[:2]
    avg, am, scores, kp = cases.decode_oracle(hm, hmf, flip, shift, cs)
    if "avg" not in null:
        np.testing.assert_array_equal(_f(out["avg"]), avg)
    if "argmax" not in null:
        np.testing.assert_array_equal(out["argmax"], am)
    np.testing.assert_array_equal(_f(out["scores"]), scores)
    np.testing.assert_array_equal(_f(out["kpts"]), kp)
    if "tkv" not in null:
        t = _f(out["tkv"])  # [t][k][3][V], crops ordered (t, v)
        assert t.shape == (N // V, K, 3, V)
        for i in range(N):
            np.testing.assert_array_equal(t[i // V, :, :2, i % V], kp[i])
            np.testing.assert_array_equal(t[i // V, :, 2, i % V], scores[i])
    for k in null:
        assert (out[k] == SENT32).all(), k


@pytest.mark.parametrize("K,H,W,N", cases.DECODE_CASES)
def test_decode_map_sizes(lib, K, H, W, N):
    """avg, argmax, scores, keypoints and kpts_tkv bit-exact at every (K, H, W) of
    cases.DECODE_CASES, with a flip table that is a rotation where K != 17 and V = N
    views.  3x3: no cell satisfies 1 < px < W - 1, so no peak is refined — the smallest
    map the ABI admits is about exactly that."""
    hm, hmf, flip, cs = cases.decode_inputs(K, H, W, N)
    out = _decode_call(lib[0], _decode_buffers(N, K, H, W, N), hm, hmf, flip, 1, cs, N)
    _check_decode(out, hm, hmf, flip, 1, cs, N)


@pytest.fixture(scope="module", params=cases.DECODE_VARIANT_BASES, ids=lambda p: "x".join(map(str, p)))
def decode_base(request, lib):
    """Inputs of the variant tests (N = 6, so that V = 3 divides it and V = 4 does not)
    and the full run's outputs (V = 2) the NULL variants are compared with."""
    K, H, W, N = request.param
    hm, hmf, flip, cs = cases.decode_inputs(K, H, W, N, cases.DECODE_VARIANT_SEED)
    full = _decode_call(lib[0], _decode_buffers(N, K, H, W, 2), hm, hmf, flip, 1, cs, 2)
    _check_decode(full, hm, hmf, flip, 1, cs, 2)
    return hm, hmf, flip, cs, full


def test_decode_without_flipped_maps(lib, decode_base):
    """hm_flip = NULL: avg is the input, decode is msra_decode(hm)."""
    hm, _, flip, cs, _ = decode_base
    out = _decode_call(lib[0], _decode_buffers(*hm.shape, 2), hm, None, flip, 1, cs, 2)
    np.testing.assert_array_equal(_f(out["avg"]), hm)
    _check_decode(out, hm, None, flip, 1, cs, 2)


def test_decode_without_shift(lib, decode_base):
    hm, hmf, flip, cs, _ = decode_base
    out = _decode_call(lib[0], _decode_buffers(*hm.shape, 2), hm, hmf, flip, 0, cs, 2)
    _check_decode(out, hm, hmf, flip, 0, cs, 2)


@pytest.mark.parametrize("null", ["avg", "argmax", "tkv"])
def test_decode_optional_output_null(lib, decode_base, null):
    """Each optional output NULL in turn: the others are bit for bit those of the full run."""
    hm, hmf, flip, cs, full = decode_base
    out = _decode_call(lib[0], _decode_buffers(*hm.shape, 2), hm, hmf, flip, 1, cs, 2, null=(null,))
    _check_decode(out, hm, hmf, flip, 1, cs, 2, null=(null,))
    for k in full:
        if k != null:
            np.testing.assert_array_equal(out[k], full[k], err_msg=k)


def test_decode_three_views(lib, decode_base):
    """V = 3, N = 6: kpts_tkv is [t][k][3][V]."""
    hm, hmf, flip, cs, _ = decode_base
    out = _decode_call(lib[0], _decode_buffers(*hm.shape, 3), hm, hmf, flip, 1, cs, 3)
    _check_decode(out, hm, hmf, flip, 1, cs, 3)


def test_decode_refuses_views_not_dividing(lib, decode_base):
    """V = 4, N = 6: refused, every output left at its sentinel."""
    from mvpose._lib import MvposeError
    hm, hmf, flip, cs, _ = decode_base
    bufs = _decode_buffers(*hm.shape, 4)
    with pytest.raises(MvposeError, match="not a multiple"):
        _decode_call(lib[0], bufs, hm, hmf, flip, 1, cs, 4)
    torch.cuda.synchronize()
    for k, v in bufs.items():
        assert (v.cpu().numpy() == SENT32).all(), k


# ------------------------------------------------------------------- moments --
def _moments(_lib, hm, minv, hw, separable, sep_dev=None):
    """mvp_heatmap_moments into a sentinel-filled (N, K, 6) buffer; float64 values."""
    N, K, h, w = hm.shape
    hd = torch.tensor(np.ascontiguousarray(hm), device="cuda")
    md = torch.tensor(np.ascontiguousarray(minv, np.float64).reshape(N, 6), device="cuda")
    sd = torch.tensor(sep_dev, dtype=torch.int32, device="cuda") if sep_dev is not None else None
    out = _sent((N, K, 6), torch.int64)
    try:
        _lib.call("mvp_heatmap_moments", _p(hd), N, K, h, w, _p(md), hw[0], hw[1], ctypes.c_float(0.01),
                  int(separable), _p(sd), _p(out), _s())
    finally:
        torch.cuda.synchronize()
    return out.cpu().numpy()


def _device_revert_minv(geometry, name):
    """The image -> map matrix the product forms for a registered case (CropGeometry; for
    another map size geometry.warp_matrix with it; for the rotated case inverse_map of the
    oracle's matrix)."""
    c = cases.MOMENT_CASES[name]
    box, _, _, Mh = cases.moment_geometry(name)
    if box is None:
        return geometry.inverse_map(Mh)
    g = geometry.CropGeometry(box)
    if c["map_hw"] == (64, 48):
        return g.revert_minv
    return geometry.inverse_map(geometry.warp_matrix(g.center, g.scale, (c["map_hw"][1], c["map_hw"][0]), inv=True))


MOMENT_RUNS = [(name, kind, path) for name, c in cases.MOMENT_CASES.items() for kind in cases.MOMENT_KINDS
               for path in c["paths"]]


@pytest.mark.parametrize("name,kind,path", MOMENT_RUNS)
def test_moments_sizes_vs_oracle(lib, name, kind, path):
    """Every case of cases.MOMENT_CASES (frame sizes 1080x1920 .. 240x318 and the 1600x360
    portrait, an overhanging box, K = 20 / 1, a 32x24 map, a 12° rotated revert map) on the
    kernel paths listed there (`separable` = 1: closed forms, 2: every column walked,
    0: general per-pixel path), dense and peaked maps, against warp_affine_linear_f32 +
    heatmap_means_cov_f64 within test_moments_full_frame_vs_oracle's bound (means rtol 2e-6
    atol 1e-6; covariances 2e-6·|ref| + 1e-9·(mx² + my²) + 1e-9).  Measured on an MI355X
    (printed per case; error / bound is the largest ratio over the case's 6·K numbers),
    maxima over all cases of a path:
      separable = 0: |d mean| 8.0e-13 px, |d cov| 2.2e-08 px², error / bound 9.4e-07 (1080x1920-box
                     peaked) — OpenCV's operation order, only the fp64 summation order differs;
      separable = 1: |d mean| 2.1e-07 px (1080x1920-box dense), |d cov| 6.5e-05 px² (1080x1920
                     dense), error / bound 0.047 (480x854 dense); the 1600x360 portrait, without
                     the mixed-column closed forms: 9.5e-08 px, 4.9e-05 px², 0.020;
      separable = 2: |d mean| 1.5e-05 px, |d cov| 3.0e-03 px² (1080x1920 dense), error / bound
                     0.29 (480x854-map32x24 peaked) — every column walked with f32 partial sums
                     per run of rows (44 image rows per map row there).
    No size or path misses the bound, so it stands as it is."""
    from mvpose.estimator import warp_is_separable
    _lib, geometry = lib
    c = cases.MOMENT_CASES[name]
    H, W = c["hw"]
    h, w = c["map_hw"]
    minv = _device_revert_minv(geometry, name)
    assert warp_is_separable(minv, H, W) == (c["geom"] != "rot12")
    if name == "1600x360":
        # mvp_heatmap_moments: mixcf = separable == 1 && lds0 + img_h * 48 <= 96 KiB.  Past it here,
        # so separable = 1 runs the closed forms for full / empty columns with a walk for mixed ones
        lds0 = ((h * w + 3) & ~3) * 4 + W * 8 + ((H + 2) & ~1) * 4 + ((h + 2) & ~1) * 8 + (h + 1) * 48
        assert lds0 <= 64 * 1024 < 96 * 1024 < lds0 + H * 48
    case = cases.moment_case(name, kind)
    got = _moments(_lib, case["hm"], minv, (H, W), path).view(np.float64)[0]
    dm, dc, worst, ok = cases.moments_errors(got, case["ref"])
    print(f"\nmoments {name} {kind} separable={path}: max|d mean| {dm:.3g} px, max|d cov| {dc:.3g} px², "
          f"error/bound {worst:.3g}")
    assert ok, (name, kind, path, dm, dc, worst)


@pytest.mark.parametrize("separable", [1, 0])
def test_moments_k20_groups_equal_one_joint_per_workgroup(lib, separable, monkeypatch):
    """K = 20 with the default joints per workgroup (groups of 17 + 3) is bit for bit the
    MVPOSE_MOM_JPB=1 run (20 groups of one)."""
    _lib, geometry = lib
    name = "480x854-K20"
    minv, hw = _device_revert_minv(geometry, name), cases.MOMENT_CASES[name]["hw"]
    for kind in cases.MOMENT_KINDS:
        hm = cases.moment_case(name, kind)["hm"]
        monkeypatch.delenv("MVPOSE_MOM_JPB", raising=False)
        default = _moments(_lib, hm, minv, hw, separable)
        monkeypatch.setenv("MVPOSE_MOM_JPB", "1")
        one = _moments(_lib, hm, minv, hw, separable)
        assert (default != SENT64).all() and not np.isnan(default.view(np.float64)).any()
        np.testing.assert_array_equal(default, one)


def test_moments_mixed_separable_flags(lib):
    """Three crops at 479x641 — whole image, the 12° rotated map, an overhanging box — with
    separable = 1 and device flags [1, 0, 1]: each crop is bit for bit the same crop run
    alone with the scalar flag (1, 0, 1), so the flagged crop takes the general path and
    its neighbours keep the separable one."""
    _lib, geometry = lib
    hw = (479, 641)
    box = cases.preprocess_boxes(hw)[cases.OVERHANG_BOX]
    mh_rot = cases.rotated_geometry(hw, 12.0)[3]
    minv = np.stack([geometry.CropGeometry.whole_image(hw[1], hw[0]).revert_minv, geometry.inverse_map(mh_rot),
                     geometry.CropGeometry(box).revert_minv])
    cells = cases.visible_cells(cases.box_geometry(box)[3], hw, (64, 48))
    hm = np.concatenate([cases.moment_maps("peaked", 31, 17, (64, 48), cells),
                         cases.moment_maps("dense", 32, 17, (64, 48), cells),
                         cases.moment_maps("peaked", 33, 17, (64, 48), cells)])
    flags = [1, 0, 1]
    batch = _moments(_lib, hm, minv, hw, 1, sep_dev=flags)
    assert (batch != SENT64).all()
    for i, f in enumerate(flags):
        alone = _moments(_lib, hm[i:i + 1], minv[i:i + 1], hw, f)
        np.testing.assert_array_equal(batch[i], alone[0], err_msg=f"crop {i}")
    # the two paths differ in their last bits, so the equalities above tell them apart: had
    # crop 1's flag sent its neighbours to the general path too, crop 0 would equal this run
    assert not np.array_equal(_moments(_lib, hm[0:1], minv[0:1], hw, 0)[0], batch[0])


def test_moments_refuses_frame_past_lds_budget(lib):
    from mvpose._lib import MvposeError
    _lib, geometry = lib
    hm = cases.moment_case("480x854-K1", "dense")["hm"]
    minv = geometry.CropGeometry.whole_image(8000, 480).revert_minv
    hd = torch.tensor(hm, device="cuda")
    md = torch.tensor(minv[None], device="cuda")
    out = _sent((1, 1, 6), torch.int64)
    with pytest.raises(MvposeError, match="LDS budget"):
        _lib.call("mvp_heatmap_moments", _p(hd), 1, 1, 64, 48, _p(md), 480, 8000, ctypes.c_float(0.01), 1, None,
                  _p(out), _s())
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENT64).all()


# -------------------------------------------------------------------- revert --
@pytest.mark.parametrize("pair", [("whole", "box"), ("box", "rot12")], ids="-".join)
@pytest.mark.parametrize("hw", [(479, 641), (240, 318)])
def test_revert_bit_exact(lib, hw, pair):
    """mvp_heatmap_revert of N = 2 crops with different maps, K = 3 random maps, bit-exact
    against warp_affine_linear_f32; widths 641 and 318 leave a partly filled last block of
    256 columns; pixels outside the map are exactly 0."""
    _lib, geometry = lib
    H, W = hw
    hm, mats = cases.revert_inputs(hw)
    boxes = {"whole": cases.whole_box(hw), "box": cases.preprocess_boxes(hw)[cases.OVERHANG_BOX]}
    minv = np.stack([geometry.CropGeometry(boxes[k]).revert_minv if k in boxes else geometry.inverse_map(mats[k])
                     for k in pair])
    hd, md = torch.tensor(hm, device="cuda"), torch.tensor(minv, device="cuda")
    out = _sent((2, 3, H, W), torch.int32)
    _lib.call("mvp_heatmap_revert", _p(hd), 2, 3, 64, 48, _p(md), H, W, _p(out), _s())
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.float32)
    for n, k in enumerate(pair):
        np.testing.assert_array_equal(got[n], heatmap_ref.warp_affine_linear_f32(hm[n], mats[k], H, W), err_msg=k)
        assert (got[n][:, cases.outside_map(mats[k], hw)] == 0).all()


# ----------------------------------------------------------------- estimator --
EST_SIZES = {"480x854": dict(hw=(480, 854), moment_crops=6), "1080x1920": dict(hw=(1080, 1920), moment_crops=2)}


@pytest.fixture(scope="module", params=list(EST_SIZES))
def est_run(request):
    """tests/test_bbox_gpu.py's run at another frame size: its BOXES rescaled to the frame."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mvpose import hrnet, synthetic as syn
    from mvpose.estimator import BatchPoseEstimator
    H, W = EST_SIZES[request.param]["hw"]
    boxes = BOXES * np.array([W / 1280, H / 720, W / 1280, H / 720])
    n = len(boxes)
    est = BatchPoseEstimator(hrnet.random_state_dict(41), max_frames=6, frame_hw=(H, W))
    frames = syn.make_frames(n, seed=43, h=H, w=W)
    r = est.run(torch.tensor(frames, device="cuda"), argmax=True, bboxes=boxes)
    torch.cuda.synchronize()
    out = {k: r[k].cpu().numpy() for k in ("keypoints", "scores", "gaussians", "argmax")}
    out["avg"] = est.avg[:n].cpu().numpy()
    out["crops"] = est.crops[: 2 * n].float().cpu().numpy()
    return (H, W), boxes, frames, out, EST_SIZES[request.param]["moment_crops"]


def test_estimator_preprocess_bit_exact(est_run):
    (H, W), boxes, frames, out, _ = est_run
    n = len(boxes)
    for i, box in enumerate(boxes):
        _, _, M, _ = _oracle_geometry(box, W, H)
        ref = cases.oracle_crop(frames[i], M)
        np.testing.assert_array_equal(out["crops"][i, :, :, :3], ref, err_msg=f"box {i}")
        np.testing.assert_array_equal(out["crops"][n + i, :, :, :3], ref[:, ::-1], err_msg=f"box {i} flipped")


def test_estimator_decode_bit_exact(est_run):
    (H, W), boxes, _, out, _ = est_run
    for i, box in enumerate(boxes):
        center, scale, _, _ = _oracle_geometry(box, W, H)
        rk, rs, ri = heatmap_ref.msra_decode(out["avg"][i])
        np.testing.assert_array_equal(out["argmax"][i], ri)
        np.testing.assert_array_equal(out["scores"][i], rs)
        np.testing.assert_array_equal(out["keypoints"][i], heatmap_ref.keypoints_to_image(rk, center, scale),
                                      err_msg=f"box {i}")


def test_estimator_moments_vs_oracle(est_run):
    """The bound of test_moments_sizes_vs_oracle on the backbone's own maps (6 crops at
    480x854, 2 at 1080x1920 to keep the numpy oracle short).  Measured on an MI355X, largest
    over the crops: 480x854 |d mean| 1.1e-07 px, |d cov| 1.7e-05 px², error / bound 0.013;
    1080x1920 1.5e-07 px, 3.8e-05 px², 0.0024."""
    (H, W), boxes, _, out, crops = est_run
    for i, box in enumerate(boxes[:crops]):
        _, _, _, Mh = _oracle_geometry(box, W, H)
        ref = heatmap_ref.heatmap_means_cov_f64(heatmap_ref.warp_affine_linear_f32(out["avg"][i], Mh, H, W))
        dm, dc, worst, ok = cases.moments_errors(out["gaussians"][i], ref)
        print(f"\nestimator {H}x{W} box {i}: max|d mean| {dm:.3g} px, max|d cov| {dc:.3g} px², error/bound {worst:.3g}")
        assert ok, (i, dm, dc, worst)


def test_estimator_without_flip_test_and_swap(lib):
    """BatchPoseEstimator(flip_test=False, swap_rb=False) at 720x1280 — the setting documented
    for decoded frames: crops equal the oracle without the channel swap, est.avg is the
    backbone's maps bit for bit, keypoints are msra_decode of those maps."""
    from mvpose import hrnet, synthetic as syn
    from mvpose.estimator import BatchPoseEstimator
    est = BatchPoseEstimator(hrnet.random_state_dict(41), max_frames=6, flip_test=False, swap_rb=False)
    n = 3
    frames = syn.make_frames(n, seed=47)
    r = est.run(torch.tensor(frames, device="cuda"), argmax=True)
    torch.cuda.synchronize()
    M, center, scale = heatmap_ref.topdown_crop_matrix(1280, 720)
    crops = est.crops[:n].float().cpu().numpy()
    for i in range(n):
        np.testing.assert_array_equal(crops[i, :, :, :3], cases.oracle_crop(frames[i], M, swap_rb=False))
    maps = est.heatmaps[:n].cpu().numpy()
    np.testing.assert_array_equal(est.avg[:n].cpu().numpy().view(np.int32), maps.view(np.int32))
    for i in range(n):
        rk, rs, ri = heatmap_ref.msra_decode(maps[i])
        np.testing.assert_array_equal(r["argmax"][i].cpu().numpy(), ri)
        np.testing.assert_array_equal(r["scores"][i].cpu().numpy(), rs)
        np.testing.assert_array_equal(r["keypoints"][i].cpu().numpy(),
                                      heatmap_ref.keypoints_to_image(rk, center, scale))
