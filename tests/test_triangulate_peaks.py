"""CPU: mvp_triangulate_peaks is declared and exported and rejects bad arguments before any device
work; the numpy reference solves the shared cases to their constructed truth with both margins
above MIN_MARGIN (a condition of the inputs the GPU comparison relies on); the Python and
command-line fronts accept the new options and reject the combinations that make no sense."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import tri_peaks_cases as cases
from tri_peaks_ref import INLIER_PX, MIN_MARGIN, PeaksReference

HEADER = os.path.join(ROOT, "include", "mvpose.h")


def test_header_declares_and_library_exports():
    from mvpose import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ("mvp_triangulate_peaks", "mvp_heatmap_peaks"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src)
        assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES
    assert re.search(r"#define\s+MVP_MAX_PEAKS\s+4\b", src)


def _call(n, M, V, n_cams, idx, inlier_px=10.0, min_conf=0.0):
    from mvpose import _lib
    ci = (ctypes.c_int * len(idx))(*idx)
    rc = _lib.lib.mvp_triangulate_peaks(None, n, M, V, None, n_cams, ci, len(idx), inlier_px, min_conf, None, None,
                                        None, None, None, None)
    return rc, _lib.last_error()


@pytest.mark.parametrize("kw,msg", [
    (dict(idx=[0, 1], M=0), "M=0"),
    (dict(idx=[0, 1], M=5), "M=5"),
    (dict(idx=[0]), "n_cam_idx=1"),
    (dict(idx=[0, 1], inlier_px=0.0), "inlier_px"),
    (dict(idx=[0, 1], inlier_px=float("inf")), "inlier_px"),
    (dict(idx=[0, 1], inlier_px=float("nan")), "inlier_px"),
    (dict(idx=[0, 1], min_conf=float("nan")), "min_conf"),
    (dict(idx=[0, 5]), "cam_idx[1]=5"),
    (dict(idx=[0, -1]), "cam_idx[1]=-1"),
    (dict(idx=[0, 1], n=-1), "n_points"),
])
def test_bad_arguments_are_reported(kw, msg):
    kw = dict(dict(n=10, M=2), **kw)
    rc, err = _call(kw.pop("n"), kw.pop("M"), 2, 2, **kw)
    assert rc == -1
    assert msg in err, err


def test_null_pointers_and_empty_batch():
    rc, err = _call(10, 2, 2, 2, idx=[0, 1])
    assert rc == -1 and "null device pointer" in err
    rc, _ = _call(0, 2, 2, 2, idx=[0, 1])       # n_points == 0 is a no-op, before the pointer checks
    assert rc == 0


# ------------------------------------------------------------------ the shared cases
@pytest.mark.parametrize("V,M", cases.CASES)
def test_cases_are_determined_and_solved(V, M):
    """The reference finds the constructed truth, and no comparison it made is closer than
    MIN_MARGIN to flipping: the GPU test may then demand equal masks and selections."""
    cams, peaks, tmask, tslot, ref, (xyz, mask, sel, err) = cases.case_with_reference(V, M)
    print(f"V={V} M={M}: margin {ref.margin:.3g} px, candidate gap {ref.gap:.3g} px")
    assert ref.margin > MIN_MARGIN and ref.gap > MIN_MARGIN
    assert np.array_equal(mask, tmask) and np.array_equal(sel, tslot)
    assert (mask.sum(-1) >= 3).all() and np.isfinite(xyz).all()
    assert (V == 3 or (~tmask).any()) and (tslot > 0).any()      # V = 3 keeps all three views (kind 0 only)
    assert (err[mask] <= INLIER_PX).all()
    k = ref.select(peaks, mask, sel)
    for v in range(V):
        chosen = np.take_along_axis(peaks[..., v], np.maximum(tslot[..., v], 0)[..., None, None].astype(np.int64), -2)
        want = np.where(tmask[..., v, None], chosen[..., 0, :], peaks[:, :, 0, :, v])
        assert np.array_equal(k[..., v], want, equal_nan=True)


def test_reference_with_one_slot_is_the_robust_reference():
    from test_triangulate_robust_gpu import Reference, contaminated
    cams, k, truth = contaminated(4, 2, max_bad=1, frames=4)
    rx, rm, re_ = Reference(cams, [0, 1, 2, 3])(k)
    ref = PeaksReference(cams, [0, 1, 2, 3])
    px, pm, ps, pe = ref(k[:, :, None])
    assert np.array_equal(pm, rm) and np.array_equal(pm, truth)
    assert np.array_equal(px.view(np.uint32), rx.view(np.uint32))
    assert np.array_equal(ps, np.where(rm, 0, -1))
    np.testing.assert_allclose(pe, re_, rtol=1e-6, atol=1e-6, equal_nan=True)
    assert np.array_equal(ref.select(k[:, :, None], pm, ps), k, equal_nan=True)


# ------------------------------------------------------------------ fronts
def test_modes_and_methods():
    from mvpose import ops, pipeline, pose_estimation
    assert ops.TRI_PEAKS not in (ops.TRI_REFERENCE, ops.TRI_ALL_VIEWS, ops.TRI_ROBUST)
    assert ops.TRI_PEAKS & (ops.TRI_EXACT_JACOBI | ops.TRI_TOLERANCE) == 0
    assert ops.MAX_PEAKS == 4
    assert "peaks" in pose_estimation.TRIANGULATION_METHODS
    with pytest.raises(ValueError, match="peaks"):      # method="peaks" needs the peaks
        pose_estimation.get_pose_3D({}, np.zeros((1, 17, 3, 3), np.float32), camera_indices=[0, 1, 2],
                                    method="peaks")
    with pytest.raises(ValueError, match="heatmap"):    # the moments describe the mixture, not the mode
        pipeline.MultiViewPipeline({}, estimator=object(), mode=ops.TRI_PEAKS, refine="heatmap")
    with pytest.raises(ValueError):                     # tri_solver does not apply, as for TRI_ROBUST
        pipeline.MultiViewPipeline({}, estimator=object(), mode=ops.TRI_PEAKS, tri_solver="reference_compat")
    with pytest.raises(ValueError, match="max_peaks"):
        pipeline.MultiViewPipeline({}, estimator=object(), mode=ops.TRI_PEAKS, max_peaks=5)
    with pytest.raises(ValueError, match="heatmap"):    # likewise in the drop-ins, peaks given or not yet loaded
        pose_estimation.get_pose_3D({}, np.zeros((1, 17, 3, 3), np.float32), camera_indices=[0, 1, 2], method="peaks",
                                    peaks=np.zeros((1, 17, 2, 3, 3), np.float32), refine="heatmap",
                                    heatmaps_2d=np.zeros((1, 3, 17, 6)))
    with pytest.raises(ValueError, match='refine="heatmap" does not apply'):
        pose_estimation.estimate_pose_from_video(["a", "b", "c"], ["x", "y", "z"], None, triangulation="peaks",
                                                 refine="heatmap")
    # a valid preset: the peak lists are not carried through the label exchange
    with pytest.raises(ValueError, match="fix_swaps does not apply"):
        pose_estimation.estimate_pose_from_video(["a", "b", "c"], ["x", "y", "z"], None, triangulation="peaks",
                                                 fix_swaps="limbs")


def test_cli_parser_accepts_the_new_flags():
    from mvpose import cli
    p = cli.record_and_estimate_pose_parser(extensions=True)
    a = p.parse_args(["--camera_names", "a", "b", "c", "--triangulation", "peaks", "--max_peaks", "3",
                      "--peak_threshold", "0.2", "--peak_min_rel", "0.4"])
    assert (a.triangulation, a.max_peaks, a.peak_threshold, a.peak_min_rel) == ("peaks", 3, 0.2, 0.4)
    d = p.parse_args(["--camera_names", "a", "b"])
    assert d.max_peaks is None and d.peak_threshold is None and d.peak_min_rel is None   # function defaults apply


def test_apply_frame_offsets_takes_the_camera_axis():
    """Peaks (T, J, M, 3, V) take the per-camera offsets kpts_2d (T, J, 3, V) takes."""
    from mvpose import sync
    rng = np.random.default_rng(0)
    pk = rng.normal(size=(9, 17, 2, 3, 3)).astype(np.float32)
    off = [0, 2, -1]
    (out,), first = sync.apply_frame_offsets([pk], off, (4,))
    for m in range(2):
        (want,), first_m = sync.apply_frame_offsets([pk[:, :, m]], off, (3,))
        assert np.array_equal(out[:, :, m], want) and np.array_equal(first, first_m)
