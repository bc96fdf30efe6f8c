"""torch-tensor front of the libmvpose C-ABI.

Device tensors are handed over as raw pointers with the current HIP stream;
the library enqueues stream-ordered kernels.  Shapes and dtypes are checked
here before any launch (the kernels assume them).
"""
from __future__ import annotations

import ctypes
from typing import Sequence

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream

CAM_DOUBLES = 40
TRI_REFERENCE = 0
TRI_ALL_VIEWS = 1
TRI_EXACT_JACOBI = 0x10  # mode flag: exact Jacobi SVD for every point (mvpose.h)
TRI_TOLERANCE = 0x20     # mode flag: throughput solver, certified bit-identical to the exact path (mvpose.h)
TRI_ROBUST = 2           # Python-level only (MultiViewPipeline mode): triangulate_robust, never an mvp_triangulate mode
TRI_PEAKS = 3            # Python-level only (MultiViewPipeline mode): heatmap_peaks + triangulate_peaks
MAX_PEAKS = 4            # mvpose.h MVP_MAX_PEAKS
REFINE_W_UNIT = 0        # mvp_triangulate_refine weights (mvpose.h MVP_REFINE_W_*)
REFINE_W_CONF = 1
REFINE_W_GAUSS = 2
REFINE_WEIGHTS = {"unit": REFINE_W_UNIT, "conf": REFINE_W_CONF, "heatmap": REFINE_W_GAUSS}


def _require(t: torch.Tensor, dtype, name: str):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_cuda:
        raise ValueError(f"{name} must live on the GPU (no CPU fallback)")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def _tri_args(kpts: torch.Tensor, cams: torch.Tensor, cam_idx: Sequence[int]):
    """The triangulation fronts' shared checks: kpts (..., 3, V) float32 and cams (n_cams, 40)
    float64, both on the GPU.  Returns V, the leading shape, its number of points and cam_idx as
    a ctypes int array."""
    _require(kpts, torch.float32, "kpts")
    _require(cams, torch.float64, "cams")
    if kpts.dim() < 2 or kpts.shape[-2] != 3:
        raise ValueError(f"kpts must be (..., 3, V), got {tuple(kpts.shape)}")
    if cams.dim() != 2 or cams.shape[1] != CAM_DOUBLES:
        raise ValueError(f"cams must be (n_cams, {CAM_DOUBLES}), got {tuple(cams.shape)}")
    lead = tuple(kpts.shape[:-2])
    n = int(np.prod(lead)) if lead else 1
    ci = (ctypes.c_int * len(cam_idx))(*[int(c) for c in cam_idx])
    return kpts.shape[-1], lead, n, ci


def _pack_view_bits(mask: torch.Tensor) -> torch.Tensor:
    """(..., NV) bool -> (...) uint8 with bit i set for view i: the kernels' per-point view mask."""
    place = torch.tensor([1 << i for i in range(mask.shape[-1])], dtype=torch.int32, device=mask.device)
    return (mask.to(torch.int32) * place).sum(-1).to(torch.uint8).contiguous()


def _unpack_view_bits(bits: torch.Tensor, nv: int) -> torch.Tensor:
    """_pack_view_bits' inverse: (...) uint8 -> (..., nv) bool."""
    shifts = torch.arange(nv, dtype=torch.uint8, device=bits.device)
    return ((bits.unsqueeze(-1) >> shifts) & 1).to(torch.bool)


def _obs_args(kpts, cams, cam_idx, xyz, weights, gauss, mask, min_conf, cov_floor, *, xyz_name="xyz", frames=False,
              free=None):
    """Shared front of the reprojection-error solvers (triangulate_refine, bundle_adjust*,
    trajectory_fit*, skeleton_fit*): the checks of kpts (..., 3, V), cams, cam_idx, xyz (..., 3),
    weights, gauss (T, V, J, 6) and mask (..., NV), and the packed arguments.  frames: kpts must be
    (T, P, 3, V), and the C call takes T, P in place of the point count and no J (the fits); free: the
    view positions whose bit mask follows n_cam_idx (the bundle adjustment).  Returns (lead, the number of
    points, nv, args, bits): args is the C call's leading arguments, kpts_dev .. cov_floor; bits is the
    packed mask that args points into, which the caller holds until it has made the call."""
    if weights not in REFINE_WEIGHTS:
        raise ValueError(f"weights {weights!r}: one of {tuple(REFINE_WEIGHTS)}")
    V, lead, n, ci = _tri_args(kpts, cams, cam_idx)
    if frames and len(lead) != 2:
        raise ValueError(f"kpts must be (T, P, 3, V), got {tuple(kpts.shape)}")
    nv = len(ci)
    _require(xyz, torch.float32, xyz_name)
    if tuple(xyz.shape) != lead + (3,):
        raise ValueError(f"{xyz_name} must be {lead + (3,)}, got {tuple(xyz.shape)}")
    J = 0
    if weights == "heatmap":
        if gauss is None:
            raise ValueError('weights="heatmap" needs gauss, the (T, V, J, 6) float64 heatmap Gaussians')
        _require(gauss, torch.float64, "gauss")
        if len(lead) != 2 or tuple(gauss.shape) != (lead[0], V, lead[1], 6):
            raise ValueError(f"gauss must be (T, V, J, 6) = {(lead[0] if lead else None, V, lead[-1] if lead else None, 6)} "
                             f"for kpts (T, J, 3, V), got {tuple(gauss.shape)}")
        J = lead[1]
    bits = None
    if mask is not None:
        _require(mask, torch.bool, "mask")
        if tuple(mask.shape) != lead + (nv,):
            raise ValueError(f"mask must be {lead + (nv,)}, got {tuple(mask.shape)}")
        bits = _pack_view_bits(mask)
    args = ((ptr(kpts),) + ((int(lead[0]), int(lead[1])) if frames else (n,)) + (V, ptr(cams), cams.shape[0], ci, nv)
            + (() if free is None else (_free_mask(free),))
            + (ptr(xyz), ptr(bits), REFINE_WEIGHTS[weights], ptr(gauss) if weights == "heatmap" else None)
            + (() if frames else (int(J),)) + (float(min_conf), float(cov_floor)))
    return lead, n, nv, args, bits


def pack_camera(K, R, T, dist) -> np.ndarray:
    """One MVP_CAM_DOUBLES record: [K | dist | R | T | P | pad] with
    P = np.dot(K, hstack(R, T)) exactly as reference utils.py:1318-1319 — in the parameters'
    own dtype (float32 camera tensors give the reference a float32 P, e.g. the extrinsic
    branch's decomposed parameters, pose_refinement.py:808-811), stored as float64."""
    P = np.dot(np.asarray(K), np.hstack((np.asarray(R), np.asarray(T).reshape(-1, 1))))
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    T = np.asarray(T, dtype=np.float64).reshape(3, 1)
    d = np.zeros(5)
    dd = np.asarray(dist, dtype=np.float64).ravel()
    d[: min(5, dd.size)] = dd[:5]
    if dd.size > 5 and np.any(dd[5:] != 0):
        raise ValueError("only the 5-coefficient Brown-Conrady model is supported (reference calibration)")
    rec = np.zeros(CAM_DOUBLES)
    rec[0:9] = K.ravel()
    rec[9:14] = d
    rec[14:23] = R.ravel()
    rec[23:26] = T.ravel()
    rec[26:38] = np.asarray(P, dtype=np.float64).ravel()
    return rec


def pack_cameras(camera_params) -> np.ndarray:
    """camera_params: {idx: [K, R, T, dist]} (utils.get_params_from_name order) or a
    list of such lists, ordered by camera key.  Returns (n, 40) float64."""
    if isinstance(camera_params, dict):
        items = [camera_params[k] for k in camera_params]
    else:
        items = list(camera_params)
    return np.stack([pack_camera(K, R, T, dist) for (K, R, T, dist) in items])


def triangulate(kpts: torch.Tensor, cams: torch.Tensor, cam_idx: Sequence[int] = (0, 1),
                mode: int = TRI_REFERENCE, out: torch.Tensor | None = None,
                return_xyzw: bool = False, exact: bool = False, tolerance: bool = False):
    """kpts (..., 3, V) float32 on GPU (reference layout) -> (..., 3) float32.

    cams: (n_cams, 40) float64 on GPU (pack_cameras).  Every solver returns the exact path's
    float32 bits (OpenCV 4.9's rounding sequence restated).  Default: QR + inverse iteration,
    the Jacobi restatement where that has not converged or is not certified; exact=True: the
    JacobiSVDImpl_ restatement for every point; tolerance=True: the throughput solver
    (MVP_TRI_TOLERANCE, reference mode with two listed cameras), certified per point, the
    exact path by a second launch where it is not.  The certification bound is empirical (its
    rounding-floor constants were fitted on 1.4 M synthetic and random points, with margin; see
    include/mvpose.h MVP_TRI_TOLERANCE): pass exact=True where a proof of bit-identity is
    required.  return_xyzw: the float64 null vectors
    (diagnostic; bit-identical to the exact path's only where that path solved the point —
    every point in tolerance mode)."""
    if exact and tolerance:
        raise ValueError("exact and tolerance exclude each other")
    if exact:
        mode = int(mode) | TRI_EXACT_JACOBI
    if tolerance:
        mode = int(mode) | TRI_TOLERANCE
    V, lead, n, ci = _tri_args(kpts, cams, cam_idx)
    if out is None:
        out = torch.empty(lead + (3,), dtype=torch.float32, device=kpts.device)
    else:
        _require(out, torch.float32, "out")
        if tuple(out.shape) != lead + (3,):
            raise ValueError("out has the wrong shape")
    xyzw = torch.empty(lead + (4,), dtype=torch.float64, device=kpts.device) if return_xyzw else None
    call("mvp_triangulate", ptr(kpts), n, V, ptr(cams), cams.shape[0], ci, len(ci), int(mode),
         ptr(out), ptr(xyzw), stream(kpts.device))
    return (out, xyzw) if return_xyzw else out


def triangulate_robust(kpts: torch.Tensor, cams: torch.Tensor, cam_idx: Sequence[int], inlier_px: float = 10.0,
                       min_conf: float = 0.0, return_err: bool = True):
    """N-view triangulation with per-point outlier-view rejection (mvp_triangulate_robust; the
    algorithm is stated in include/mvpose.h; no reference counterpart).

    kpts (..., 3, V) float32 on GPU, cams (n_cams, 40) float64 on GPU; view i reads column
    cam_idx[i] with camera cam_idx[i]'s parameters, as TRI_ALL_VIEWS does.  Returns
    (xyz (..., 3) float32, inliers (..., NV) bool, err (..., NV) float32 or None): the point
    triangulated from its inlier views (bit-identical to the all-views DLT over exactly those
    views; NaN where fewer than two views agree within inlier_px), the views used, and every
    valid view's reprojection error in undistorted pixels against the returned point (+inf
    behind the camera, NaN for views that are not finite or below min_conf)."""
    V, lead, n, ci = _tri_args(kpts, cams, cam_idx)
    nv = len(ci)
    out = torch.empty(lead + (3,), dtype=torch.float32, device=kpts.device)
    bits = torch.empty(lead, dtype=torch.uint8, device=kpts.device)
    err = torch.empty(lead + (nv,), dtype=torch.float32, device=kpts.device) if return_err else None
    call("mvp_triangulate_robust", ptr(kpts), n, V, ptr(cams), cams.shape[0], ci, nv, float(inlier_px),
         float(min_conf), ptr(out), ptr(bits), ptr(err), stream(kpts.device))
    return out, _unpack_view_bits(bits, nv), err


def heatmap_peaks(heatmaps: torch.Tensor, center_scale: torch.Tensor, *, max_peaks: int = 4, radius: int = 1,
                  thr: float = 0.1, min_rel: float = 0.3, n_views: int = 1, input_size=(192, 256)):
    """Up to max_peaks local maxima of every heatmap, decoded like the argmax (mvp_heatmap_peaks; the
    peak definition is stated in include/mvpose.h; no reference counterpart).

    heatmaps (N, K, H, W) float32 on GPU: the maps the decode looks at (BatchPoseEstimator.run's
    "heatmaps"), crops ordered (t, v) when n_views > 1; center_scale (N, 4) float32 (cx, cy, sw,
    sh); input_size the network input (w, h).  A peak exceeds thr, beats its (2·radius+1)² window
    and, after the first, reaches min_rel times the first.  Returns (peaks (N/V, K, max_peaks, 3,
    V) float32 [x, y, score] in image pixels, best first — peaks[:, :, m] has the kpts_2d layout,
    unfilled slots x = y = NaN, score 0 — and counts (N/V, K, V) int32)."""
    _require(heatmaps, torch.float32, "heatmaps")
    _require(center_scale, torch.float32, "center_scale")
    if heatmaps.dim() != 4:
        raise ValueError(f"heatmaps must be (N, K, H, W), got {tuple(heatmaps.shape)}")
    N, K, H, W = heatmaps.shape
    if tuple(center_scale.shape) != (N, 4):
        raise ValueError(f"center_scale must be ({N}, 4), got {tuple(center_scale.shape)}")
    M, V = int(max_peaks), int(n_views)
    if V < 1 or N % V:
        raise ValueError(f"n_views={V} does not divide the {N} crops")
    if not 1 <= M <= MAX_PEAKS:
        raise ValueError(f"max_peaks={M}: 1..{MAX_PEAKS}")
    peaks = torch.empty((N // V, K, M, 3, V), dtype=torch.float32, device=heatmaps.device)
    counts = torch.empty((N // V, K, V), dtype=torch.int32, device=heatmaps.device)
    call("mvp_heatmap_peaks", ptr(heatmaps), N, K, H, W, ptr(center_scale), int(input_size[0]), int(input_size[1]),
         M, int(radius), float(thr), float(min_rel), V, ptr(peaks), ptr(counts), stream(heatmaps.device))
    return peaks, counts


def triangulate_peaks(peaks: torch.Tensor, cams: torch.Tensor, cam_idx: Sequence[int], inlier_px: float = 10.0,
                      min_conf: float = 0.0):
    """triangulate_robust over several candidates per view, choosing one per inlier view
    (mvp_triangulate_peaks; the algorithm is stated in include/mvpose.h; no reference counterpart).

    peaks (..., M, 3, V) float32 on GPU (heatmap_peaks' layout: slot m of a point is a kpts
    column set), cams and cam_idx as for triangulate_robust.  Returns (xyz (..., 3) float32,
    inliers (..., NV) bool, sel (..., NV) int8: the slot each inlier view used, -1 otherwise,
    err (..., NV) float32: the selected candidate's reprojection error, for a valid view outside
    the mask its nearest candidate's, and kpts (..., 3, V) float32: slot 0 with the inlier views'
    columns replaced by their selected candidates — a kpts_2d for every later stage).  With
    M = 1 xyz and inliers are triangulate_robust's bit for bit and kpts is the input."""
    _require(peaks, torch.float32, "peaks")
    if peaks.dim() < 3 or peaks.shape[-2] != 3 or not 1 <= peaks.shape[-3] <= MAX_PEAKS:
        raise ValueError(f"peaks must be (..., M, 3, V) with 1 <= M <= {MAX_PEAKS}, got {tuple(peaks.shape)}")
    M = int(peaks.shape[-3])
    V, _, _, ci = _tri_args(peaks, cams, cam_idx)
    lead = tuple(peaks.shape[:-3])
    n = int(np.prod(lead)) if lead else 1
    nv = len(ci)
    dev = peaks.device
    out = torch.empty(lead + (3,), dtype=torch.float32, device=dev)
    bits = torch.empty(lead, dtype=torch.uint8, device=dev)
    sel = torch.empty(lead + (nv,), dtype=torch.int8, device=dev)
    err = torch.empty(lead + (nv,), dtype=torch.float32, device=dev)
    kpts = torch.empty(lead + (3, V), dtype=torch.float32, device=dev)
    call("mvp_triangulate_peaks", ptr(peaks), n, M, V, ptr(cams), cams.shape[0], ci, nv, float(inlier_px),
         float(min_conf), ptr(out), ptr(bits), ptr(sel), ptr(err), ptr(kpts), stream(dev))
    return out, _unpack_view_bits(bits, nv), sel, err, kpts


def triangulate_refine(kpts: torch.Tensor, cams: torch.Tensor, cam_idx: Sequence[int], xyz0: torch.Tensor, *,
                       weights: str = "unit", gauss: torch.Tensor | None = None, mask: torch.Tensor | None = None,
                       min_conf: float = 0.0, cov_floor: float = 1.0, max_iter: int = 10, tol: float = 1e-7):
    """Maximum-likelihood refinement of triangulated points with their 3D covariance
    (mvp_triangulate_refine; the algorithm is stated in include/mvpose.h; no reference counterpart).

    kpts (..., 3, V) float32, cams (n_cams, 40) float64, cam_idx as for triangulate_robust; xyz0
    (..., 3) float32 seed from any triangulator.  weights: "unit" (every view alike), "conf" (the
    keypoint confidences) or "heatmap" (each view's own 2D Gaussian: gauss (T, V, J, 6) float64,
    the heatmaps_2d layout, with kpts (T, J, 3, V); cov_floor px² is added to its variances).
    mask: (..., NV) bool, the views that may be used (triangulate_robust's inliers), or None.
    Levenberg-Marquardt on the Mahalanobis reprojection error of the raw, distorted pixels, at
    most max_iter trials, converged at a step <= tol·(|X| + tol).  Returns (xyz (..., 3) float32,
    cov (..., 3, 3) float32 symmetric, world units², cost (...) float32, status (...) uint8: bits
    0-5 trials, 0x40 not converged, 0x80 failed).  A failed point (fewer than 2 usable views, a
    seed that is not finite or behind a camera) returns its seed, NaN cov and cost.  With equal
    isotropic noise in every view this does not beat the DLT seed: the gain is in the weighting
    and in the covariance."""
    lead, _, _, args, _bits = _obs_args(kpts, cams, cam_idx, xyz0, weights, gauss, mask, min_conf, cov_floor,
                                        xyz_name="xyz0")
    out = torch.empty(lead + (3,), dtype=torch.float32, device=kpts.device)
    cov6 = torch.empty(lead + (6,), dtype=torch.float32, device=kpts.device)
    cost = torch.empty(lead, dtype=torch.float32, device=kpts.device)
    status = torch.empty(lead, dtype=torch.uint8, device=kpts.device)
    call("mvp_triangulate_refine", *args, int(max_iter), float(tol), ptr(out), ptr(cov6), ptr(cost), ptr(status),
         stream(kpts.device))
    sym = torch.tensor([0, 1, 2, 1, 3, 4, 2, 4, 5], device=kpts.device)
    cov = cov6.index_select(-1, sym).reshape(lead + (3, 3))
    return out, cov, cost, status


def triangulate_fallback_total(device=None) -> int:
    """Points the MVP_TRI_TOLERANCE solver has re-solved on the exact path on the current stream
    so far (mvp_triangulate_fallback_total; synchronises the stream)."""
    out = ctypes.c_ulonglong(0)
    call("mvp_triangulate_fallback_total", stream(device), ctypes.byref(out))
    return int(out.value)


def triangulate_points_f64(kpts: torch.Tensor, cams: torch.Tensor, return_xyzw: bool = False):
    """utils.triangulate_points on float64 keypoints (mvp_triangulate_points_f64): kpts
    (..., 2, 2) float64 [view][x, y] on GPU, cams (2, 40) float64 (camera 1, camera 2) ->
    (..., 3) float64, OpenCV's CV_64F semantics end to end."""
    _require(kpts, torch.float64, "kpts")
    _require(cams, torch.float64, "cams")
    if kpts.dim() < 2 or tuple(kpts.shape[-2:]) != (2, 2):
        raise ValueError(f"kpts must be (..., 2, 2), got {tuple(kpts.shape)}")
    if tuple(cams.shape) != (2, CAM_DOUBLES):
        raise ValueError(f"cams must be (2, {CAM_DOUBLES}), got {tuple(cams.shape)}")
    lead = tuple(kpts.shape[:-2])
    n = int(np.prod(lead)) if lead else 1
    out = torch.empty(lead + (3,), dtype=torch.float64, device=kpts.device)
    xyzw = torch.empty(lead + (4,), dtype=torch.float64, device=kpts.device) if return_xyzw else None
    call("mvp_triangulate_points_f64", ptr(kpts), n, ptr(cams), ptr(out),
         ptr(xyzw), stream(kpts.device))
    return (out, xyzw) if return_xyzw else out


def _smooth_inputs(xyz, cov, valid):
    """The checks trajectory_smooth makes of (xyz, cov, valid): T, P, the (T, P, 6) covariance and the
    uint8 mask (or None)."""
    _require(xyz, torch.float32, "xyz")
    if xyz.dim() != 3 or xyz.shape[2] != 3:
        raise ValueError(f"xyz must be (T, P, 3), got {tuple(xyz.shape)}")
    T, P = int(xyz.shape[0]), int(xyz.shape[1])
    cov6 = None
    if cov is not None:
        if not isinstance(cov, torch.Tensor) or cov.dtype != torch.float32 or not cov.is_cuda:
            raise TypeError("cov must be a float32 torch.Tensor on the GPU")
        if tuple(cov.shape) == (T, P, 3, 3):
            cov6 = cov.reshape(T, P, 9)[..., [0, 1, 2, 4, 5, 8]].contiguous()
        elif tuple(cov.shape) == (T, P, 6):
            cov6 = cov.contiguous()
        else:
            raise ValueError(f"cov must be {(T, P, 3, 3)} or {(T, P, 6)}, got {tuple(cov.shape)}")
    v8 = None
    if valid is not None:
        if not isinstance(valid, torch.Tensor) or valid.dtype not in (torch.bool, torch.uint8) or not valid.is_cuda:
            raise TypeError("valid must be a bool or uint8 torch.Tensor on the GPU")
        if tuple(valid.shape) != (T, P):
            raise ValueError(f"valid must be {(T, P)}, got {tuple(valid.shape)}")
        v8 = valid.to(torch.uint8).contiguous()
    return T, P, cov6, v8


def _plan3(name: str, *ints):
    """A *_plan call of the time-parallel solvers: (chunk used, chunks per chain, workspace bytes)."""
    used, n_chunks, nbytes = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int64(0)
    call(name, *[int(i) for i in ints], ctypes.byref(used), ctypes.byref(n_chunks), ctypes.byref(nbytes))
    return used.value, n_chunks.value, nbytes.value


def trajectory_smooth_plan(T: int, P: int, chunk: int = 0):
    """What trajectory_smooth will use for (T, P, chunk) (mvp_trajectory_smooth_plan): the chunk
    length, the chunks per chain and the workspace bytes."""
    return _plan3("mvp_trajectory_smooth_plan", T, P, chunk)


def trajectory_smooth(xyz: torch.Tensor, cov: torch.Tensor | None = None, valid: torch.Tensor | None = None, *,
                      lambda_smooth: float = 1.0, sigma0: float = 1.0, cov_floor: float = 0.0, chunk: int = 0,
                      want_resid: bool = True, want_observed: bool = True, want_status: bool = True):
    """Covariance-weighted trajectory smoothing with gap filling (mvp_trajectory_smooth; the
    problem is stated in include/mvpose.h; no reference counterpart).

    xyz (T, P, 3) float32 on the GPU; cov (T, P, 3, 3) or (T, P, 6) float32 (the upper triangle
    xx, xy, xz, yy, yz, zz is the one read) or None (every observed frame then weighs
    I / sigma0²); valid (T, P) bool or uint8 or None.  Per chain p the minimiser of
    ½ Σ (X_t − z_t)ᵀ W_t (X_t − z_t) + ½ lambda_smooth Σ |X_t − 2 X_{t−1} + X_{t−2}|² with
    W_t = (cov_t + cov_floor·I)⁻¹ on observed frames and 0 elsewhere: gaps are filled, the ends
    continue as straight lines.  chunk: frames per lane of the time-parallel solve, 0 = automatic.
    Returns (xyz (T, P, 3) float32, resid (T, P) float32 squared Mahalanobis distance of each
    observed frame to the smooth track (NaN elsewhere), observed (T, P) bool, status (P,) uint8:
    0, or 0x80 for a chain with fewer than 2 observed frames, which returns its input).  An
    output switched off by its want_* flag comes back as None.  The workspace is a torch.empty on
    the call's stream, sized by trajectory_smooth_plan."""
    T, P, cov6, v8 = _smooth_inputs(xyz, cov, valid)
    _, _, nbytes = trajectory_smooth_plan(T, P, chunk)
    dev = xyz.device
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty_like(xyz)
    resid = torch.empty((T, P), dtype=torch.float32, device=dev) if want_resid else None
    observed = torch.empty((T, P), dtype=torch.uint8, device=dev) if want_observed else None
    status = torch.empty((P,), dtype=torch.uint8, device=dev) if want_status else None
    call("mvp_trajectory_smooth", ptr(xyz), ptr(cov6), ptr(v8), T, P, float(lambda_smooth), float(sigma0),
         float(cov_floor), int(chunk), ptr(work), int(nbytes), ptr(out), ptr(resid), ptr(observed), ptr(status),
         stream(dev))
    return out, resid, observed.to(torch.bool) if observed is not None else None, status


def trajectory_smooth_cov_plan(T: int, P: int, chunk: int = 0):
    """What trajectory_smooth_cov will use for (T, P, chunk) (mvp_trajectory_smooth_cov_plan): the
    chunk length, the chunks per chain and the workspace bytes."""
    return _plan3("mvp_trajectory_smooth_cov_plan", T, P, chunk)


def trajectory_smooth_cov(xyz: torch.Tensor, cov: torch.Tensor | None = None, valid: torch.Tensor | None = None, *,
                          lambda_smooth: float = 1.0, sigma0: float = 1.0, cov_floor: float = 0.0, chunk: int = 0,
                          want_cross: bool = True, want_status: bool = True):
    """Posterior covariance of trajectory_smooth's result (mvp_trajectory_smooth_cov; stated in
    include/mvpose.h): the blocks of Σ = A⁻¹, A the smoother's matrix for the same arguments.

    Arguments as for trajectory_smooth; the coordinates count only through being finite.  Returns
    (cov (T, P, 6) float32: (xx, xy, xz, yy, yz, zz) of Σ_{t,t}, for every frame, observed or not;
    cross (T, P, 3, 3) float32: Σ_{t,t+1}, row = coordinate of X_t, NaN at t = T−1, or None without
    want_cross; status (P,) uint8: 0, or 0x80 for a failed chain, whose blocks are all NaN), in world
    units², all on the GPU.  Stream-ordered, no host synchronisation."""
    T, P, cov6, v8 = _smooth_inputs(xyz, cov, valid)
    _, _, nbytes = trajectory_smooth_cov_plan(T, P, chunk)
    dev = xyz.device
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty((T, P, 6), dtype=torch.float32, device=dev)
    cross = torch.empty((T, P, 3, 3), dtype=torch.float32, device=dev) if want_cross else None
    status = torch.empty((P,), dtype=torch.uint8, device=dev) if want_status else None
    call("mvp_trajectory_smooth_cov", ptr(xyz), ptr(cov6), ptr(v8), T, P, float(lambda_smooth), float(sigma0),
         float(cov_floor), int(chunk), ptr(work), int(nbytes), ptr(out), ptr(cross), ptr(status), stream(dev))
    return out, cross, status


def epipolar_lag_cost_plan(T: int, J: int, nv: int, max_lag: int):
    """What epipolar_lag_cost will use for (T, J, nv, max_lag) (mvp_epipolar_lag_cost_plan): the
    kernel's time tile in frames and the workspace bytes."""
    tile, nbytes = ctypes.c_int(0), ctypes.c_int64(0)
    call("mvp_epipolar_lag_cost_plan", int(T), int(J), int(nv), int(max_lag), ctypes.byref(tile),
         ctypes.byref(nbytes))
    return tile.value, nbytes.value


def epipolar_lag_cost(kpts: torch.Tensor, cams: torch.Tensor, cam_idx: Sequence[int], max_lag: int,
                      min_conf: float = 0.0, trunc_px: float = 20.0):
    """The epipolar lag-cost scan of pose-based frame synchronisation (mvp_epipolar_lag_cost; the
    problem is stated in include/mvpose.h; no reference counterpart).

    kpts (T, J, 3, V) float32 on the GPU, cams (n_cams, 40) float64 on the GPU; view i reads column
    cam_idx[i] with camera cam_idx[i]'s parameters, as triangulate_robust does.  For every pair
    (a, b), a < b, of listed views and every lag l in [-max_lag, max_lag]: the sum over frames t
    and joints of min(d², trunc_px²), d the Sampson distance in undistorted pixels between view
    a's keypoint at frame t and view b's at frame t + l, over the terms whose two keypoints are
    usable (finite, conf >= min_conf).  Returns (sum (NP, 2·max_lag+1) float64, cnt likewise
    int64, pairs: the NP (a, b) tuples in row order).  The workspace is a torch.empty on the
    call's stream, sized by epipolar_lag_cost_plan."""
    V, lead, n, ci = _tri_args(kpts, cams, cam_idx)
    if len(lead) != 2:
        raise ValueError(f"kpts must be (T, J, 3, V), got {tuple(kpts.shape)}")
    T, J = int(lead[0]), int(lead[1])
    nv = len(ci)
    pairs = [(a, b) for a in range(nv) for b in range(a + 1, nv)]
    _, nbytes = epipolar_lag_cost_plan(T, J, nv, max_lag)
    dev = kpts.device
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    nl = 2 * int(max_lag) + 1
    out_sum = torch.empty((len(pairs), nl), dtype=torch.float64, device=dev)
    out_cnt = torch.empty((len(pairs), nl), dtype=torch.int64, device=dev)
    call("mvp_epipolar_lag_cost", ptr(kpts), T, J, V, ptr(cams), cams.shape[0], ci, nv, int(max_lag),
         float(min_conf), float(trunc_px), ptr(work), int(nbytes), ptr(out_sum), ptr(out_cnt), stream(dev))
    return out_sum, out_cnt, pairs


def associate_views_plan(T: int, P: int, J: int, nv: int, *, min_conf: float = 0.0, trunc_px: float = 20.0,
                         max_cost_px: float = 8.0, min_joints: int = 5):
    """What associate_views will use for (T, P, J, nv) (mvp_associate_views_plan, which refuses
    what the call refuses): the LDS bytes of a frame's workgroup and the workspace bytes."""
    lds, nbytes = ctypes.c_int(0), ctypes.c_int64(0)
    call("mvp_associate_views_plan", int(T), int(P), int(J), int(nv), float(min_conf), float(trunc_px),
         float(max_cost_px), int(min_joints), ctypes.byref(lds), ctypes.byref(nbytes))
    return lds.value, nbytes.value


def associate_views(kpts: torch.Tensor, cams: torch.Tensor, cam_idx: Sequence[int], *, min_conf: float = 0.0,
                    trunc_px: float = 20.0, max_cost_px: float = 8.0, min_joints: int = 5,
                    return_affinity: bool = False):
    """Which 2D skeletons of the listed views are the same person (mvp_associate_views; the
    problem is stated in include/mvpose.h; no reference counterpart).

    kpts (T, P, J, 3, V) float32 on the GPU: kpts[:, p] is the kpts_2d layout of person slot p;
    slots are independent per view and an empty slot is NaN.  cams (n_cams, 40) float64 on the
    GPU; view i reads column cam_idx[i] with camera cam_idx[i]'s parameters, as triangulate_robust
    does.  Per frame, nodes (view, slot) with at least min_joints usable keypoints (finite,
    conf >= min_conf) are grouped by complete-linkage agglomeration on the mean truncated squared
    Sampson distance of their common joints, merging while the link is <= max_cost_px² and never
    two nodes of one view.  Returns (group (T, NV, P) int8: the node's group number, -1 for a node
    that is not usable, groups ordered by (-views, smallest node); count (T, 2) uint8: groups and
    groups seen by at least two views; affinity (T, NP, P, P) float64 with -1 for undefined, or
    None; pairs: the NP (a, b) tuples in row order).  The workspace is a torch.empty on the call's
    stream, sized by associate_views_plan."""
    V, lead, n, ci = _tri_args(kpts, cams, cam_idx)
    if len(lead) != 3:
        raise ValueError(f"kpts must be (T, P, J, 3, V), got {tuple(kpts.shape)}")
    T, P, J = (int(d) for d in lead)
    nv = len(ci)
    pairs = [(a, b) for a in range(nv) for b in range(a + 1, nv)]
    _, nbytes = associate_views_plan(T, P, J, nv, min_conf=min_conf, trunc_px=trunc_px, max_cost_px=max_cost_px,
                                     min_joints=min_joints)
    dev = kpts.device
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    group = torch.empty((T, nv, P), dtype=torch.int8, device=dev)
    count = torch.empty((T, 2), dtype=torch.uint8, device=dev)
    aff = torch.empty((T, len(pairs), P, P), dtype=torch.float64, device=dev) if return_affinity else None
    call("mvp_associate_views", ptr(kpts), T, P, J, V, ptr(cams), cams.shape[0], ci, nv, float(min_conf),
         float(trunc_px), float(max_cost_px), int(min_joints), ptr(work), int(nbytes), ptr(group), ptr(count),
         ptr(aff), stream(dev))
    return group, count, aff, pairs


def _swap_lists(pairs, units):
    """pairs (NS, 2), units (NS,) -> (NS, U, the two ctypes int arrays); the library checks the values."""
    pairs = np.asarray(pairs, dtype=np.int64)
    units = np.asarray(units, dtype=np.int64).ravel()
    if pairs.ndim != 2 or pairs.shape[1] != 2 or len(pairs) != len(units) or len(units) == 0:
        raise ValueError(f"pairs must be (NS, 2) and units (NS,), NS >= 1; got {pairs.shape} and {units.shape}")
    ns = len(units)
    return (ns, int(units.max()) + 1, (ctypes.c_int * (2 * ns))(*[int(j) for j in pairs.ravel()]),
            (ctypes.c_int * ns)(*[int(u) for u in units]))


def label_swap_plan(T: int, J: int, nv: int, n_pairs: int, n_units: int) -> int:
    """The workspace bytes that serve label_swap_costs and label_swap_solve for (T, J, nv, NS, U)
    (mvp_label_swap_plan, which refuses what the calls refuse of these)."""
    nbytes = ctypes.c_int64(0)
    call("mvp_label_swap_plan", int(T), int(J), int(nv), int(n_pairs), int(n_units), ctypes.byref(nbytes))
    return nbytes.value


def label_swap_solve_plan(T: int, n_units: int, nv: int) -> int:
    """The workspace bytes of label_swap_solve alone for (T, U, nv) (mvp_label_swap_solve_plan, which
    refuses what the call refuses of these)."""
    nbytes = ctypes.c_int64(0)
    call("mvp_label_swap_solve_plan", int(T), int(n_units), int(nv), ctypes.byref(nbytes))
    return nbytes.value


def label_swap_costs(kpts: torch.Tensor, cams: torch.Tensor, cam_idx: Sequence[int], pairs, units, *,
                     min_conf: float = 0.0, trunc_px: float = 20.0, motion_trunc_px: float = 40.0,
                     motion_weight: float = 1.0, swap_prior_px: float = 2.0, return_n: bool = False):
    """The cost tables of the left/right label-swap decision (mvp_label_swap_costs; the model is
    stated in include/mvpose.h; no reference counterpart).

    kpts (T, J, 3, V) float32 and cams (n_cams, 40) float64 on the GPU, cam_idx as for
    epipolar_lag_cost; pairs (NS, 2): the (left, right) joint of every symmetric pair; units (NS,):
    the unit each pair is exchanged with.  Returns (same, cross (T, U, NP) float64, keep, change,
    prior (T, U, NV) float64) and, with return_n, the complete-pair counts n (T, U, NV) int32 as a
    sixth.  The workspace is a torch.empty on the call's stream, sized by label_swap_plan."""
    V, lead, _, ci = _tri_args(kpts, cams, cam_idx)
    if len(lead) != 2:
        raise ValueError(f"kpts must be (T, J, 3, V), got {tuple(kpts.shape)}")
    T, J = int(lead[0]), int(lead[1])
    nv = len(ci)
    ns, U, cp, cu = _swap_lists(pairs, units)
    nbytes = label_swap_plan(T, J, nv, ns, U)
    dev = kpts.device
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    n_vp = nv * (nv - 1) // 2
    same, cross = (torch.empty((T, U, n_vp), dtype=torch.float64, device=dev) for _ in range(2))
    keep, change, prior = (torch.empty((T, U, nv), dtype=torch.float64, device=dev) for _ in range(3))
    n = torch.empty((T, U, nv), dtype=torch.int32, device=dev) if return_n else None
    call("mvp_label_swap_costs", ptr(kpts), T, J, V, ptr(cams), cams.shape[0], ci, nv, cp, ns, cu, U, float(min_conf),
         float(trunc_px), float(motion_trunc_px), float(motion_weight), float(swap_prior_px), ptr(work), int(nbytes),
         ptr(same), ptr(cross), ptr(keep), ptr(change), ptr(prior), ptr(n), stream(dev))
    return (same, cross, keep, change, prior, n) if return_n else (same, cross, keep, change, prior)


def label_swap_solve(same: torch.Tensor, cross: torch.Tensor, keep: torch.Tensor, change: torch.Tensor,
                     prior: torch.Tensor):
    """The label-swap recursion and backtrack on given tables (mvp_label_swap_solve; include/mvpose.h):
    same, cross (T, U, NP) and keep, change, prior (T, U, NV) float64 on the GPU, NP = NV·(NV−1)/2.
    Returns (swap (T, U) uint8: bit a set where view a's labels of the unit are exchanged, cost (U,)
    float64: the minimum of the objective).  The solver only adds and compares: the same tables
    give the same answer as any implementation that adds in the stated order."""
    for name, t in (("same", same), ("cross", cross), ("keep", keep), ("change", change), ("prior", prior)):
        _require(t, torch.float64, name)
        if t.dim() != 3:
            raise ValueError(f"{name} must be (T, U, n), got {tuple(t.shape)}")
    T, U, nv = (int(d) for d in keep.shape)
    n_vp = nv * (nv - 1) // 2
    if not (same.shape == cross.shape == (T, U, n_vp) and change.shape == prior.shape == (T, U, nv)):
        raise ValueError(f"tables disagree: same {tuple(same.shape)}, cross {tuple(cross.shape)}, keep "
                         f"{tuple(keep.shape)}, change {tuple(change.shape)}, prior {tuple(prior.shape)}")
    dev = keep.device
    nbytes = label_swap_solve_plan(T, U, nv)
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    swap = torch.empty((T, U), dtype=torch.uint8, device=dev)
    cost = torch.empty((U,), dtype=torch.float64, device=dev)
    call("mvp_label_swap_solve", ptr(same), ptr(cross), ptr(keep), ptr(change), ptr(prior), T, U, nv, ptr(work),
         int(nbytes), ptr(swap), ptr(cost), stream(dev))
    return swap, cost


def label_swap_apply(kpts: torch.Tensor, swap: torch.Tensor, cam_idx: Sequence[int], pairs, units, *, gauss=None):
    """kpts (T, J, 3, V) float32 with the labels exchanged where swap (T, U) uint8 says so
    (mvp_label_swap_apply): for every set bit a of swap[t, u], the (x, y, conf) records of the left
    and right joint of unit u's pairs change places in column cam_idx[a].  gauss (T, V, J, C) float64
    or None is treated the same way.  Returns (kpts_out, gauss_out or None), new tensors; applying
    the same mask to them restores the input's bits."""
    _require(kpts, torch.float32, "kpts")
    _require(swap, torch.uint8, "swap")
    if kpts.dim() != 4 or kpts.shape[2] != 3:
        raise ValueError(f"kpts must be (T, J, 3, V), got {tuple(kpts.shape)}")
    T, J, _, V = (int(d) for d in kpts.shape)
    ns, U, cp, cu = _swap_lists(pairs, units)
    if tuple(swap.shape) != (T, U):
        raise ValueError(f"swap must be (T, U) = {(T, U)}, got {tuple(swap.shape)}")
    C = 0
    if gauss is not None:
        _require(gauss, torch.float64, "gauss")
        if gauss.dim() != 4 or tuple(gauss.shape[:3]) != (T, V, J):
            raise ValueError(f"gauss must be (T, V, J, C) = {(T, V, J)} + (C,), got {tuple(gauss.shape)}")
        C = int(gauss.shape[3])
    ci = (ctypes.c_int * len(cam_idx))(*[int(c) for c in cam_idx])
    out = torch.empty_like(kpts)
    gout = torch.empty_like(gauss) if gauss is not None else None
    call("mvp_label_swap_apply", ptr(kpts), ptr(gauss), T, J, V, C, ci, len(ci), cp, ns, cu, U, ptr(swap), ptr(out),
         ptr(gout), stream(kpts.device))
    return out, gout


def fix_label_swaps(kpts: torch.Tensor, cams: torch.Tensor, cam_idx: Sequence[int], pairs, units, *, gauss=None,
                    min_conf: float = 0.0, trunc_px: float = 20.0, motion_trunc_px: float = 40.0,
                    motion_weight: float = 1.0, swap_prior_px: float = 2.0):
    """Find and undo the left/right label exchanges of every listed view: label_swap_costs,
    label_swap_solve, label_swap_apply on one stream, no synchronisation between them.  Returns
    (kpts_fixed, gauss_fixed or None, swap (T, U) uint8)."""
    tables = label_swap_costs(kpts, cams, cam_idx, pairs, units, min_conf=min_conf, trunc_px=trunc_px,
                              motion_trunc_px=motion_trunc_px, motion_weight=motion_weight,
                              swap_prior_px=swap_prior_px)
    swap, _ = label_swap_solve(*tables)
    fixed, gfixed = label_swap_apply(kpts, swap, cam_idx, pairs, units, gauss=gauss)
    return fixed, gfixed, swap


def track_people_plan(M: int, T: int, G: int, J: int, max_gap: int = 5) -> int:
    """The LDS bytes of track_people's workgroup for (M, T, G, J, max_gap) (mvp_track_people_plan,
    which refuses what the call refuses of these)."""
    lds = ctypes.c_int(0)
    call("mvp_track_people_plan", int(M), int(T), int(G), int(J), int(max_gap), ctypes.byref(lds))
    return lds.value


def track_people(xyz: torch.Tensor, *, max_gap: int = 5, max_jump: float = 50.0, gap_growth: float = 0.5,
                 min_joints: int = 1, return_links: bool = False):
    """Which group of a frame is the person of which group of an earlier frame
    (mvp_track_people; the rules are stated in include/mvpose.h; no reference counterpart).

    xyz (T, G, J, 3) or (M, T, G, J, 3) float32 on the GPU: per frame G triangulated skeletons in
    no particular order, NaN joints allowed, a group with no finite joint is absent; the M
    sequences are independent.  A group of frame t is linked to the open track whose latest
    observation, at most max_gap + 1 frames back, is nearest by the mean joint distance over the
    joints finite in both (at least min_joints of them), greedily in ascending (distance, lag,
    earlier group, group) while the distance is <= max_jump·(1 + gap_growth·(lag − 1)); a group
    left over starts a track.  Returns (track (..., T, G) int32, −1 = absent; n_tracks (...) int32
    on the device; link_cost (..., T, G) float64 and link_lag (..., T, G) uint8 with
    return_links, else None, None: the distance and the lag of the link a group was taken by, NaN
    and 0 for a new track or an absent group).  One stream-ordered launch, no workspace."""
    _require(xyz, torch.float32, "xyz")
    if xyz.dim() not in (4, 5) or xyz.shape[-1] != 3:
        raise ValueError(f"xyz must be (T, G, J, 3) or (M, T, G, J, 3), got {tuple(xyz.shape)}")
    lead = tuple(int(d) for d in xyz.shape[:-2])
    M, T, G = (1,) + lead if len(lead) == 2 else lead
    J = int(xyz.shape[-2])
    track_people_plan(M, T, G, J, max_gap)
    dev = xyz.device
    track = torch.empty(lead, dtype=torch.int32, device=dev)
    n_tracks = torch.empty(lead[:-2], dtype=torch.int32, device=dev)
    cost = torch.empty(lead, dtype=torch.float64, device=dev) if return_links else None
    lag = torch.empty(lead, dtype=torch.uint8, device=dev) if return_links else None
    call("mvp_track_people", ptr(xyz), M, T, G, J, int(max_gap), float(max_jump), float(gap_growth), int(min_joints),
         ptr(track), ptr(n_tracks), ptr(cost) if return_links else None, ptr(lag) if return_links else None,
         stream(dev))
    return track, n_tracks, cost, lag


BA_INFO_FIELDS = ("cost_seed", "cost", "trials", "accepted", "status", "lambda", "active_points", "used_views")
BA_STATUS = {0: "converged", 1: "out of trials", 2: "stalled", 3: "free view observed by fewer than 3 points"}


def _free_mask(free: Sequence[int]) -> int:
    """View positions (indices into cam_idx) -> the C-ABI's bit mask.  A position that has no bit
    sets bit 31, which the library refuses by name."""
    m = 0
    for i in free:
        i = int(i)
        m |= (1 << i) if 0 <= i < 31 else (1 << 31)
    return m


def bundle_adjust_plan(n_points: int, nv: int, free: Sequence[int]) -> int:
    """Workspace bytes of bundle_adjust / bundle_adjust_system (mvp_bundle_adjust_plan, which
    refuses what the calls refuse).  free: positions in cam_idx of the views to optimise."""
    nbytes = ctypes.c_int64(0)
    call("mvp_bundle_adjust_plan", int(n_points), int(nv), _free_mask(free), ctypes.byref(nbytes))
    return nbytes.value


def bundle_adjust_system(kpts: torch.Tensor, cams: torch.Tensor, cam_idx: Sequence[int], free: Sequence[int],
                         xyz: torch.Tensor, *, lam: float = 0.0, weights: str = "unit",
                         gauss: torch.Tensor | None = None, mask: torch.Tensor | None = None, min_conf: float = 0.0,
                         cov_floor: float = 1.0, huber_delta: float = 0.0, trans_prior_sigma: float = 0.0):
    """One linearisation of the bundle adjustment (mvp_bundle_adjust_system; stated in
    include/mvpose.h): the reduced camera system at the given cameras, f32 points and damping.

    kpts, cams, cam_idx, weights, gauss, mask, min_conf, cov_floor as for triangulate_refine; free:
    positions in cam_idx of the views whose R, T are unknowns (F of them, at least one view stays
    fixed).  Returns (S (6F, 6F) float64, b (6F,) float64, cost () float64, counts (2,) int64:
    active points and their used views), all on the GPU."""
    lead, n, nv, args, _bits = _obs_args(kpts, cams, cam_idx, xyz, weights, gauss, mask, min_conf, cov_floor, free=free)
    nbytes = bundle_adjust_plan(n, nv, free)
    dev = kpts.device
    n6 = 6 * bin(_free_mask(free)).count("1")
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    S = torch.empty((n6, n6), dtype=torch.float64, device=dev)
    b = torch.empty((n6,), dtype=torch.float64, device=dev)
    cost = torch.empty((), dtype=torch.float64, device=dev)
    counts = torch.empty((2,), dtype=torch.int64, device=dev)
    call("mvp_bundle_adjust_system", *args, float(huber_delta), float(trans_prior_sigma), float(lam), ptr(work), nbytes,
         ptr(S), ptr(b), ptr(cost), ptr(counts), stream(dev))
    return S, b, cost, counts


def bundle_adjust(kpts: torch.Tensor, cams: torch.Tensor, cam_idx: Sequence[int], free: Sequence[int],
                  xyz0: torch.Tensor, *, weights: str = "unit", gauss: torch.Tensor | None = None,
                  mask: torch.Tensor | None = None, min_conf: float = 0.0, cov_floor: float = 1.0,
                  huber_delta: float = 0.0, trans_prior_sigma: float = 0.0, max_iter: int = 30, tol: float = 1e-6):
    """Bundle adjustment of the free views' R, T and the 3D points over the 2D keypoints
    (mvp_bundle_adjust; the problem and the solver are stated in include/mvpose.h).

    Arguments as for bundle_adjust_system, xyz0 (..., 3) float32 being the seed.  Levenberg-Marquardt,
    at most max_iter trials, converged at an accepted cost decrease <= tol·cost; with a single fixed
    view trans_prior_sigma > 0 (world units) is what pins the scale.  Stream-ordered, no host
    synchronisation.  Returns (cams (n_cams, 40) float64: the input with the free views' R, T and P
    replaced; xyz (..., 3) float32; point_status (...) uint8: 0x80 for a point that took no part
    and is returned as its seed; cam_cov (6F, 6F) float64 over (dw, du) per free view in ascending
    position; info (8,) float64: BA_INFO_FIELDS), all on the GPU."""
    lead, n, nv, args, _bits = _obs_args(kpts, cams, cam_idx, xyz0, weights, gauss, mask, min_conf, cov_floor,
                                         free=free)
    nbytes = bundle_adjust_plan(n, nv, free)
    dev = kpts.device
    n6 = 6 * bin(_free_mask(free)).count("1")
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out_cams = torch.empty_like(cams)
    out = torch.empty(lead + (3,), dtype=torch.float32, device=dev)
    status = torch.empty(lead, dtype=torch.uint8, device=dev)
    cov = torch.empty((n6, n6), dtype=torch.float64, device=dev)
    info = torch.empty((8,), dtype=torch.float64, device=dev)
    call("mvp_bundle_adjust", *args, float(huber_delta), float(trans_prior_sigma), int(max_iter), float(tol), ptr(work),
         nbytes, ptr(out_cams), ptr(out), ptr(status), ptr(cov), ptr(info), stream(dev))
    return out_cams, out, status, cov, info


def trajectory_fit_plan(T: int, P: int, chunk: int = 0):
    """What trajectory_fit will use for (T, P, chunk) (mvp_trajectory_fit_plan): the chunk length
    of its time-parallel solve, the chunks per chain and the workspace bytes."""
    return _plan3("mvp_trajectory_fit_plan", T, P, chunk)


def _fit_args(kpts, cams, cam_idx, xyz, weights, gauss, mask, min_conf, cov_floor, huber_delta):
    """Shared front of the trajectory-fit and skeleton-fit calls: (T, P, the C call's leading
    arguments kpts_dev .. huber_delta, the packed mask to hold until the call is made)."""
    (T, P), _, _, args, bits = _obs_args(kpts, cams, cam_idx, xyz, weights, gauss, mask, min_conf, cov_floor,
                                         frames=True)
    return int(T), int(P), args + (float(huber_delta),), bits


def trajectory_fit_system(kpts: torch.Tensor, cams: torch.Tensor, cam_idx: Sequence[int], xyz: torch.Tensor, *,
                          weights: str = "conf", gauss: torch.Tensor | None = None,
                          mask: torch.Tensor | None = None, min_conf: float = 0.0, cov_floor: float = 1.0,
                          huber_delta: float = 0.0):
    """One linearisation of the trajectory fit's data term (mvp_trajectory_fit_system; stated in
    include/mvpose.h) at the float32 trajectory xyz (T, P, 3).

    kpts (T, P, 3, V), cams, cam_idx, weights, gauss (T, V, P, 6), mask (T, P, NV) bool, min_conf,
    cov_floor as for triangulate_refine; huber_delta as for bundle_adjust.  Returns (H (T, P, 6)
    float64: Σ Jᵀ W̃ J per frame as (xx, xy, xz, yy, yz, zz); g (T, P, 3) float64: Σ Jᵀ W̃ r;
    nviews (T, P) uint8: used views; cost (P, 2) float64: Σ rho and ½ Σ |second difference|² per
    chain), all on the GPU."""
    T, P, args, _bits = _fit_args(kpts, cams, cam_idx, xyz, weights, gauss, mask, min_conf, cov_floor, huber_delta)
    dev = kpts.device
    H = torch.empty((T, P, 6), dtype=torch.float64, device=dev)
    g = torch.empty((T, P, 3), dtype=torch.float64, device=dev)
    nviews = torch.empty((T, P), dtype=torch.uint8, device=dev)
    cost = torch.empty((P, 2), dtype=torch.float64, device=dev)
    call("mvp_trajectory_fit_system", *args, ptr(H), ptr(g), ptr(nviews), ptr(cost), stream(dev))
    return H, g, nviews, cost


def trajectory_fit(kpts: torch.Tensor, cams: torch.Tensor, cam_idx: Sequence[int], xyz0: torch.Tensor, *,
                   weights: str = "conf", gauss: torch.Tensor | None = None, mask: torch.Tensor | None = None,
                   min_conf: float = 0.0, cov_floor: float = 1.0, huber_delta: float = 0.0,
                   lambda_smooth: float = 1.0, max_iter: int = 30, tol: float = 1e-6, chunk: int = 0):
    """Trajectories fitted to the 2D keypoints (mvp_trajectory_fit; the problem and the solver are
    stated in include/mvpose.h): per chain p the minimiser of the used views' reprojection cost plus
    ½ lambda_smooth Σ |X_t − 2 X_{t−1} + X_{t−2}|², by Levenberg-Marquardt from the seed xyz0
    (T, P, 3) float32.  A frame seen by one view still pins two of its three coordinates; a frame
    seen by none is carried by the prior.  Arguments as for trajectory_fit_system; at most
    max_iter trials (0..63), converged at an accepted cost decrease <= tol·cost; chunk as for
    trajectory_smooth.  Stream-ordered, no host synchronisation.

    Returns (xyz (T, P, 3) float32; resid (T, P) float32: Σ over the used views of the whitened
    squared residual at the result, NaN without a used view; nviews (T, P) uint8; cost (P, 2)
    float64: the cost at the seed and at the result; status (P,) uint8: bits 0-5 the trials, 0x40
    not converged, 0x80 invalid chain (returned as its seed; NaN resid and cost)), all on the GPU."""
    T, P, args, _bits = _fit_args(kpts, cams, cam_idx, xyz0, weights, gauss, mask, min_conf, cov_floor, huber_delta)
    _, _, nbytes = trajectory_fit_plan(T, P, chunk)
    dev = kpts.device
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty((T, P, 3), dtype=torch.float32, device=dev)
    resid = torch.empty((T, P), dtype=torch.float32, device=dev)
    nviews = torch.empty((T, P), dtype=torch.uint8, device=dev)
    cost = torch.empty((P, 2), dtype=torch.float64, device=dev)
    status = torch.empty((P,), dtype=torch.uint8, device=dev)
    call("mvp_trajectory_fit", *args, float(lambda_smooth), int(max_iter), float(tol), int(chunk), ptr(work),
         int(nbytes), ptr(out), ptr(resid), ptr(nviews), ptr(cost), ptr(status), stream(dev))
    return out, resid, nviews, cost, status


def trajectory_fit_cov_plan(T: int, P: int, chunk: int = 0):
    """What trajectory_fit_cov will use for (T, P, chunk) (mvp_trajectory_fit_cov_plan): the chunk
    length, the chunks per chain and the workspace bytes."""
    return _plan3("mvp_trajectory_fit_cov_plan", T, P, chunk)


def trajectory_fit_cov(kpts: torch.Tensor, cams: torch.Tensor, cam_idx: Sequence[int], xyz: torch.Tensor, *,
                       weights: str = "conf", gauss: torch.Tensor | None = None, mask: torch.Tensor | None = None,
                       min_conf: float = 0.0, cov_floor: float = 1.0, huber_delta: float = 0.0,
                       lambda_smooth: float = 1.0, chunk: int = 0, want_cross: bool = True):
    """Covariance of a fitted trajectory (mvp_trajectory_fit_cov; stated in include/mvpose.h): the
    blocks of Σ = (blockdiag(H̃) + lambda_smooth·D₂ᵀD₂ ⊗ I₃)⁻¹, H̃ trajectory_fit's linearisation at
    xyz (T, P, 3) float32, normally trajectory_fit's output.  This is the Gauss-Newton / Laplace
    covariance at that state.  Arguments as for trajectory_fit.

    Returns (cov (T, P, 6) float32: (xx, xy, xz, yy, yz, zz) of Σ_{t,t}; cross (T, P, 3, 3) float32:
    Σ_{t,t+1}, row = coordinate of X_t, NaN at t = T−1, or None without want_cross; status (P,)
    uint8: 0, or 0x80 for an invalid chain, whose blocks are all NaN), in world units², all on the
    GPU.  Stream-ordered, no host synchronisation."""
    T, P, args, _bits = _fit_args(kpts, cams, cam_idx, xyz, weights, gauss, mask, min_conf, cov_floor, huber_delta)
    _, _, nbytes = trajectory_fit_cov_plan(T, P, chunk)
    dev = kpts.device
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty((T, P, 6), dtype=torch.float32, device=dev)
    cross = torch.empty((T, P, 3, 3), dtype=torch.float32, device=dev) if want_cross else None
    status = torch.empty((P,), dtype=torch.uint8, device=dev)
    call("mvp_trajectory_fit_cov", *args, float(lambda_smooth), int(chunk), ptr(work), int(nbytes), ptr(out),
         ptr(cross), ptr(status), stream(dev))
    return out, cross, status


def trajectory_fit_lag_plan(T: int, P: int, chunk: int = 0):
    """What trajectory_fit_lag will use for (T, P, chunk) (mvp_trajectory_fit_lag_plan): the chunk
    length, the chunks per chain and the workspace bytes."""
    return _plan3("mvp_trajectory_fit_lag_plan", T, P, chunk)


def _lag_args(args, frac, nv):
    """The fits' leading arguments with frac_host behind n_cam_idx: frac (nv,) fractional offsets,
    each in [0, 1) (the library checks the values)."""
    a = np.asarray(frac, dtype=np.float64).reshape(-1)
    if a.size != nv:
        raise ValueError(f"frac must hold one offset per listed view ({nv}), got {a.size}")
    return args[:8] + ((ctypes.c_double * nv)(*a.tolist()),) + args[8:]


def trajectory_fit_lag_system(kpts: torch.Tensor, cams: torch.Tensor, cam_idx: Sequence[int], frac,
                              xyz: torch.Tensor, *, weights: str = "conf", gauss: torch.Tensor | None = None,
                              mask: torch.Tensor | None = None, min_conf: float = 0.0, cov_floor: float = 1.0,
                              huber_delta: float = 0.0):
    """One linearisation of the trajectory fit with sub-frame camera offsets
    (mvp_trajectory_fit_lag_system; stated in include/mvpose.h) at the float32 trajectory xyz
    (T, P, 3): view i's frame t scores (1 − frac[i])·X_t + frac[i]·X_{t+1}.

    frac (NV,) host floats in [0, 1), one per entry of cam_idx; the other arguments as for
    trajectory_fit_system.  Returns (H (T, P, 6) float64: the nodes' blocks; C (T, P, 6) float64: the
    block between t and t+1, zero in the last row; g (T, P, 3) float64; nviews (T, P) uint8;
    cost (P, 2) float64; dlag (P, NV, 2) float64: the cost's first derivative with respect to
    frac[i] at fixed xyz and its Gauss-Newton curvature), all on the GPU."""
    T, P, args, _bits = _fit_args(kpts, cams, cam_idx, xyz, weights, gauss, mask, min_conf, cov_floor, huber_delta)
    nv = len(cam_idx)
    args = _lag_args(args, frac, nv)
    dev = kpts.device
    H = torch.empty((T, P, 6), dtype=torch.float64, device=dev)
    C = torch.empty((T, P, 6), dtype=torch.float64, device=dev)
    g = torch.empty((T, P, 3), dtype=torch.float64, device=dev)
    nviews = torch.empty((T, P), dtype=torch.uint8, device=dev)
    cost = torch.empty((P, 2), dtype=torch.float64, device=dev)
    dlag = torch.empty((P, nv, 2), dtype=torch.float64, device=dev)
    call("mvp_trajectory_fit_lag_system", *args, ptr(H), ptr(C), ptr(g), ptr(nviews), ptr(cost), ptr(dlag), stream(dev))
    return H, C, g, nviews, cost, dlag


def trajectory_fit_lag(kpts: torch.Tensor, cams: torch.Tensor, cam_idx: Sequence[int], frac, xyz0: torch.Tensor, *,
                       weights: str = "conf", gauss: torch.Tensor | None = None, mask: torch.Tensor | None = None,
                       min_conf: float = 0.0, cov_floor: float = 1.0, huber_delta: float = 0.0,
                       lambda_smooth: float = 1.0, max_iter: int = 30, tol: float = 1e-6, chunk: int = 0):
    """trajectory_fit for cameras that are a fraction of a frame apart (mvp_trajectory_fit_lag;
    stated in include/mvpose.h): frame t of view i was taken frac[i] of a frame after rig instant t
    and scores the chain's position interpolated between X_t and X_{t+1}; a view with frac > 0 is
    not used in the last frame.  frac (NV,) host floats in [0, 1); the recordings are aligned by
    the whole frames beforehand (sync.split_frame_offsets, sync.apply_frame_offsets).  The other
    arguments, the solver and the outputs as for trajectory_fit.  Stream-ordered, no host
    synchronisation.

    Returns (xyz, resid, nviews, cost, status as trajectory_fit's; dlag (P, NV, 2) float64: per
    chain and view the derivative of the minimised cost with respect to frac[i] and the
    Gauss-Newton curvature at fixed xyz, NaN for an invalid chain), all on the GPU."""
    T, P, args, _bits = _fit_args(kpts, cams, cam_idx, xyz0, weights, gauss, mask, min_conf, cov_floor, huber_delta)
    nv = len(cam_idx)
    args = _lag_args(args, frac, nv)
    _, _, nbytes = trajectory_fit_lag_plan(T, P, chunk)
    dev = kpts.device
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty((T, P, 3), dtype=torch.float32, device=dev)
    resid = torch.empty((T, P), dtype=torch.float32, device=dev)
    nviews = torch.empty((T, P), dtype=torch.uint8, device=dev)
    cost = torch.empty((P, 2), dtype=torch.float64, device=dev)
    status = torch.empty((P,), dtype=torch.uint8, device=dev)
    dlag = torch.empty((P, nv, 2), dtype=torch.float64, device=dev)
    call("mvp_trajectory_fit_lag", *args, float(lambda_smooth), int(max_iter), float(tol), int(chunk), ptr(work),
         int(nbytes), ptr(out), ptr(resid), ptr(nviews), ptr(cost), ptr(status), ptr(dlag), stream(dev))
    return out, resid, nviews, cost, status, dlag


def skeleton_fit_plan(T: int, P: int, J: int, chunk: int = 0):
    """What skeleton_fit will use for (T, P, J, chunk) (mvp_skeleton_fit_plan): the chunk length of
    its time-parallel solve, the chunks per chain and the workspace bytes."""
    return _plan3("mvp_skeleton_fit_plan", T, P, J, chunk)


def _skeleton_args(P, J, pairs, lengths, dev):
    """The segment arguments of the two skeleton-fit calls: the host pair table and the (G, n_seg)
    float32 lengths on the device."""
    J = int(J)
    if J < 1 or P % J:
        raise ValueError(f"P={P} must be a multiple of J={J} >= 1")
    G = P // J
    pr = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    n_seg = pr.shape[0]
    seg = (ctypes.c_int * max(2 * n_seg, 1))(*pr.reshape(-1).tolist())
    ln = torch.as_tensor(lengths, dtype=torch.float32, device=dev)
    if ln.dim() == 1:
        ln = ln.unsqueeze(0).expand(G, -1)
    if tuple(ln.shape) != (G, n_seg):
        raise ValueError(f"lengths must be {(n_seg,)} or {(G, n_seg)}, got {tuple(ln.shape)}")
    return J, G, seg, n_seg, ln.contiguous()


def skeleton_fit_system(kpts: torch.Tensor, cams: torch.Tensor, cam_idx: Sequence[int], xyz: torch.Tensor,
                        J: int, pairs, lengths, *, lambda_bone: float = 1.0, weights: str = "conf",
                        gauss: torch.Tensor | None = None, mask: torch.Tensor | None = None, min_conf: float = 0.0,
                        cov_floor: float = 1.0, huber_delta: float = 0.0):
    """One linearisation of the skeleton fit (mvp_skeleton_fit_system; stated in include/mvpose.h) at
    the float32 trajectory xyz (T, P, 3), P = G·J, chain g·J + j the joint j of person g.

    pairs (n_seg, 2) int: the joints a segment joins; lengths (n_seg,) or (G, n_seg) float32: a
    length that is not finite or not > 0 switches the segment off for that person.  The other
    arguments as for trajectory_fit_system.  Returns (H (T, P, 6) float64 and g (T, P, 3) float64:
    the data term plus the bone terms with lambda_bone applied; nviews (T, P) uint8; cost (G, 3)
    float64: Σ rho, ½ Σ |second difference|², ½ Σ (r − L)²), all on the GPU."""
    T, P, args, _bits = _fit_args(kpts, cams, cam_idx, xyz, weights, gauss, mask, min_conf, cov_floor, huber_delta)
    dev = kpts.device
    J, G, seg, n_seg, ln = _skeleton_args(P, J, pairs, lengths, dev)
    H = torch.empty((T, P, 6), dtype=torch.float64, device=dev)
    g = torch.empty((T, P, 3), dtype=torch.float64, device=dev)
    nviews = torch.empty((T, P), dtype=torch.uint8, device=dev)
    cost = torch.empty((G, 3), dtype=torch.float64, device=dev)
    call("mvp_skeleton_fit_system", *args, J, seg, n_seg, ptr(ln) if n_seg else None, float(lambda_bone), ptr(H),
         ptr(g), ptr(nviews), ptr(cost), stream(dev))
    return H, g, nviews, cost


def skeleton_fit(kpts: torch.Tensor, cams: torch.Tensor, cam_idx: Sequence[int], xyz0: torch.Tensor, J: int, pairs,
                 lengths, *, lambda_bone: float = 1.0, weights: str = "conf", gauss: torch.Tensor | None = None,
                 mask: torch.Tensor | None = None, min_conf: float = 0.0, cov_floor: float = 1.0,
                 huber_delta: float = 0.0, lambda_smooth: float = 1.0, max_iter: int = 30, tol: float = 1e-6,
                 chunk: int = 0):
    """The trajectory fit with each person's joints coupled by bone lengths (mvp_skeleton_fit; stated
    in include/mvpose.h): per person the minimiser of the chains' trajectory-fit costs plus
    ½ lambda_bone Σ_t Σ_segments (|X_b − X_a| − L)², by Levenberg-Marquardt from the seed xyz0
    (T, P, 3) float32, one damping factor and one accept / reject per person.  Arguments as for
    skeleton_fit_system and trajectory_fit.  Stream-ordered, no host synchronisation.

    Returns (xyz (T, P, 3) float32; resid (T, P) float32; nviews (T, P) uint8; bone (T, G, n_seg)
    float32: r − L at the result, NaN for a segment that is off; cost (G, 4) float64: the cost at the
    seed and at the result, the bone part of each; group_status (G,) uint8: bits 0-5 the trials, 0x40
    not converged, 0x80 invalid; chain_status (P,) uint8: 0x80 for a chain returned as its seed), all
    on the GPU."""
    T, P, args, _bits = _fit_args(kpts, cams, cam_idx, xyz0, weights, gauss, mask, min_conf, cov_floor, huber_delta)
    dev = kpts.device
    J, G, seg, n_seg, ln = _skeleton_args(P, J, pairs, lengths, dev)
    _, _, nbytes = skeleton_fit_plan(T, P, J, chunk)
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty((T, P, 3), dtype=torch.float32, device=dev)
    resid = torch.empty((T, P), dtype=torch.float32, device=dev)
    nviews = torch.empty((T, P), dtype=torch.uint8, device=dev)
    bone = torch.empty((T, G, n_seg), dtype=torch.float32, device=dev)
    cost = torch.empty((G, 4), dtype=torch.float64, device=dev)
    gstatus = torch.empty((G,), dtype=torch.uint8, device=dev)
    cstatus = torch.empty((P,), dtype=torch.uint8, device=dev)
    call("mvp_skeleton_fit", *args, float(lambda_smooth), J, seg, n_seg, ptr(ln) if n_seg else None,
         float(lambda_bone), int(max_iter), float(tol), int(chunk), ptr(work), int(nbytes), ptr(out), ptr(resid),
         ptr(nviews), ptr(bone), ptr(cost), ptr(gstatus), ptr(cstatus), stream(dev))
    return out, resid, nviews, bone, cost, gstatus, cstatus
