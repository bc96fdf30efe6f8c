"""Extrinsics repair from the keypoints already detected: bundle adjustment of the cameras that may
have moved since calibration (ops.bundle_adjust; the problem is stated in include/mvpose.h).

No reference counterpart: the reference's extrinsic branch (refine.py, mvp_sgd_refine_cams) is f32
Adam over trajectory windows with at most two learnable cameras and no uncertainty.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from . import synthetic as syn


def _reproj_rms(points, kpts, params, positions, inliers):
    """Root mean square reprojection error (raw, distorted pixels) of points (n, 3) against kpts
    (n, 3, V) over the views inliers (n, NV) marks, fp64 on the host."""
    se, cnt = 0.0, 0
    for i, pos in enumerate(positions):
        K, R, T, dist = params[pos]
        sel = inliers[:, i] & np.isfinite(points).all(1)
        if not sel.any():
            continue
        cam = {"K": np.asarray(K, dtype=np.float64), "R": np.asarray(R, dtype=np.float64),
               "T": np.asarray(T, dtype=np.float64).reshape(3, 1),
               "dist": np.resize(np.asarray(dist, dtype=np.float64).ravel(), 5)}
        uv = syn.project(points[sel].astype(np.float64), cam)
        d = uv - kpts[sel][:, :2, pos].astype(np.float64)
        se += float((d * d).sum())
        cnt += int(sel.sum())
    return float(np.sqrt(se / cnt)) if cnt else float("nan")


def refine_extrinsics(kpts_2d, camera_params, camera_indices=None, free=None, weights="conf", gauss=None,
                      inlier_px=25.0, min_conf=0.0, huber_px=0.0, trans_prior_sigma=0.0, max_iter=30, tol=1e-6):
    """Corrected R, T of the cameras that may have moved, from 2D keypoints.

    kpts_2d: (T, J, 3, V) keypoints (numpy or torch; get_pose_3D's layout), or process_people's
    (T, G, J, 3, V), whose groups are folded into frames (NaN-padded groups take no part).
    camera_params {key: [K, R, T, dist]}; camera_indices: the keys of the cameras to use (default
    all); free: the keys of the cameras whose R, T are optimised (default: every listed camera but
    the first).  K and the distortion are never touched.

    ops.triangulate_robust at inlier_px supplies the seeds and each point's inlier views; then
    ops.bundle_adjust with weights "unit" / "conf" / "heatmap" (gauss: the heatmap Gaussians,
    (T, V, J, 6) or (T, G, V, J, 6)), a Huber threshold huber_px on the whitened residual (pixels
    for "unit"; 0 = off) and at most max_iter Levenberg-Marquardt trials.

    With a single fixed camera the pixels do not fix the overall scale of (points, free
    translations): trans_prior_sigma (world units, the belief in how far a camera can have moved)
    pins it and must then be > 0.  With two or more fixed cameras their baseline sets the scale
    and it may stay 0.

    Returns (camera_params in the same {key: [K, R, T, dist]} structure, info): info holds the
    solver's record by name (ops.BA_INFO_FIELDS; "status_text"), "cam_cov" (6F, 6F) over (dw, du)
    of the free cameras in listed order with "free" naming them, "rms_before" / "rms_after" (the
    reprojection RMS in pixels over the inlier views, seeds with the input cameras against the
    adjusted points with the returned ones), "points" (T[, G], J, 3) float32 and "point_status"."""
    keys = list(camera_params.keys())
    listed = list(keys if camera_indices is None else camera_indices)
    positions = [keys.index(c) for c in listed]
    if free is None:
        free_keys = listed[1:]
    else:
        free_keys = list(free)
        for c in free_keys:
            if c not in listed:
                raise ValueError(f"free camera {c!r} is not among the listed cameras {listed}")
    free_pos = sorted(listed.index(c) for c in free_keys)
    if not free_pos:
        raise ValueError("no camera to optimise: free is empty")
    if len(listed) - len(set(free_pos)) < 1:
        raise ValueError("at least one listed camera must stay fixed")
    if len(listed) - len(set(free_pos)) == 1 and not trans_prior_sigma > 0:
        raise ValueError(
            "with a single fixed camera the keypoints do not determine the overall scale of the scene and of the "
            "free cameras' translations: give trans_prior_sigma > 0 (world units, how far a camera can have moved), "
            "or keep two cameras fixed through free=...")
    if isinstance(kpts_2d, torch.Tensor):
        dev = kpts_2d.device if kpts_2d.is_cuda else torch.device("cuda")
        kp = kpts_2d.to(device=dev, dtype=torch.float32)
    else:
        dev = torch.device("cuda")
        kp = torch.as_tensor(np.ascontiguousarray(np.asarray(kpts_2d, dtype=np.float32)), device=dev)
    if kp.dim() not in (4, 5) or kp.shape[-2] != 3:
        raise ValueError(f"kpts_2d must be (T, J, 3, V) or (T, G, J, 3, V), got {tuple(kp.shape)}")
    lead = tuple(kp.shape[:-2])
    J, V = int(kp.shape[-3]), int(kp.shape[-1])
    kp = kp.reshape(-1, J, 3, V).contiguous()
    g = None
    if weights == "heatmap":
        if gauss is None:
            raise ValueError('weights="heatmap" needs gauss, the heatmap Gaussians')
        g = torch.as_tensor(gauss, dtype=torch.float64, device=dev)
        g = g.reshape(-1, V, J, 6).contiguous()
    params = [camera_params[k] for k in keys]
    cams = torch.tensor(ops.pack_cameras(camera_params), device=dev)
    seed, inliers, _ = ops.triangulate_robust(kp, cams, positions, inlier_px=inlier_px, min_conf=min_conf,
                                              return_err=False)
    out_cams, xyz, pstat, cov, info = ops.bundle_adjust(
        kp, cams, positions, free_pos, seed, weights=weights, gauss=g, mask=inliers, min_conf=min_conf,
        huber_delta=huber_px, trans_prior_sigma=trans_prior_sigma, max_iter=max_iter, tol=tol)
    rec = out_cams.cpu().numpy()
    new_params = {}
    for i, k in enumerate(keys):
        K, R, T, dist = camera_params[k]
        if listed.count(k) and listed.index(k) in free_pos:
            R = rec[i, 14:23].reshape(3, 3).copy()
            T = rec[i, 23:26].reshape(np.asarray(T).shape).copy()
        new_params[k] = [K, R, T, dist]
    iv = info.cpu().numpy()
    res = {name: (float(v) if name in ("cost_seed", "cost", "lambda") else int(v))
           for name, v in zip(ops.BA_INFO_FIELDS, iv)}
    res["status_text"] = ops.BA_STATUS.get(res["status"], "?")
    res["cam_cov"] = cov.cpu().numpy()
    res["free"] = [listed[i] for i in free_pos]
    ps = pstat.cpu().numpy().reshape(-1)
    act = ps == 0
    kp_h = kp.reshape(-1, 3, V).cpu().numpy()
    inl = inliers.reshape(-1, len(positions)).cpu().numpy() & act[:, None]
    new_list = [new_params[k] for k in keys]
    res["rms_before"] = _reproj_rms(seed.reshape(-1, 3).cpu().numpy(), kp_h, params, positions, inl)
    res["rms_after"] = _reproj_rms(xyz.reshape(-1, 3).cpu().numpy(), kp_h, new_list, positions, inl)
    res["points"] = xyz.reshape(lead + (3,)).cpu().numpy()
    res["point_status"] = ps.reshape(lead)
    return new_params, res
