"""Pose-based frame synchronisation of the cameras (no reference counterpart: the reference's
synchronize_videos.py asks an operator for a frame number per camera).

Convention: frame ``t`` of camera ``v`` was taken at rig instant ``t + s_v``, with ``s_0 = 0``.
Pair ``(a, b)`` at lag ``l`` matches a-frame ``t`` with b-frame ``t + l``; both show the same
instant when ``l = s_a - s_b``.

* ``estimate_frame_offsets``: the epipolar lag-cost scan on the GPU (ops.epipolar_lag_cost, the
  problem is stated in include/mvpose.h), then ``offsets_from_curves``: per pair the lag of the
  lowest mean cost with a rejection rule, and a least-squares fit of ``s`` over the accepted pairs.
* ``apply_frame_offsets``: cuts every camera to the instants all cameras saw (pure indexing).
* ``split_frame_offsets``: ``s = n + a``, the whole frames to align by and the fractions that
  ``refine.fit_trajectory(frame_offsets=a)`` models.
* ``refine_frame_offsets``: refines ``s`` to a fraction of a frame from trajectory fits alone.

Synchronise, then fit: ``_, info = estimate_frame_offsets(kpts_2d, params)``; ``n, a =
split_frame_offsets(info["s"])``; ``(kpts,), _ = apply_frame_offsets([kpts_2d], n, [3])``; a seed
at those instants (e.g. triangulate and smooth the aligned keypoints); optionally ``s, _ =
refine_frame_offsets(kpts_2d, params, seed_at_camera_0_frames, info["s"])``; then
``refine.fit_trajectory(kpts, params, seed, frame_offsets=a)``.
"""
from __future__ import annotations

from collections import deque

import numpy as np

NO_OFFSET = np.iinfo(np.int64).min   # offsets_int of a camera whose offset could not be fixed (its s is NaN)


def offsets_from_curves(cost_sum, cost_cnt, pairs, n_views, n_terms, min_overlap=0.5, min_contrast=2.0):
    """The pair and global logic of estimate_frame_offsets on the scan's curves (numpy, host).

    cost_sum / cost_cnt (NP, 2L+1): the scan's sums and term counts, pairs the NP (a, b) view
    positions, n_terms = T·J.  Per pair: mean = sum / cnt over the lags with cnt >= min_overlap ·
    n_terms (the valid lags); lag = argmin of the mean (the first one on a tie); sub-frame lag =
    the vertex of the parabola through the three means around it (the integer lag when a
    neighbour is missing or the three are not strictly convex); contrast = median(mean) /
    min(mean) over the valid lags.  A pair is rejected, in this order of tests, for "overlap" (no
    valid lag), "contrast" (contrast < min_contrast) or "edge" (its minimum sits on the first or
    the last valid lag of the scan: the true lag may lie outside).  Global solve: least squares
    of s_a - s_b = sub-frame lag over the accepted pairs, unit weights, s_0 = 0, over the cameras
    connected to camera 0 through accepted pairs; the others get NaN (NO_OFFSET as integer).
    Returns (offsets_int (n_views,) int64 = round(s), info)."""
    cost_sum = np.asarray(cost_sum, np.float64)
    cost_cnt = np.asarray(cost_cnt, np.int64)
    n_pairs, n_lags = cost_sum.shape
    L = (n_lags - 1) // 2
    lag = np.zeros(n_pairs, np.int64)
    sub = np.full(n_pairs, np.nan)
    contrast = np.full(n_pairs, np.nan)
    accepted = np.zeros(n_pairs, bool)
    reason = []
    valid = cost_cnt >= max(min_overlap * n_terms, 1.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(valid, cost_sum / np.maximum(cost_cnt, 1), np.nan)
    for p in range(n_pairs):
        idx = np.flatnonzero(valid[p])
        if idx.size == 0:
            reason.append("overlap")
            continue
        m = mean[p, idx]
        k = int(idx[int(np.argmin(m))])
        lo = float(mean[p, k])
        lag[p] = k - L
        sub[p] = float(lag[p])
        contrast[p] = float(np.median(m)) / lo if lo > 0 else np.inf
        if 0 < k < n_lags - 1 and valid[p, k - 1] and valid[p, k + 1]:
            curv = mean[p, k - 1] - 2.0 * lo + mean[p, k + 1]
            if curv > 0:
                sub[p] = lag[p] + 0.5 * (mean[p, k - 1] - mean[p, k + 1]) / curv
        if not contrast[p] >= min_contrast:
            reason.append("contrast")
        elif k == idx[0] or k == idx[-1]:
            reason.append("edge")
        else:
            reason.append("")
            accepted[p] = True
    # cameras connected to camera 0 through accepted pairs
    adj = [[] for _ in range(n_views)]
    for p, (a, b) in enumerate(pairs):
        if accepted[p]:
            adj[a].append(b)
            adj[b].append(a)
    connected = np.zeros(n_views, bool)
    connected[0] = True
    queue = deque([0])
    while queue:
        u = queue.popleft()
        for w in adj[u]:
            if not connected[w]:
                connected[w] = True
                queue.append(w)
    s = np.full(n_views, np.nan)
    s[0] = 0.0
    unknown = [v for v in range(1, n_views) if connected[v]]
    col = {v: i for i, v in enumerate(unknown)}
    rows = [p for p, (a, b) in enumerate(pairs) if accepted[p] and connected[a]]
    if unknown:
        A = np.zeros((len(rows), len(unknown)))
        for r, p in enumerate(rows):
            a, b = pairs[p]
            if a in col:
                A[r, col[a]] = 1.0
            if b in col:
                A[r, col[b]] = -1.0
        s[unknown] = np.linalg.lstsq(A, sub[rows], rcond=None)[0]
    residual = np.full(n_pairs, np.nan)
    for p in rows:
        a, b = pairs[p]
        residual[p] = sub[p] - (s[a] - s[b])
    offsets = np.full(n_views, NO_OFFSET, np.int64)
    offsets[connected] = np.round(s[connected]).astype(np.int64)
    info = {"s": s, "pairs": [tuple(int(c) for c in pr) for pr in pairs], "lag": lag, "lag_subframe": sub,
            "contrast": contrast, "accepted": accepted, "reason": reason, "residual": residual,
            "cost_sum": cost_sum, "cost_cnt": cost_cnt, "cost_mean": mean, "max_lag": L}
    return offsets, info


def _lag_cost(kpts_2d, camera_params, positions, max_lag, min_conf, trunc_px, device=None):
    """ops.epipolar_lag_cost on host arrays -> (sum, cnt, pairs) as numpy."""
    import torch
    from . import ops
    dev = torch.device(device if device is not None else "cuda")
    kp = torch.as_tensor(np.ascontiguousarray(np.asarray(kpts_2d, dtype=np.float32)), device=dev)
    cams = torch.tensor(ops.pack_cameras(camera_params), device=dev)
    cost_sum, cost_cnt, pairs = ops.epipolar_lag_cost(kp, cams, positions, max_lag, min_conf=min_conf,
                                                      trunc_px=trunc_px)
    return cost_sum.cpu().numpy(), cost_cnt.cpu().numpy(), pairs


def estimate_frame_offsets(kpts_2d, camera_params, camera_indices=None, max_lag=60, min_conf=0.0, trunc_px=20.0,
                           min_overlap=0.5, min_contrast=2.0, device=None):
    """Frame offsets of the listed cameras from their 2D keypoints and the calibration.

    kpts_2d (T, J, 3, V) (the reference layout), camera_params {key: [K, R, T, dist]} as for
    get_pose_3D, camera_indices the keys of the cameras to synchronise (default: all): view i of
    the result is camera camera_indices[i], read from the column of kpts_2d at that key's
    position in camera_params.  Lags of
    -max_lag..max_lag frames are scanned (max_lag < T); keypoints below min_conf are ignored; a
    pair's Sampson distances are truncated at trunc_px undistorted pixels.  The per-pair and
    global rules are offsets_from_curves'.  Returns (offsets_int (NV,) int64, info): camera v's
    frame t was taken at rig instant t + offsets_int[v], offsets_int[0] = 0; a camera that no
    chain of accepted pairs connects to the first one has NO_OFFSET (info["s"] NaN).  info: "s"
    (fractional offsets), "pairs", "lag", "lag_subframe", "contrast", "accepted", "reason" (""
    or why the pair was rejected), "residual" (sub-frame lag minus the fit's, accepted pairs),
    "cost_sum", "cost_cnt", "cost_mean" (NP, 2·max_lag+1) and "max_lag"."""
    keys = list(camera_params.keys())
    if camera_indices is None:
        camera_indices = keys
    positions = [keys.index(c) for c in camera_indices]
    shape = np.shape(kpts_2d)
    if len(shape) != 4 or shape[2] != 3:
        raise ValueError(f"kpts_2d must be (T, J, 3, V), got {shape}")
    cost_sum, cost_cnt, pairs = _lag_cost(kpts_2d, camera_params, positions, max_lag, min_conf, trunc_px, device)
    return offsets_from_curves(cost_sum, cost_cnt, pairs, len(positions), shape[0] * shape[1],
                               min_overlap=min_overlap, min_contrast=min_contrast)


def apply_frame_offsets(arrays, offsets_int, view_axes):
    """Cuts every camera to the common instants tau in [max s, T + min s): camera v contributes
    its frames tau - s_v.

    arrays: arrays with time on axis 0 and the cameras on axis view_axes[i] (kpts_2d (T, J, 3, V):
    3; heatmaps_2d (T, V, J, 6): 1); a None entry stays None.  Returns (aligned arrays, each of
    T - (max s - min s) frames, first (V,) int64: the index of each camera's first kept frame).
    Pure indexing: the fractions of a frame that remain (split_frame_offsets) are not resampled
    away but modelled by refine.fit_trajectory(frame_offsets=a)."""
    s = np.asarray(offsets_int, np.int64)
    if s.ndim != 1 or (s == NO_OFFSET).any():
        raise ValueError(f"offsets_int must be (V,) with every camera's offset known, got {s}")
    first = s.max() - s
    out = []
    for arr, axis in zip(arrays, view_axes):
        if arr is None:
            out.append(None)
            continue
        arr = np.asarray(arr)
        if arr.shape[axis] != s.size:
            raise ValueError(f"axis {axis} of an array of shape {arr.shape} does not hold {s.size} cameras")
        n = arr.shape[0] - int(s.max() - s.min())
        if n < 1:
            raise ValueError(f"offsets {s.tolist()} leave no common frame of {arr.shape[0]}")
        res = np.empty((n,) + arr.shape[1:], arr.dtype)
        for v in range(s.size):
            sel = [slice(None)] * arr.ndim
            sel[axis] = v
            src = list(sel)
            src[0] = slice(int(first[v]), int(first[v]) + n)
            res[tuple(sel)] = arr[tuple(src)]
        out.append(res)
    return out, first


def split_frame_offsets(s):
    """s (V,) fractional offsets (estimate_frame_offsets' info["s"]; s[0] = 0 is the gauge) ->
    (n (V,) int64 = floor(s), a (V,) float64 = s - n in [0, 1)): align the recordings by n
    (apply_frame_offsets), hand a to refine.fit_trajectory(frame_offsets=a)."""
    s = np.asarray(s, np.float64)
    if s.ndim != 1 or not np.isfinite(s).all():
        raise ValueError(f"s must be (V,) with every camera's offset known, got {s}")
    n = np.floor(s)
    a = s - n
    up = a >= 1.0                      # s a hair below an integer: s - floor(s) rounds to 1
    n, a = np.where(up, n + 1, n), np.where(up, 0.0, a)
    return n.astype(np.int64), a


def refine_frame_offsets(kpts_2d, camera_params, seed, s0, rounds=4, h=0.02, stop=0.01, device=None, **fit_kw):
    """Refines the cameras' frame offsets to a fraction of a frame from trajectory fits alone.

    kpts_2d (T, J, 3, V) as recorded (not aligned), one column per camera of camera_params, in
    sorted key order, which is refine.fit_trajectory's default view list; seed (T, J, 3): the
    trajectory at camera 0's frames, which are the rig instants (s[0] = 0 is the gauge and stays);
    s0 (V,) the offsets to start from, e.g. estimate_frame_offsets' info["s"], one per camera in the
    same order.  Always all cameras: the whole frames are applied to kpts_2d's columns by position
    and the fractions go to the fit's views by position, so a subset or another order would send
    them to different cameras.  fit_kw goes to refine.fit_trajectory (weights, lambda_smooth,
    huber_px, ...; not camera_indices).

    Per round: split s (split_frame_offsets), align by the whole frames (apply_frame_offsets; a
    fraction that crossed 0 or 1 is thereby re-split and re-aligned), fit with the fractions, and
    sum info["dlag"][..., 0] over the valid joints on the host in ascending order: at a fitted
    state that is the derivative of the minimised cost with respect to each offset.  A Newton step
    on it follows, its Jacobian from central differences of that sum between 2·(V−1) further
    fits at s_j ± h; the curvature the fit reports at fixed trajectory (dlag[..., 1]) overestimates
    the reduced curvature badly and is not used.  A step is limited to half a frame.  At most
    `rounds` rounds; stops on a step below `stop` frames.  Returns (s (V,) float64, info): "cost"
    every round's summed cost and the final one, "step" every round's largest step, "fits" the
    number of fits made."""
    from . import refine
    if "camera_indices" in fit_kw:
        raise ValueError("refine_frame_offsets uses every camera of camera_params in sorted order; camera_indices is not taken")
    kp = np.asarray(kpts_2d)
    sd = np.asarray(seed)
    s = np.array(s0, np.float64)
    nv = len(camera_params)
    if s.shape != (nv,):
        raise ValueError(f"s0 must hold one offset per camera ({nv}), got shape {s.shape}")
    if kp.ndim != 4 or kp.shape[-1] != nv:
        raise ValueError(f"kpts_2d must be (T, J, 3, {nv}), one column per camera, got {kp.shape}")
    fits = [0]

    def reduced(sv):
        n, a = split_frame_offsets(sv)
        (k,), _ = apply_frame_offsets([kp], n, [3])
        lo = int(n.max())
        _, info = refine.fit_trajectory(np.ascontiguousarray(k), camera_params, sd[lo:lo + k.shape[0]],
                                        frame_offsets=a, return_info=True, device=device,
                                        **fit_kw)
        fits[0] += 1
        ok = np.flatnonzero(info["status"].reshape(-1) != 0x80)
        dl = info["dlag"].reshape(-1, nv, 2)
        ga = np.zeros(nv)
        for p in ok:
            ga = ga + dl[p, :, 0]
        return ga, float(info["cost"].reshape(-1, 2)[ok, 1].sum())
    costs, steps = [], []
    for _ in range(int(rounds)):
        g0, f0 = reduced(s)
        costs.append(f0)
        jac = np.zeros((nv - 1, nv - 1))
        for j in range(1, nv):
            sp, sm = s.copy(), s.copy()
            sp[j] += h
            sm[j] -= h
            jac[:, j - 1] = (reduced(sp)[0][1:] - reduced(sm)[0][1:]) / (2 * h)
        step = np.clip(-np.linalg.solve(jac, g0[1:]), -0.5, 0.5)
        s[1:] += step
        steps.append(float(np.abs(step).max()))
        if steps[-1] < stop:
            break
    costs.append(reduced(s)[1])
    return s, {"cost": costs, "step": steps, "fits": fits[0]}
