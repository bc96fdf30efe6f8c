"""Several people per camera: what sits between ops.associate_views and the per-person stages
(no reference counterpart; the reference handles one person per camera).

* ``gather_groups``: the per-slot keypoints (and heatmap Gaussians) re-ordered by the group
  numbers of ops.associate_views into the single-person layout every later stage takes, one
  kpts_2d per group.  Torch indexing on the tensors' own device, no host synchronisation.
* ``link_tracks``: frame-to-frame identity of the triangulated groups, so that
  ops.trajectory_smooth can run per person.
* ``track_people``: the same identity on the device and through dropouts (ops.track_people).
* ``person_trajectories``: the per-frame groups re-ordered by track number into one trajectory per
  person, the layout refine.smooth_trajectory takes.
"""
from __future__ import annotations

from typing import Sequence

import numpy as np
import torch


def gather_groups(kpts: torch.Tensor, group: torch.Tensor, cam_idx: Sequence[int], max_groups: int,
                  gauss: torch.Tensor | None = None):
    """kpts (T, P, J, 3, V) per-slot keypoints, group (T, NV, P) int8 from ops.associate_views over
    cam_idx -> (kpts_g (T, G, J, 3, V), gauss_g or None, dropped (T,) int64), G = max_groups.

    kpts_g[t, g, :, :, cam_idx[i]] is the skeleton of the slot p with group[t, i, p] == g and NaN
    where group g has no member in that view; columns that cam_idx does not list are NaN.  gauss
    (T, V, P, J, 6), the per-slot heatmap Gaussians, is gathered the same way into
    (T, G, V, J, 6).  dropped[t] counts the groups of frame t numbered max_groups and above, which
    are not returned (the groups are ordered by the number of views that see them, so the ones
    dropped are the least supported)."""
    if kpts.dim() != 5 or kpts.shape[3] != 3:
        raise ValueError(f"kpts must be (T, P, J, 3, V), got {tuple(kpts.shape)}")
    T, P, J, _, V = kpts.shape
    nv = len(cam_idx)
    if tuple(group.shape) != (T, nv, P):
        raise ValueError(f"group must be {(T, nv, P)}, got {tuple(group.shape)}")
    G = int(max_groups)
    if G < 1:
        raise ValueError(f"max_groups={max_groups} < 1")
    if gauss is not None and tuple(gauss.shape) != (T, V, P, J, 6):
        raise ValueError(f"gauss must be {(T, V, P, J, 6)}, got {tuple(gauss.shape)}")
    g = group.to(torch.int64)
    # row G collects what is not returned: unusable nodes and the groups beyond max_groups
    row = torch.where((g >= 0) & (g < G), g, torch.full_like(g, G))
    out = torch.full((T, G, J, 3, V), float("nan"), dtype=kpts.dtype, device=kpts.device)
    out_g = None
    if gauss is not None:
        out_g = torch.full((T, G, V, J, 6), float("nan"), dtype=gauss.dtype, device=gauss.device)
    for i, c in enumerate(cam_idx):
        c = int(c)
        buf = torch.full((T, G + 1, J, 3), float("nan"), dtype=kpts.dtype, device=kpts.device)
        buf.scatter_(1, row[:, i, :, None, None].expand(T, P, J, 3), kpts[..., c])
        out[..., c] = buf[:, :G]
        if gauss is not None:
            bg = torch.full((T, G + 1, J, 6), float("nan"), dtype=gauss.dtype, device=gauss.device)
            bg.scatter_(1, row[:, i, :, None, None].expand(T, P, J, 6), gauss[:, c])
            out_g[:, :, c] = bg[:, :G]
    n_groups = g.reshape(T, -1).amax(1) + 1
    return out, out_g, (n_groups - G).clamp_(min=0)


def link_tracks(xyz, max_jump: float = 50.0) -> np.ndarray:
    """xyz (T, G, J, 3) triangulated groups (NaN joints allowed; a group with no finite joint is
    absent) -> track (T, G) int32, -1 for an absent group.

    Greedy frame-to-frame linking on the host in numpy: the distance between a group of frame t
    and a track seen at frame t - 1 is the mean over the joints finite in both of the joint-to-joint
    distance; the pairs are taken in ascending order of distance while it is <= max_jump (world
    units), each track and each group at most once per frame; a group left over starts a new track,
    and a track not seen in a frame ends there.  Track numbers count up from 0 in order of first
    appearance.  Not a hot path: T·G² distances of J joints each, once per recording."""
    x = np.asarray(xyz.detach().cpu() if isinstance(xyz, torch.Tensor) else xyz, dtype=np.float64)
    if x.ndim != 4 or x.shape[3] != 3:
        raise ValueError(f"xyz must be (T, G, J, 3), got {x.shape}")
    T, G = x.shape[:2]
    seen = np.isfinite(x).all(-1)                      # (T, G, J)
    present = seen.any(-1)
    track = np.full((T, G), -1, np.int32)
    n_tracks = 0
    for t in range(T):
        pairs = []
        if t > 0:
            for g in np.flatnonzero(present[t]):
                for h in np.flatnonzero(present[t - 1]):
                    both = seen[t, g] & seen[t - 1, h]
                    if both.any():
                        d = float(np.linalg.norm(x[t, g, both] - x[t - 1, h, both], axis=-1).mean())
                        if d <= max_jump:
                            pairs.append((d, int(h), int(g)))
        used = set()
        for d, h, g in sorted(pairs):
            if track[t, g] < 0 and h not in used:
                track[t, g] = track[t - 1, h]
                used.add(h)
        for g in np.flatnonzero(present[t]):
            if track[t, g] < 0:
                track[t, g] = n_tracks
                n_tracks += 1
    return track


def track_people(xyz: torch.Tensor, **kw):
    """xyz (T, G, J, 3) float32 on the GPU -> (track (T, G) int32 on the device, -1 for an absent
    group; n_tracks, a 0-dim int32 tensor on the device).  kw: max_gap, max_jump, gap_growth,
    min_joints of ops.track_people.

    How it differs from link_tracks: it runs on the device in one stream-ordered launch (no copy of
    xyz to the host, no synchronisation; reading n_tracks as a Python int is the caller's
    choice), and a track survives up to max_gap (default 5) consecutive frames without an
    observation: the returning group is linked at lag k to the track's last observation while
    their distance is <= max_jump·(1 + gap_growth·(k − 1)), so a person occluded for a few frames
    keeps their number and the gap lies inside one trajectory, where refine.smooth_trajectory can
    fill it.  link_tracks ends a track at its first missed frame.  With max_gap=0 and
    min_joints=1 the track numbers are link_tracks' own."""
    if not isinstance(xyz, torch.Tensor) or xyz.dim() != 4:
        raise ValueError(f"xyz must be a (T, G, J, 3) tensor, got {tuple(getattr(xyz, 'shape', ()))}")
    from . import ops
    track, n_tracks, _, _ = ops.track_people(xyz, **kw)
    return track, n_tracks


def person_trajectories(track: torch.Tensor, arrays: dict, min_len: int = 1, max_people: int | None = None):
    """track (T, G) integer track numbers (-1 = absent; each number at most once per frame), arrays
    {name: tensor with leading dimensions (T, G)}, e.g. kpts_3d, kpts_3d_cov, tri_refine_status or
    the per-group kpts_2d -> (out {name: (T, Np, ...)}, present (T, Np) bool, chosen (Np,) int64).

    The tracks are ranked by the key (-frames present, track number); those present in at least
    min_len frames are kept, at most max_people of them.  out[name][t, p] is arrays[name][t, g] for
    the g with track[t, g] == chosen[p]; where person p is absent it is NaN for floating-point
    arrays and 0 for integer and bool ones.  Torch indexing on track's own device, as
    gather_groups; ranking the tracks by length takes one small device-to-host read, of the
    per-track frame counts (torch.bincount also reads the largest track number to size them)."""
    if not isinstance(track, torch.Tensor) or track.dim() != 2 or track.dtype.is_floating_point:
        raise ValueError("track must be a (T, G) integer tensor")
    T, G = track.shape
    for name, a in arrays.items():
        if not isinstance(a, torch.Tensor) or tuple(a.shape[:2]) != (T, G):
            raise ValueError(f"arrays[{name!r}] must be a tensor with leading dimensions {(T, G)}")
    if min_len < 1 or (max_people is not None and max_people < 0):
        raise ValueError(f"min_len={min_len} must be >= 1 and max_people={max_people} >= 0")
    dev = track.device
    tr = track.to(torch.int64)
    counts = torch.bincount((tr.clamp(min=-1) + 1).reshape(-1))[1:].cpu().numpy()      # the one host read
    order = sorted((i for i in range(len(counts)) if counts[i] >= min_len), key=lambda i: (-int(counts[i]), i))
    if max_people is not None:
        order = order[:int(max_people)]
    chosen = torch.tensor(order, dtype=torch.int64, device=dev)
    match = tr[:, :, None] == chosen[None, None, :]                      # (T, G, Np)
    present = match.any(1)
    g_of = match.to(torch.int8).argmax(1) if G > 0 and len(order) else torch.zeros((T, len(order)), dtype=torch.int64,
                                                                                  device=dev)
    rows = torch.arange(T, device=dev)[:, None]
    out = {}
    for name, a in arrays.items():
        a = a.to(dev)
        got = a[rows, g_of]                                              # (T, Np, ...)
        fill = float("nan") if a.dtype.is_floating_point else 0
        keep = present.reshape(present.shape + (1,) * (a.dim() - 2))
        out[name] = torch.where(keep, got, torch.full((), fill, dtype=a.dtype, device=dev))
    return out, present, chosen


def estimate_bone_lengths(xyz: torch.Tensor, pairs, valid: torch.Tensor | None = None, min_frames: int = 10):
    """Segment lengths of each person from their own 3D points, for skeleton_fit when nobody measured
    them: per person and segment the median over the frames of |X_b − X_a| where both ends are
    finite (and valid), e.g. the two-view frames of kpts_3d.  xyz (T, J, 3) or (T, Np, J, 3); pairs
    (n_seg, 2); valid (T, [Np,] J) bool or None.  Returns float32 (n_seg,) or (Np, n_seg) on xyz's
    device; NaN where fewer than min_frames frames have the segment, which switches it off in
    skeleton_fit.  Torch only, no host synchronisation."""
    if xyz.dim() not in (3, 4) or xyz.shape[-1] != 3:
        raise ValueError(f"xyz must be (T, J, 3) or (T, Np, J, 3), got {tuple(xyz.shape)}")
    pr = torch.as_tensor(np.asarray(pairs, dtype=np.int64).reshape(-1, 2), device=xyz.device)
    x = xyz.to(torch.float32)
    ok = torch.isfinite(x).all(-1)
    if valid is not None:
        if tuple(valid.shape) != tuple(xyz.shape[:-1]):
            raise ValueError(f"valid must be {tuple(xyz.shape[:-1])}, got {tuple(valid.shape)}")
        ok = ok & valid.to(device=xyz.device, dtype=torch.bool)
    a, b = pr[:, 0], pr[:, 1]
    d = torch.linalg.vector_norm(x.index_select(-2, b) - x.index_select(-2, a), dim=-1)       # (T, [Np,] n_seg)
    both = ok.index_select(-1, a) & ok.index_select(-1, b)
    d = torch.where(both, d, torch.full((), float("nan"), dtype=d.dtype, device=d.device))
    if d.shape[-1] == 0 or d.shape[0] == 0:
        return torch.full(d.shape[1:], float("nan"), dtype=torch.float32, device=d.device)
    med = torch.nanmedian(d, dim=0).values
    return torch.where(both.sum(0) >= int(min_frames), med, torch.full_like(med, float("nan")))
