"""Several people per camera: what sits between ops.associate_views and the per-person stages
(no reference counterpart; the reference handles one person per camera).

* ``gather_groups``: the per-slot keypoints (and heatmap Gaussians) re-ordered by the group
  numbers of ops.associate_views into the single-person layout every later stage takes, one
  kpts_2d per group.  Torch indexing on the tensors' own device, no host synchronisation.
* ``link_tracks``: frame-to-frame identity of the triangulated groups, so that
  ops.trajectory_smooth can run per person.
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
