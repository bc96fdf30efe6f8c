"""Left/right label swaps of the 2D detector, per camera (no reference counterpart: the reference
takes the joint labels on trust).  The model is stated in include/mvpose.h ("Left/right label
swaps per camera"); the kernels are in csrc/label_swap.hip.

* ``COCO_PAIRS``: the eight (left, right) pairs of the 17 COCO joints.
* ``PRESETS`` / ``preset``: which pairs are exchanged together.  "limbs": arms (shoulders, elbows,
  wrists) and legs (hips, knees, ankles) as two units; "body": the same six pairs as one unit.
  Both leave out the eye and ear pairs: they lie a few pixels apart, so neither the epipolar nor
  the motion term can tell their two labellings apart.
* ``fix_label_swaps``: host arrays and the reference's camera_params in, fixed arrays out.
"""
from __future__ import annotations

import numpy as np

COCO_PAIRS = ((1, 2), (3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14), (15, 16))
_LIMB_PAIRS = COCO_PAIRS[2:]
PRESETS = {
    "limbs": (_LIMB_PAIRS, (0, 0, 0, 1, 1, 1)),
    "body": (_LIMB_PAIRS, (0, 0, 0, 0, 0, 0)),
}


def preset(name: str):
    """-> (pairs (NS, 2) int32, units (NS,) int32) of a preset."""
    if name not in PRESETS:
        raise ValueError(f"label-swap preset {name!r}: one of {tuple(PRESETS)}")
    pairs, units = PRESETS[name]
    return np.asarray(pairs, np.int32), np.asarray(units, np.int32)


def fix_label_swaps(kpts_2d, camera_params, camera_indices=None, units="limbs", heatmaps_2d=None, min_conf=0.0,
                    trunc_px=20.0, motion_trunc_px=40.0, motion_weight=1.0, swap_prior_px=2.0, device=None):
    """Undo the per-camera left/right exchanges of kpts_2d (T, J, 3, V) (ops.fix_label_swaps on
    host arrays).

    camera_params {key: [K, R, T, dist]} as for get_pose_3D, camera_indices the keys of the cameras
    that take part (default: all): view i is camera camera_indices[i], read from the column of
    kpts_2d at that key's position in camera_params; other columns are returned unchanged.  units:
    a preset name or (pairs (NS, 2), units (NS,)).  heatmaps_2d (T, V, J, C) or None is exchanged
    with the keypoints.  Returns (kpts_2d float32, heatmaps_2d in its own dtype or None,
    swap (T, U) uint8: bit i set where view i's labels of unit u were exchanged)."""
    import torch
    from . import ops
    keys = list(camera_params.keys())
    if camera_indices is None:
        camera_indices = keys
    positions = [keys.index(c) for c in camera_indices]
    pairs, unit = preset(units) if isinstance(units, str) else units
    dev = torch.device(device if device is not None else "cuda")
    kp = torch.as_tensor(np.ascontiguousarray(np.asarray(kpts_2d, dtype=np.float32)), device=dev)
    cams = torch.tensor(ops.pack_cameras(camera_params), device=dev)
    gauss = None
    if heatmaps_2d is not None:
        gauss = torch.as_tensor(np.ascontiguousarray(np.asarray(heatmaps_2d, dtype=np.float64)), device=dev)
    fixed, gfixed, swap = ops.fix_label_swaps(kp, cams, positions, pairs, unit, gauss=gauss, min_conf=min_conf,
                                              trunc_px=trunc_px, motion_trunc_px=motion_trunc_px,
                                              motion_weight=motion_weight, swap_prior_px=swap_prior_px)
    if gfixed is not None:
        gfixed = gfixed.cpu().numpy().astype(np.asarray(heatmaps_2d).dtype, copy=False)
    return fixed.cpu().numpy(), gfixed, swap.cpu().numpy()
