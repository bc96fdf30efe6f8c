"""Kernel time of mvp_triangulate_robust beside the all-views DLT (MVP_TRI_ALL_VIEWS, default
solver) at the same V, in the same process: ms per 1 M points, HIP events on the launch stream.

    timeout -k 10 300 python tools/tri_robust_time.py --views 4
    timeout -k 10 300 python tools/tri_robust_time.py --views 8

Three variants over the same 1 M points (seeded synthetic rig, 1 px noise, tiled from 2,000 frames):
  all_views    mvp_triangulate, MVP_TRI_ALL_VIEWS
  robust_clean mvp_triangulate_robust, every point accepted in step A (checked: all masks full,
               xyz bit-identical to all_views)
  robust_10pct mvp_triangulate_robust with one view of 10 % of the points pushed 80-300 px
The C-ABI is called directly on preallocated outputs (no allocation or mask unpacking in the timed
window).  Each variant is warmed up, then timed in ROUNDS rounds of REPS launches with the
variants alternating; the median, minimum and maximum round are printed, and one JSON line."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-camera_3d_pose_estimation_amd"))
import numpy as np
import torch
from mvpose import _lib, ops, synthetic as syn

ap = argparse.ArgumentParser()
ap.add_argument("--views", type=int, default=4)
ap.add_argument("--points", type=int, default=1_000_000)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--inlier_px", type=float, default=10.0)
ap.add_argument("--contaminated", type=float, default=0.10)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("tri_robust_time: needs a GPU (no CPU timing)")

V, N = args.views, args.points
cams = syn.make_rig(V, seed=1)
base = syn.make_kpts_2d(syn.make_poses(2000, seed=2), cams, seed=3, noise_px=1.0).reshape(-1, 3, V)
clean = np.ascontiguousarray(np.tile(base, (N // base.shape[0] + 1, 1, 1))[:N])
rng = np.random.default_rng(4)
dirty = clean.copy()
bad = np.flatnonzero(rng.random(N) < args.contaminated)
view = rng.integers(0, V, bad.size)
r, th = rng.uniform(80.0, 300.0, bad.size), rng.uniform(0.0, 2 * np.pi, bad.size)
dirty[bad, 0, view] += (r * np.cos(th)).astype(np.float32)
dirty[bad, 1, view] += (r * np.sin(th)).astype(np.float32)

dev = torch.device("cuda")
cd = torch.tensor(ops.pack_cameras(syn.reference_camera_params(cams)), device=dev)
kc, kd = torch.tensor(clean, device=dev), torch.tensor(dirty, device=dev)
ci = (ctypes.c_int * V)(*range(V))
xyz = {k: torch.empty((N, 3), dtype=torch.float32, device=dev) for k in ("all_views", "robust_clean", "robust_10pct")}
mask = {k: torch.empty((N,), dtype=torch.uint8, device=dev) for k in ("robust_clean", "robust_10pct")}
err = torch.empty((N, V), dtype=torch.float32, device=dev)
stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
ptr = lambda t: ctypes.c_void_p(t.data_ptr())


def all_views():
    _lib.call("mvp_triangulate", ptr(kc), N, V, ptr(cd), V, ci, V, ops.TRI_ALL_VIEWS, ptr(xyz["all_views"]), None,
              stream)


def robust(name, k):
    _lib.call("mvp_triangulate_robust", ptr(k), N, V, ptr(cd), V, ci, V, args.inlier_px, 0.0, ptr(xyz[name]),
              ptr(mask[name]), ptr(err), stream)


variants = {"all_views": all_views, "robust_clean": lambda: robust("robust_clean", kc),
            "robust_10pct": lambda: robust("robust_10pct", kd)}
for fn in variants.values():          # warm-up: code objects loaded, clocks up
    for _ in range(3):
        fn()
torch.cuda.synchronize()
full = (1 << V) - 1
assert bool((mask["robust_clean"] == full).all()), "clean data: some point left step A"
assert torch.equal(xyz["robust_clean"].view(torch.int32), xyz["all_views"].view(torch.int32)), \
    "clean data: robust xyz differs from the all-views DLT"
rejected = int((mask["robust_10pct"] != full).sum())

times = {k: [] for k in variants}
for _ in range(args.rounds):
    for name, fn in variants.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        times[name].append(e0.elapsed_time(e1) / args.reps * 1e6 / N)

res = {"views": V, "points": N, "rounds": args.rounds, "reps": args.reps, "inlier_px": args.inlier_px,
       "contaminated_points": int(bad.size), "points_with_a_rejected_view": rejected,
       "device": torch.cuda.get_device_name(0)}
print(f"V={V}, {N} points, {args.rounds} rounds x {args.reps} launches, ms per 1 M points (median [min, max]):")
for name, t in times.items():
    med = float(np.median(t))
    res[name + "_ms_per_Mpt"] = round(med, 4)
    res[name + "_min_max"] = [round(min(t), 4), round(max(t), 4)]
    print(f"  {name:13s} {med:8.4f}  [{min(t):.4f}, {max(t):.4f}]")
res["clean_over_all_views"] = round(res["robust_clean_ms_per_Mpt"] / res["all_views_ms_per_Mpt"], 3)
res["contaminated_over_all_views"] = round(res["robust_10pct_ms_per_Mpt"] / res["all_views_ms_per_Mpt"], 3)
read_b, write_b = 12 * V, 12 + 1 + 4 * V
print(f"  robust_clean / all_views {res['clean_over_all_views']}, robust_10pct / all_views "
      f"{res['contaminated_over_all_views']}; {read_b} B read + {write_b} B written per point = "
      f"{(read_b + write_b) / res['robust_clean_ms_per_Mpt'] * 1e-3:.3f} TB/s algorithmic (clean)")
print(json.dumps(res))
