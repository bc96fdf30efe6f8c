"""Kernel time of mvp_triangulate_refine beside mvp_triangulate_robust at the same V, in the same
process: ms per 1 M points, HIP events on the launch stream.

    timeout -k 10 300 python tools/tri_refine_time.py --views 4
    timeout -k 10 300 python tools/tri_refine_time.py --views 8

Three variants over the same 1 M points (seeded synthetic rig, 1 px noise, tiled from 2,000 frames):
  robust_clean    mvp_triangulate_robust, every point accepted in step A; its points seed the others
  refine_unit     mvp_triangulate_refine, MVP_REFINE_W_UNIT, all outputs written
  refine_heatmap  mvp_triangulate_refine, MVP_REFINE_W_GAUSS with one anisotropic Gaussian per view
                  (eigenvalues 1..30 px², the keypoint as its mean), all outputs written
The C-ABI is called directly on preallocated outputs.  Each variant is warmed up, then timed in
ROUNDS rounds of REPS launches with the variants alternating; the median, minimum and maximum
round are printed, with the mean trial count, and one JSON line."""
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
ap.add_argument("--max_iter", type=int, default=10)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("tri_refine_time: needs a GPU (no CPU timing)")

V, J = args.views, 17
N = args.points // J * J
cams = syn.make_rig(V, seed=1)
base = syn.make_kpts_2d(syn.make_poses(2000, seed=2), cams, seed=3, noise_px=1.0).reshape(-1, 3, V)
clean = np.ascontiguousarray(np.tile(base, (N // base.shape[0] + 1, 1, 1))[:N])
rng = np.random.default_rng(4)
T = N // J
ev = rng.uniform(1.0, 30.0, (T, V, J, 2))
th = rng.uniform(0.0, np.pi, (T, V, J))
c, s = np.cos(th), np.sin(th)
gauss = np.empty((T, V, J, 6))
gauss[..., 0] = clean[:, 0].reshape(T, J, V).transpose(0, 2, 1)
gauss[..., 1] = clean[:, 1].reshape(T, J, V).transpose(0, 2, 1)
gauss[..., 2] = c * c * ev[..., 0] + s * s * ev[..., 1]
gauss[..., 3] = gauss[..., 4] = c * s * (ev[..., 0] - ev[..., 1])
gauss[..., 5] = s * s * ev[..., 0] + c * c * ev[..., 1]

dev = torch.device("cuda")
cd = torch.tensor(ops.pack_cameras(syn.reference_camera_params(cams)), device=dev)
kc, gd = torch.tensor(clean, device=dev), torch.tensor(gauss, device=dev)
ci = (ctypes.c_int * V)(*range(V))
seed = torch.empty((N, 3), dtype=torch.float32, device=dev)
mask = torch.empty((N,), dtype=torch.uint8, device=dev)
err = torch.empty((N, V), dtype=torch.float32, device=dev)
out = {k: {"xyz": torch.empty((N, 3), dtype=torch.float32, device=dev),
           "cov": torch.empty((N, 6), dtype=torch.float32, device=dev),
           "cost": torch.empty((N,), dtype=torch.float32, device=dev),
           "status": torch.empty((N,), dtype=torch.uint8, device=dev)} for k in ("refine_unit", "refine_heatmap")}
stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
ptr = lambda t: ctypes.c_void_p(t.data_ptr())


def robust():
    _lib.call("mvp_triangulate_robust", ptr(kc), N, V, ptr(cd), V, ci, V, 10.0, 0.0, ptr(seed), ptr(mask), ptr(err),
              stream)


def refine(name, weights):
    o = out[name]
    _lib.call("mvp_triangulate_refine", ptr(kc), N, V, ptr(cd), V, ci, V, ptr(seed), ptr(mask), weights,
              ptr(gd) if weights == ops.REFINE_W_GAUSS else None, J, 0.0, 1.0, args.max_iter, 1e-7, ptr(o["xyz"]),
              ptr(o["cov"]), ptr(o["cost"]), ptr(o["status"]), stream)


variants = {"robust_clean": robust, "refine_unit": lambda: refine("refine_unit", ops.REFINE_W_UNIT),
            "refine_heatmap": lambda: refine("refine_heatmap", ops.REFINE_W_GAUSS)}
for fn in variants.values():          # warm-up: code objects loaded, clocks up
    for _ in range(3):
        fn()
torch.cuda.synchronize()
assert bool((mask == (1 << V) - 1).all()), "clean data: some point left step A"
trials = {}
for name, o in out.items():
    st = o["status"]
    assert bool((st & 0xC0 == 0).all()), f"{name}: some point failed or did not converge"
    trials[name] = (float((st & 63).float().mean()), int((st & 63).max()))

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

res = {"views": V, "points": N, "rounds": args.rounds, "reps": args.reps, "max_iter": args.max_iter,
       "device": torch.cuda.get_device_name(0)}
print(f"V={V}, {N} points, {args.rounds} rounds x {args.reps} launches, ms per 1 M points (median [min, max]):")
for name, t in times.items():
    med = float(np.median(t))
    res[name + "_ms_per_Mpt"] = round(med, 4)
    res[name + "_min_max"] = [round(min(t), 4), round(max(t), 4)]
    print(f"  {name:15s} {med:8.4f}  [{min(t):.4f}, {max(t):.4f}]")
# x, y, conf per view + seed + mask byte read; xyz + cov + cost + status written; + 48 B per view of Gaussian
bytes_pt = {"refine_unit": 12 * V + 12 + 1 + 12 + 24 + 4 + 1, "refine_heatmap": 12 * V + 48 * V + 12 + 1 + 12 + 24 + 4 + 1}
for name in ("refine_unit", "refine_heatmap"):
    res[name + "_over_robust"] = round(res[name + "_ms_per_Mpt"] / res["robust_clean_ms_per_Mpt"], 3)
    res[name + "_trials_mean_max"] = [round(trials[name][0], 3), trials[name][1]]
    res[name + "_bytes_per_point"] = bytes_pt[name]
    print(f"  {name} / robust_clean {res[name + '_over_robust']}; trials mean {trials[name][0]:.3f} max "
          f"{trials[name][1]}; {bytes_pt[name]} B per point = "
          f"{bytes_pt[name] / res[name + '_ms_per_Mpt'] * 1e-3:.3f} TB/s algorithmic")
print(json.dumps(res))
