"""Kernel time of mvp_triangulate_peaks beside mvp_triangulate_robust at the same V, and of
mvp_heatmap_peaks beside mvp_heatmap_decode, in the same process: HIP events on the launch stream.

    timeout -k 10 300 python tools/tri_peaks_time.py --views 4
    timeout -k 10 300 python tools/tri_peaks_time.py --views 8

Triangulation, ms per 1 M points (seeded synthetic rig, 1 px noise, tiled from 2,000 frames):
  robust_clean   mvp_triangulate_robust on the clean points: the baseline
  peaks_m1_clean mvp_triangulate_peaks, M = 1, the same points (checked: xyz and masks bit-identical)
  peaks_m4_clean mvp_triangulate_peaks, M = 4: slot 0 the clean point, slots 1-3 decoys 80-300 px
                 away with lower scores; every point is accepted in step A (checked: all masks
                 full, every sel 0, xyz bit-identical to the baseline)
  robust_10pct   mvp_triangulate_robust with one view of 10 % of the points pushed 80-300 px
  peaks_m4_10pct mvp_triangulate_peaks, M = 4, on those points with the displaced position in slot 0
                 and the true one in slot 1 of that view: step B recovers it (checked: all masks full)
2D stage, ms per launch over 1024 x 17 maps of 64 x 48 (a blob and a second mode on noise):
  decode         mvp_heatmap_decode without the flip test
  heatmap_peaks  mvp_heatmap_peaks, max_peaks 4, radius 1, thr 0.1, min_rel 0.3
The C-ABI is called directly on preallocated outputs.  Each variant is warmed up, then timed in
ROUNDS rounds of REPS launches with the variants alternating; the median, minimum and maximum round
are printed, and one JSON line."""
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
ap.add_argument("--crops", type=int, default=1024)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("tri_peaks_time: needs a GPU (no CPU timing)")

V, N, M = args.views, args.points, ops.MAX_PEAKS
cams = syn.make_rig(V, seed=1)
base = syn.make_kpts_2d(syn.make_poses(2000, seed=2), cams, seed=3, noise_px=1.0).reshape(-1, 3, V)
clean = np.ascontiguousarray(np.tile(base, (N // base.shape[0] + 1, 1, 1))[:N])
rng = np.random.default_rng(4)


def offsets(shape):
    r, th = rng.uniform(80.0, 300.0, shape), rng.uniform(0.0, 2 * np.pi, shape)
    return (r * np.cos(th)).astype(np.float32), (r * np.sin(th)).astype(np.float32)


pk_clean = np.empty((N, M, 3, V), np.float32)
pk_clean[:, 0] = clean
for m in range(1, M):
    dx, dy = offsets((N, V))
    pk_clean[:, m, 0], pk_clean[:, m, 1] = clean[:, 0] + dx, clean[:, 1] + dy
    pk_clean[:, m, 2] = clean[:, 2] * np.float32(0.8 ** m)
dirty = clean.copy()
bad = np.flatnonzero(rng.random(N) < args.contaminated)
view = rng.integers(0, V, bad.size)
dx, dy = offsets(bad.size)
dirty[bad, 0, view] += dx
dirty[bad, 1, view] += dy
pk_dirty = pk_clean.copy()
pk_dirty[bad, 1, :, view] = clean[bad, :, view]            # the truth, second
pk_dirty[bad, 0, :, view] = dirty[bad, :, view]            # the displaced argmax, first

dev = torch.device("cuda")
cd = torch.tensor(ops.pack_cameras(syn.reference_camera_params(cams)), device=dev)
kc, kd = torch.tensor(clean, device=dev), torch.tensor(dirty, device=dev)
pc, pd = torch.tensor(pk_clean, device=dev), torch.tensor(pk_dirty, device=dev)
ci = (ctypes.c_int * V)(*range(V))
names = ("robust_clean", "peaks_m1_clean", "peaks_m4_clean", "robust_10pct", "peaks_m4_10pct")
xyz = {k: torch.empty((N, 3), dtype=torch.float32, device=dev) for k in names}
mask = {k: torch.empty((N,), dtype=torch.uint8, device=dev) for k in names}
sel = {k: torch.empty((N, V), dtype=torch.int8, device=dev) for k in names}
err = torch.empty((N, V), dtype=torch.float32, device=dev)
kout = torch.empty((N, 3, V), dtype=torch.float32, device=dev)
stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
ptr = lambda t: ctypes.c_void_p(t.data_ptr())


def robust(name, k):
    _lib.call("mvp_triangulate_robust", ptr(k), N, V, ptr(cd), V, ci, V, args.inlier_px, 0.0, ptr(xyz[name]),
              ptr(mask[name]), ptr(err), stream)


def peaks(name, p, m):
    _lib.call("mvp_triangulate_peaks", ptr(p), N, m, V, ptr(cd), V, ci, V, args.inlier_px, 0.0, ptr(xyz[name]),
              ptr(mask[name]), ptr(sel[name]), ptr(err), ptr(kout), stream)


# 2D stage: 1024 x 17 maps with a main blob, a second mode at 60 % and noise
C, K, H, W = args.crops, 17, 64, 48
g = torch.Generator(device=dev).manual_seed(5)
ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32),
                        torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
cx = torch.rand((C, K, 2, 1, 1), device=dev, generator=g) * (W - 1)
cy = torch.rand((C, K, 2, 1, 1), device=dev, generator=g) * (H - 1)
amp = torch.tensor([0.9, 0.54], device=dev).reshape(1, 1, 2, 1, 1)
hm = (amp * torch.exp(-((xs - cx) ** 2 + (ys - cy) ** 2) / 4.5)).amax(2)
hm = torch.maximum(hm, torch.rand((C, K, H, W), device=dev, generator=g) * 0.02).contiguous()
cs = torch.tensor([[640.0, 360.0, 1600.0, 2133.3333]], device=dev).repeat(C, 1).contiguous()
d_kp = torch.empty((C, K, 2), dtype=torch.float32, device=dev)
d_sc = torch.empty((C, K), dtype=torch.float32, device=dev)
h_pk = torch.empty((C, K, M, 3, 1), dtype=torch.float32, device=dev)
h_ct = torch.empty((C, K, 1), dtype=torch.int32, device=dev)


def decode():
    _lib.call("mvp_heatmap_decode", ptr(hm), None, C, K, H, W, None, 0, ptr(cs), 192, 256, None, ptr(d_kp), ptr(d_sc),
              None, None, 1, stream)


def heatmap_peaks():
    _lib.call("mvp_heatmap_peaks", ptr(hm), C, K, H, W, ptr(cs), 192, 256, M, 1, 0.1, 0.3, 1, ptr(h_pk), ptr(h_ct),
              stream)


variants = {"robust_clean": lambda: robust("robust_clean", kc),
            "peaks_m1_clean": lambda: peaks("peaks_m1_clean", kc, 1),
            "peaks_m4_clean": lambda: peaks("peaks_m4_clean", pc, M),
            "robust_10pct": lambda: robust("robust_10pct", kd),
            "peaks_m4_10pct": lambda: peaks("peaks_m4_10pct", pd, M),
            "decode": decode, "heatmap_peaks": heatmap_peaks}
for fn in variants.values():          # warm-up: code objects loaded, clocks up
    for _ in range(3):
        fn()
torch.cuda.synchronize()
full = (1 << V) - 1
for name in ("peaks_m1_clean", "peaks_m4_clean"):
    assert bool((mask[name] == full).all()), f"{name}: some point left step A"
    assert torch.equal(xyz[name].view(torch.int32), xyz["robust_clean"].view(torch.int32)), f"{name}: xyz differs"
assert bool((sel["peaks_m4_clean"] == 0).all())
assert bool((mask["peaks_m4_10pct"] == full).all()), "contaminated data: a displaced view was not recovered"
recovered = int((sel["peaks_m4_10pct"] == 1).any(-1).sum())
assert torch.equal(h_pk[:, :, 0, :2, 0].view(torch.int32), d_kp.view(torch.int32)), "first peak is not the decode"
two_modes = float((h_ct >= 2).float().mean())

times = {k: [] for k in variants}
for _ in range(args.rounds):
    for name, fn in variants.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        per = e0.elapsed_time(e1) / args.reps
        times[name].append(per if name in ("decode", "heatmap_peaks") else per * 1e6 / N)

res = {"views": V, "points": N, "rounds": args.rounds, "reps": args.reps, "inlier_px": args.inlier_px,
       "contaminated_points": int(bad.size), "points_recovered_from_slot_1": recovered, "maps": C * K,
       "maps_with_two_modes": round(two_modes, 3), "device": torch.cuda.get_device_name(0)}
print(f"V={V}, {N} points, {C * K} maps, {args.rounds} rounds x {args.reps} launches, median [min, max]:")
for name, t in times.items():
    med = float(np.median(t))
    unit = "ms_per_launch" if name in ("decode", "heatmap_peaks") else "ms_per_Mpt"
    res[f"{name}_{unit}"] = round(med, 4)
    res[name + "_min_max"] = [round(min(t), 4), round(max(t), 4)]
    print(f"  {name:15s} {med:8.4f} {unit}  [{min(t):.4f}, {max(t):.4f}]")
for name in ("peaks_m1_clean", "peaks_m4_clean"):
    res[name + "_over_robust"] = round(res[name + "_ms_per_Mpt"] / res["robust_clean_ms_per_Mpt"], 3)
res["peaks_m4_10pct_over_robust_10pct"] = round(res["peaks_m4_10pct_ms_per_Mpt"] / res["robust_10pct_ms_per_Mpt"], 3)
print(f"  peaks M=1 / robust {res['peaks_m1_clean_over_robust']}, M=4 / robust {res['peaks_m4_clean_over_robust']} "
      f"(clean); M=4 / robust at 10 % contaminated {res['peaks_m4_10pct_over_robust_10pct']}")
print(json.dumps(res))
