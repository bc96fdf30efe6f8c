#!/usr/bin/env python
"""Times mvpose.ops.trajectory_smooth_cov and trajectory_fit_cov (mvp_trajectory_smooth_cov,
mvp_trajectory_fit_cov) on the GPU against the calls whose factorisation they share.

    python tools/traj_cov_time.py [--T 100000] [--reps 10] [--out profiles/traj_cov_time.txt]

At (T, P) = (100 000, 17), chunk 0 (automatic):
1. trajectory_smooth_cov against trajectory_smooth on the same inputs (tools/smooth_bench.py's:
   covariances and a valid mask, 20 % of the frames knocked out).  The smoother's kernels are
   instantiated from the same header as before the covariance calls existed and with the same
   frame source, so this build's smoother is the one to compare with.
2. trajectory_fit_cov (validity pass, linearisation, the three sweeps) against one trial of
   trajectory_fit (the call with max_iter = 1 minus the call with max_iter = 0, a tolerance no run
   reaches), two listed views, tools/traj_fit_time.py's inputs.

Device events around `reps` back-to-back calls after a warm-up, median [min, max] of 5 windows, in
µs per call.  Needs a GPU: no fallback."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "multi-camera_3d_pose_estimation_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

P = 17


def time_call(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / reps)
    return float(np.median(out)), float(min(out)), float(max(out))


def fmt(t):
    return f"{t[0]:.0f} [{t[1]:.0f} {t[2]:.0f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "traj_cov_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("traj_cov_time.py needs a GPU")
    from mvpose import ops, synthetic as syn
    import traj_smooth_ref as ref
    T = args.T
    lines = [f"# trajectory covariances, {torch.cuda.get_device_name(0)}, device events, {args.reps} calls per window, "
             "median [min max] of 5 windows, us per call"]

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    c = ref.make_case(T, P, seed=1, long_gap=400)
    xyz = torch.tensor(c["xyz"], device="cuda")
    cov = torch.tensor(ref._cov6(c["cov"]), device="cuda")
    valid = torch.tensor(c["valid"], device="cuda")
    used, n_chunks, nb0 = ops.trajectory_smooth_plan(T, P, 0)
    nb1 = ops.trajectory_smooth_cov_plan(T, P, 0)[2]
    ts = time_call(lambda: ops.trajectory_smooth(xyz, cov, valid, lambda_smooth=1.0), args.reps)
    tc = time_call(lambda: ops.trajectory_smooth_cov(xyz, cov, valid, lambda_smooth=1.0), args.reps)
    tn = time_call(lambda: ops.trajectory_smooth_cov(xyz, cov, valid, lambda_smooth=1.0, want_cross=False), args.reps)
    emit(f"T={T} P={P} chunk={used} ({n_chunks} chunks): trajectory_smooth {fmt(ts)} (workspace {nb0 / 1e6:.0f} MB); "
         f"trajectory_smooth_cov {fmt(tc)} (workspace {nb1 / 1e6:.0f} MB), ratio {tc[0] / ts[0]:.2f}; without the lag-1 "
         f"blocks {fmt(tn)}, ratio {tn[0] / ts[0]:.2f}")

    truth = syn.make_poses(T, seed=1, jitter=0.0)
    rng = np.random.default_rng(2)
    x0 = torch.tensor((truth + rng.normal(0.0, 1.0, truth.shape)).astype(np.float32), device="cuda")
    cams = syn.make_rig(2, seed=3)
    kpts = syn.make_kpts_2d(truth, cams, seed=3, noise_px=1.0)
    gone = rng.uniform(size=(T, P, 2)) < 0.2
    gone[..., 0] &= rng.uniform(size=(T, P)) < 0.5
    kpts[:, :, 0, :][gone] = np.nan
    k = torch.tensor(kpts, device="cuda")
    cd = torch.tensor(ops.pack_cameras(syn.reference_camera_params(cams)), device="cuda")
    kw = dict(weights="conf", lambda_smooth=1.0)
    t0 = time_call(lambda: ops.trajectory_fit(k, cd, [0, 1], x0, max_iter=0, tol=1e-30, **kw), args.reps)
    t1 = time_call(lambda: ops.trajectory_fit(k, cd, [0, 1], x0, max_iter=1, tol=1e-30, **kw), args.reps)
    tf = time_call(lambda: ops.trajectory_fit_cov(k, cd, [0, 1], x0, **kw), args.reps)
    status = ops.trajectory_fit_cov(k, cd, [0, 1], x0, **kw)[2].cpu().numpy()
    trial = t1[0] - t0[0]
    emit(f"T={T} P={P} nv=2: trajectory_fit max_iter=0 {fmt(t0)}, max_iter=1 {fmt(t1)}, one trial {trial:.0f}; "
         f"trajectory_fit_cov {fmt(tf)} (workspace {ops.trajectory_fit_cov_plan(T, P, 0)[2] / 1e6:.0f} MB), ratio to one "
         f"trial {tf[0] / trial:.2f}; status values {sorted(set(hex(s) for s in status))}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
