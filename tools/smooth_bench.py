#!/usr/bin/env python
"""Times mvpose.ops.trajectory_smooth (mvp_trajectory_smooth) on the GPU.

    python tools/smooth_bench.py [--out profiles/smooth_bench.txt] [--sweep-out profiles/smooth_chunk_sweep.txt]
                                 [--chunks 4 8 ...] [--reps 20] [--no-host]

For (T, P) = (100 000, 17) and (4 096, 17): the call with chunk = 0 (automatic), with the largest
allowed chunk (4 096: the closest setting to one lane per chain) and with every chunk of the
sweep.  Timed with device events around `reps` back-to-back calls after a warm-up of every shape
(the workspace torch.empty comes from torch's caching allocator after the first call); median of
5 such windows, in µs per call, with the bytes the three phases move and what share of the HBM
line (6.3 TB/s measured copy rate, MI355X) that is.  The host line is an fp64 banded solve of the
same problem: scipy.linalg.solveh_banded where scipy imports, else the numpy restatement
tests/traj_smooth_ref.solve_banded; the table says which.  Needs a GPU: no fallback."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "multi-camera_3d_pose_estimation_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from mvpose import ops  # noqa: E402
import traj_smooth_ref as ref  # noqa: E402

HBM_BPS = 6.3e12
SHAPES = [(100000, 17), (4096, 17)]
SWEEP = [4, 8, 16, 32, 48, 64, 72, 80, 88, 96, 128, 192, 256, 316, 352, 395, 448, 512, 768, 1024, 2048, 4096]


def traffic_bytes(T, P, chunk):
    """Bytes the three launches move, from the shapes: inputs read twice (eliminate, backsub:
    xyz 12 + cov 24 + valid 1 per frame), the factor written and read once (39 doubles per interior
    frame), the outputs (xyz 12 + resid 4 + observed 1), the Schur complements (90 doubles per
    lane, written and read) and the reduced system (63 + 6 doubles per separator and chain,
    written and read)."""
    used, n_chunks, _ = ops.trajectory_smooth_plan(T, P, chunk)
    n_seps = (T - used - 1) // (used + 2) + 1 if T > used else 0
    interior = T - 2 * n_seps if n_seps else T
    frames = T * P
    b = 2 * 37 * frames + 17 * frames
    b += 2 * 39 * 8 * interior * P
    b += 2 * 90 * 8 * n_chunks * P
    b += 2 * 69 * 8 * n_seps * P
    return b


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


def host_solve(c, lam):
    """-> (name, seconds, xyz float64) of one fp64 banded solve of all chains on the host."""
    try:
        from scipy.linalg import solveh_banded
    except ImportError:
        t0 = time.perf_counter()
        r = ref.solve_banded(c["xyz"], c["cov"], c["valid"], lambda_smooth=lam)
        return "numpy traj_smooth_ref.solve_banded", time.perf_counter() - t0, r.x64
    W, z, obs = ref.weights(c["xyz"], c["cov"], c["valid"])
    T, P = obs.shape
    t0 = time.perf_counter()
    kd = np.zeros(T)
    kd[:-2] += 1
    kd[1:-1] += 4
    kd[2:] += 1
    k1 = np.zeros(T)
    k1[:-2] += -2
    k1[1:-1] += -2
    X = np.zeros((T, P, 3))
    for p in range(P):
        ab = np.zeros((7, 3 * T))       # lower form: ab[i, j] = A[j + i, j], bandwidth 6
        for a in range(3):
            for b in range(a, 3):
                ab[b - a, a:3 * T:3] += W[:, p, b, a]
        ab[0] += lam * np.repeat(kd, 3)
        ab[3, :3 * T - 3] += lam * np.repeat(k1, 3)[:3 * T - 3]
        ab[6, :3 * T - 6] += lam
        rhs = np.einsum("tij,tj->ti", W[:, p], z[:, p]).reshape(-1)
        X[:, p] = solveh_banded(ab, rhs, lower=True).reshape(T, 3)
    return "scipy.linalg.solveh_banded", time.perf_counter() - t0, X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smooth_bench.txt"))
    ap.add_argument("--sweep-out", default=os.path.join(ROOT, "profiles", "smooth_chunk_sweep.txt"))
    ap.add_argument("--chunks", type=int, nargs="*", default=SWEEP)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("smooth_bench.py needs a GPU")
    lam = 1.0
    lines = [f"# mvp_trajectory_smooth, {torch.cuda.get_device_name(0)}, device events, {args.reps} calls per window, "
             "median [min, max] of 5 windows", "# T P chunk(requested) chunk(used) n_chunks us_per_call [min max] "
             "MB_moved TB/s share_of_6.3TB/s workspace_MB"]
    sweep = list(lines)
    host = []
    for T, P in SHAPES:
        c = ref.make_case(T, P, seed=1, long_gap=400)
        xyz = torch.tensor(c["xyz"], device="cuda")
        cov = torch.tensor(ref._cov6(c["cov"]), device="cuda")
        valid = torch.tensor(c["valid"], device="cuda")
        first = None
        for chunk in [0, 4096] + [k for k in args.chunks if k != 4096]:
            used, n_chunks, nbytes = ops.trajectory_smooth_plan(T, P, chunk)
            fn = lambda: ops.trajectory_smooth(xyz, cov, valid, lambda_smooth=lam, chunk=chunk)  # noqa: E731
            reps = max(2, args.reps // 10) if used < 16 and T > 10000 else args.reps   # a long serial reduce
            med, lo, hi = time_call(fn, reps)
            out = fn()[0]
            if first is None:
                first = out
            dmax = float((out - first).abs().nan_to_num(0).max())
            mb = traffic_bytes(T, P, chunk)
            row = (f"{T} {P} {chunk} {used} {n_chunks} {med:.1f} [{lo:.1f} {hi:.1f}] {mb / 1e6:.1f} "
                   f"{mb / med / 1e6:.3f} {100 * mb / med / 1e-6 / HBM_BPS:.1f}% {nbytes / 1e6:.1f}"
                   f"  max|xyz - xyz(chunk=0)| {dmax:.2g}")
            print(row, flush=True)
            (lines if chunk in (0, 4096) else sweep).append(row)
            if chunk in (0, 4096):
                sweep.append(row)
        if not args.no_host:
            name, sec, X = host_solve(c, lam)
            err = float(np.nanmax(np.abs(first.cpu().numpy().astype(np.float64) - X)))
            host.append(f"host {name}: T={T} P={P} {sec * 1e6:.0f} us per solve (one thread; weights not timed); "
                        f"max |device - host| {err:.3g}")
            print(host[-1], flush=True)
    lines += host
    for path, body in ((args.out, lines), (args.sweep_out, sweep)):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(body) + "\n")


if __name__ == "__main__":
    main()
