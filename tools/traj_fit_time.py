#!/usr/bin/env python
"""Times mvpose.ops.trajectory_fit (mvp_trajectory_fit) on the GPU.

    python tools/traj_fit_time.py [--T 100000] [--reps 3] [--out profiles/traj_fit_time.txt]
                                  [--parent-lib PATH/libmvpose.so] [--sgd-T 400]

1. One trial, meaning all its launches, at (T, P) = (100 000, 17) with nv = 2 and 8 listed views:
   the call is timed with max_iter = 0, 1, 2, 3 and a tolerance no run reaches, so that every
   chain runs every trial; the differences are the first trial (solve, trial cost, sum, decide), and
   a later trial (the same plus the linearisation of the moved state).  Beside them: one
   ops.trajectory_fit_system call (the linearise launch plus the per-chain cost launch) and one
   mvp_trajectory_smooth call on the same shape, which the solve of a trial repeats with another
   frame source.  With --parent-lib the smoother is timed from that library too (a build of the
   commit before the solver moved into a shared header), both through plain ctypes in child
   processes, alternating, twice each.
2. A whole fit against mvp_sgd_refine (refine.refine_trajectories, its defaults, each camera
   against its own Gaussians, no body-length term) from the same seed on the same keypoints at
   (T, V) = (400, 8), each to its own stop: time, iterations, RMS error against the truth.

Device events around `reps` back-to-back calls after a warm-up of every shape, median [min, max]
of 5 windows.  Needs a GPU: no fallback."""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "multi-camera_3d_pose_estimation_amd")
for p in (ROOT, PKG):
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


def smooth_only(lib_path, T):
    """One library's mvp_trajectory_smooth through plain ctypes (a library from before this tool
    lacks the symbols mvpose._lib asks for): prints one JSON line."""
    lib = ctypes.CDLL(lib_path)
    rng = np.random.default_rng(0)
    t = np.arange(T)[:, None, None]
    xyz = (np.concatenate([100 + 50 * np.sin(t / 9.0), 200 + 30 * np.cos(t / 13.0), 300 + 0.01 * t], -1)
           + rng.normal(0.0, 1.0, (T, P, 3))).astype(np.float32)
    x = torch.tensor(xyz, device="cuda")
    out = torch.empty_like(x)
    nbytes = ctypes.c_int64(0)
    assert lib.mvp_trajectory_smooth_plan(T, P, 0, None, None, ctypes.byref(nbytes)) == 0
    work = torch.empty(nbytes.value, dtype=torch.uint8, device="cuda")
    vp = lambda a: ctypes.c_void_p(a.data_ptr())  # noqa: E731
    lib.mvp_trajectory_smooth.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 2 + [ctypes.c_double] + \
        [ctypes.c_float] * 2 + [ctypes.c_int, ctypes.c_void_p, ctypes.c_int64] + [ctypes.c_void_p] * 5
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fn():
        rc = lib.mvp_trajectory_smooth(vp(x), None, None, T, P, 1.0, 1.0, 0.0, 0, vp(work), nbytes.value, vp(out), None,
                                       None, None, stream)
        assert rc == 0
    med = time_call(fn, 10)
    digest = float(out.double().sum())
    print(json.dumps({"lib": lib_path, "T": T, "us": med, "sum": digest}))


def drop_views(kpts, share, rng):
    T, Pn, _, V = kpts.shape
    gone = rng.uniform(size=(T, Pn, V)) < share
    gone[..., 0] &= rng.uniform(size=(T, Pn)) < 0.5          # view 0 less often: most frames keep >= 1 view
    kpts[:, :, 0, :][gone] = np.nan
    return kpts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "traj_fit_time.txt"))
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--sgd-T", type=int, default=400)
    ap.add_argument("--smooth-only", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("traj_fit_time.py needs a GPU")
    if args.smooth_only:
        smooth_only(args.smooth_only, args.T)
        return
    from mvpose import ops, refine, synthetic as syn
    T = args.T
    lines = [f"# mvp_trajectory_fit, {torch.cuda.get_device_name(0)}, device events, median [min max] of 5 windows, us"]

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    truth = syn.make_poses(T, seed=1, jitter=0.0)
    rng = np.random.default_rng(2)
    seed = (truth + rng.normal(0.0, 1.0, truth.shape)).astype(np.float32)
    x0 = torch.tensor(seed, device="cuda")
    for nv in (2, 8):
        cams = syn.make_rig(nv, seed=3)
        kpts = drop_views(syn.make_kpts_2d(truth, cams, seed=3, noise_px=1.0), 0.2, rng)
        k = torch.tensor(kpts, device="cuda")
        cd = torch.tensor(ops.pack_cameras(syn.reference_camera_params(cams)), device="cuda")
        idx = list(range(nv))
        used, n_chunks, nbytes = ops.trajectory_fit_plan(T, P, 0)
        kw = dict(weights="conf", lambda_smooth=1.0, tol=1e-30)
        t = {}
        for it in (0, 1, 2, 3):
            t[it] = time_call(lambda: ops.trajectory_fit(k, cd, idx, x0, max_iter=it, **kw), args.reps)
            st = ops.trajectory_fit(k, cd, idx, x0, max_iter=it, **kw)[4].cpu().numpy()
            emit(f"T={T} P={P} nv={nv} chunk={used} workspace {nbytes / 1e6:.0f} MB  max_iter={it}: {fmt(t[it])} us per call; "
                 f"status values {sorted(set(hex(s) for s in st))}")
        tsys = time_call(lambda: ops.trajectory_fit_system(k, cd, idx, x0, weights="conf"), args.reps)
        tsm = time_call(lambda: ops.trajectory_smooth(x0, lambda_smooth=1.0), args.reps)
        emit(f"T={T} P={P} nv={nv}: seed path (max_iter=0) {t[0][0]:.0f}; first trial {t[1][0] - t[0][0]:.0f}; a later trial "
             f"with its linearisation {t[2][0] - t[1][0]:.0f} and {t[3][0] - t[2][0]:.0f}; trajectory_fit_system {fmt(tsys)}; "
             f"trajectory_smooth (this build, through ops) {fmt(tsm)}")
    if args.parent_lib:
        here = os.path.join(PKG, "mvpose", "libmvpose.so")
        for lib in (args.parent_lib, here) * 2:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--smooth-only", lib, "--T", str(T)],
                               capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.exit(f"child for {lib} failed:\n{r.stderr[-2000:]}")
            j = json.loads(r.stdout.strip().splitlines()[-1])
            emit(f"mvp_trajectory_smooth T={T} P={P} chunk=0, {'parent' if lib == args.parent_lib else 'this'} build: "
                 f"{fmt(j['us'])} us per call; sum of the output {j['sum']!r}")

    # a whole fit against the SGD refinement
    Ts, V = args.sgd_T, 8
    cams = syn.make_rig(V, seed=3)
    truth = syn.make_poses(Ts, seed=4, jitter=0.0)
    kpts = syn.make_kpts_2d(truth, cams, seed=5, noise_px=1.0)
    seed = (truth + np.random.default_rng(6).normal(0.0, 2.0, truth.shape)).astype(np.float32)
    k = torch.tensor(kpts, device="cuda")
    cd = torch.tensor(ops.pack_cameras(syn.reference_camera_params(cams)), device="cuda")
    x0 = torch.tensor(seed, device="cuda")
    rms = lambda a: float(np.sqrt(((np.asarray(a, np.float64) - truth) ** 2).sum(-1).mean()))  # noqa: E731
    fkw = dict(weights="unit", lambda_smooth=1.0, max_iter=30, tol=1e-6)
    tf_ = time_call(lambda: ops.trajectory_fit(k, cd, list(range(V)), x0, **fkw), 10)
    out, _, _, cost, status = ops.trajectory_fit(k, cd, list(range(V)), x0, **fkw)
    emit(f"whole fit T={Ts} P={P} V={V}, unit weights, lambda 1, tol 1e-6: {fmt(tf_)} us; trials "
         f"{sorted(set(int(s) & 63 for s in status.cpu().numpy()))}, status bits {sorted(set(int(s) & 0xC0 for s in status.cpu().numpy()))}; "
         f"RMS error seed {rms(seed):.3f} -> {rms(out.cpu().numpy()):.3f} cm")
    g = np.zeros((1, Ts, V, P, 6), np.float32)
    g[0, ..., 0], g[0, ..., 1] = kpts[:, :, 0, :].transpose(0, 2, 1), kpts[:, :, 1, :].transpose(0, 2, 1)
    g[0, ..., 2] = g[0, ..., 5] = 1.0
    G, X = torch.tensor(g, device="cuda"), x0[None].contiguous()
    camlist = [[c["K"], c["R"], c["T"], c["dist"]] for c in cams]
    skw = dict(lambda_smooth=1.0, lambda_body_length=0.0, own_camera_gaussians=True)
    ts_ = time_call(lambda: refine.refine_trajectories(G, X, camlist, **skw), 1)
    r = refine.refine_trajectories(G, X, camlist, **skw)
    best = r["best"][0].cpu().numpy()
    emit(f"mvp_sgd_refine on the same keypoints and seed (defaults: lr 0.001, patience 100, tolerance 1e-5, max_iter 1000; "
         f"own Gaussians, no body lengths): {fmt(ts_)} us; iterations {int(r['iters'][0])}; RMS error -> "
         f"{rms(r['final'][0].cpu().numpy()):.3f} cm (final), {rms(best) if np.isfinite(best).all() else float('nan'):.3f} cm (best)")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
