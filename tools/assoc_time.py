#!/usr/bin/env python
"""Times mvpose.ops.associate_views (mvp_associate_views) on the GPU.

    python tools/assoc_time.py [--out profiles/assoc_time.txt] [--T 100000] [--shapes 2x2 4x4 8x8]
                               [--reps 10] [--torch-reps 2] [--max-cost-px 8]

For T = 100 000 frames, J = 17 and (nv, P) = (2, 2), (4, 4), (8, 8): the call (three launches and the
workspace torch.empty) timed with device events around `reps` back-to-back calls after a warm-up,
median of 5 windows, once with the groups alone and once with the affinity output; and the same
affinity tensor with batched torch fp64 ops on the same GPU (the undistortion, the epipolar lines
F x_a and Fᵀ x_b once per pair, the (T, P, P, J) Sampson distances, truncated and averaged), timed
the same way.  The two affinity tensors are compared (the -1 pattern exactly, the values to rtol
1e-9) before any time is reported.  The grouping has no tensor-op counterpart: for scale, the
numpy restatement tests/people_ref.py is timed on the CPU over the first frames.  The scene is
tests/people_cases.py's (people on a 90 cm circle, shuffled slots, 15 % of the sightings and 10 %
of the joints lost) over 2 000 frames, repeated to T: a frame's work does not depend on its
neighbours.  Needs a GPU: no fallback."""
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

import people_cases  # noqa: E402
import people_ref  # noqa: E402
from mvpose import ops, synthetic as syn  # noqa: E402
from sync_time import time_call, torch_undistort  # noqa: E402

PEOPLE = {2: 2, 4: 3, 8: 6}          # people in the scene by slots per view


def torch_affinity(kpts, cams, cams_host, cam_idx, min_conf, trunc_px, min_joints):
    """The affinity of mvpose.h's "Cross-view association" with batched torch fp64 ops."""
    nan = torch.tensor(float("nan"), dtype=torch.float64, device=kpts.device)
    pts = []
    for c in cam_idx:
        x, y, conf = kpts[..., 0, c], kpts[..., 1, c], kpts[..., 2, c]           # (T, P, J)
        ux, uy = torch_undistort(x, y, cams[c])
        ok = torch.isfinite(x) & torch.isfinite(y) & ~torch.isnan(conf) & (conf >= min_conf)
        pts.append(torch.stack([torch.where(ok, ux, nan), torch.where(ok, uy, nan), torch.where(ok, 1.0, nan)], -1))
    nv = len(cam_idx)
    pairs = [(a, b) for a in range(nv) for b in range(a + 1, nv)]
    T, P = kpts.shape[:2]
    out = torch.empty((T, len(pairs), P, P), dtype=torch.float64, device=kpts.device)
    tau2 = float(np.float32(trunc_px)) ** 2
    for p, (a, b) in enumerate(pairs):
        ca, cb = cams_host[cam_idx[a]], cams_host[cam_idx[b]]
        Ka, Ra, Ta = ca[:9].reshape(3, 3), ca[14:23].reshape(3, 3), ca[23:26]
        Kb, Rb, Tb = cb[:9].reshape(3, 3), cb[14:23].reshape(3, 3), cb[23:26]
        R = Rb @ Ra.T
        t = Tb - R @ Ta
        tx = np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])
        F = torch.tensor(np.linalg.inv(Kb).T @ tx @ R @ np.linalg.inv(Ka), device=kpts.device)
        la = pts[a] @ F.T                      # F x_a   (T, P, J, 3)
        lb = pts[b] @ F                        # Fᵀ x_b
        num = (pts[b][:, None] * la[:, :, None]).sum(-1)                          # (T, P, P, J)
        den = (la[..., 0] ** 2 + la[..., 1] ** 2)[:, :, None] + (lb[..., 0] ** 2 + lb[..., 1] ** 2)[:, None]
        d2 = num * num / den
        ok = torch.isfinite(d2) & (den != 0)
        cnt = ok.sum(-1)
        s = torch.where(ok, d2.clamp(max=tau2), 0.0).sum(-1)
        out[:, p] = torch.where(cnt >= min_joints, s / cnt.clamp(min=1), -1.0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assoc_time.txt"))
    ap.add_argument("--T", type=int, default=100000)
    ap.add_argument("--shapes", nargs="*", default=["2x2", "4x4", "8x8"])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-reps", type=int, default=2)
    ap.add_argument("--ref-frames", type=int, default=20)
    ap.add_argument("--max-cost-px", type=float, default=8.0,
                    help="merge threshold; 0.05 merges nothing, which leaves the staging and the affinity")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("assoc_time.py needs a GPU")
    T, J, T0 = args.T, syn.N_JOINTS, 2000
    lines = [f"# mvp_associate_views, {torch.cuda.get_device_name(0)}, T={T} J={J}, max_cost_px={args.max_cost_px:g}, "
             f"other thresholds default, device events, "
             f"median [min max] of 5 windows; kernel {args.reps} calls per window, torch {args.torch_reps}",
             "# nv P people groups_ms [min max] us_per_frame with_affinity_ms [min max] torch_affinity_ms [min max] "
             "torch/with_affinity merges_per_frame affinity_terms_per_frame max_rel_affinity_diff pattern_equal "
             "lds_bytes workspace_MB restatement_cpu_ms_per_frame"]
    for shape in args.shapes:
        nv, P = (int(s) for s in shape.split("x"))
        cams, k0, _ = people_cases.scene(PEOPLE.get(P, max(1, P - 1)), nv, P, min(T, T0), seed=0)
        k = np.concatenate([k0] * -(-T // len(k0)))[:T]
        cams_host = ops.pack_cameras(syn.reference_camera_params(cams))
        kd = torch.tensor(k, device="cuda")
        cd = torch.tensor(cams_host, device="cuda")
        ci = list(range(nv))
        kw = dict(max_cost_px=args.max_cost_px)
        groups = lambda: ops.associate_views(kd, cd, ci, **kw)  # noqa: E731
        with_aff = lambda: ops.associate_views(kd, cd, ci, return_affinity=True, **kw)  # noqa: E731
        plain = lambda: torch_affinity(kd, cd, cams_host, ci, 0.0, 20.0, 5)  # noqa: E731
        g, c, a, pairs = with_aff()
        ta = plain()
        torch.cuda.synchronize()
        same = bool(torch.equal(a == -1.0, ta == -1.0))
        d = a != -1.0
        rel = float(((a[d] - ta[d]).abs() / ta[d]).max()) if same and bool(d.any()) else float("nan")
        if not same or not rel <= 1e-9:
            sys.exit(f"{shape}: kernel and torch affinities differ (pattern equal: {same}, max rel diff {rel:.3g})")
        g2, c2, _, _ = groups()
        if not (torch.equal(g, g2) and torch.equal(c, c2)):
            sys.exit(f"{shape}: the groups differ between the calls with and without the affinity output")
        nr = min(args.ref_frames, T)
        t0 = time.perf_counter()
        r = people_ref.associate(k[:nr], cams, ci, **kw)
        cpu_ms = (time.perf_counter() - t0) * 1e3 / nr
        if not (np.array_equal(r["group"], g[:nr].cpu().numpy()) and np.array_equal(r["count"], c[:nr].cpu().numpy())):
            sys.exit(f"{shape}: the kernel's groups differ from the restatement's on the first {nr} frames")
        gm = time_call(groups, args.reps)
        am = time_call(with_aff, args.reps)
        tm = time_call(plain, args.torch_reps)
        merges = float(((g >= 0).sum((1, 2)) - c[:, 0].long()).double().mean())
        lds, nbytes = ops.associate_views_plan(T, P, J, nv)
        row = (f"{nv} {P} {PEOPLE.get(P, max(1, P - 1))} {gm[0]:.3f} [{gm[1]:.3f} {gm[2]:.3f}] {gm[0] * 1e3 / T:.4f} "
               f"{am[0]:.3f} [{am[1]:.3f} {am[2]:.3f}] {tm[0]:.1f} [{tm[1]:.1f} {tm[2]:.1f}] {tm[0] / am[0]:.0f}x "
               f"{merges:.2f} {len(pairs) * P * P * J} {rel:.3g} {same} {lds} {nbytes / 1e6:.1f} {cpu_ms:.2f}")
        print(row, flush=True)
        lines.append(row)
        del kd, a, ta, g, c
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
