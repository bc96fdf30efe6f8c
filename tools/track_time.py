#!/usr/bin/env python
"""Times mvpose.ops.track_people (mvp_track_people) on the GPU against people.link_tracks on the host.

    python tools/track_time.py [--out profiles/track_time.txt] [--T 100000] [--G 4] [--max-gap 5]
                               [--reps 1] [--host-frames 0]

T = 100 000 frames, G = 4, J = 17, max_gap = 5, the input resident on the device: the call (one
launch and the torch.empty of its outputs) timed with device events after a warm-up call, median
[min max] of 5 windows.  people.link_tracks, the host tracker it stands beside, is timed with
perf_counter on the same data, the copy of the device tensor to the host included, as its callers
pay it (--host-frames N times the first N frames only and scales to T; 0 = all of them).  Before
any time is reported the kernel's numbers at max_gap = 0 are compared with link_tracks' on the
frames timed, and its numbers at --max-gap with the restatement tests/track_ref.py on the first
300 frames.  The scene is tests/track_cases.py's crowd of three people with dropouts over 2 000
frames, repeated to T (at a seam the people are back at their first positions: some tracks end
there and new ones start, as at any other jump).  Needs a GPU: no fallback."""
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

import track_cases  # noqa: E402
import track_ref  # noqa: E402
from mvpose import ops, people  # noqa: E402
from sync_time import time_call  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_time.txt"))
    ap.add_argument("--T", type=int, default=100000)
    ap.add_argument("--G", type=int, default=4)
    ap.add_argument("--max-gap", type=int, default=5)
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--host-frames", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("track_time.py needs a GPU")
    T, G, J, T0 = args.T, args.G, 17, 2000
    x0 = track_cases._crowd(min(3, G), G, min(T, T0), J, 0, 4)
    x = np.concatenate([x0] * -(-T // len(x0)))[:T]
    xd = torch.tensor(x, device="cuda")
    kw = dict(max_gap=args.max_gap)
    nh = T if args.host_frames <= 0 else min(T, args.host_frames)

    track, n_tracks, cost, lag = ops.track_people(xd, return_links=True, **kw)
    nr = min(300, T)
    r = track_ref.track(x[:nr], **kw)
    if not (np.array_equal(track[:nr].cpu().numpy(), r["track"]) and np.array_equal(lag[:nr].cpu().numpy(), r["link_lag"])):
        sys.exit(f"the kernel's tracks differ from the restatement's on the first {nr} frames")
    t0 = time.perf_counter()
    host = people.link_tracks(xd[:nh])
    host_ms = (time.perf_counter() - t0) * 1e3 * T / nh
    t0g = ops.track_people(xd[:nh].contiguous(), max_gap=0)[0].cpu().numpy()
    if not np.array_equal(t0g, host):
        sys.exit(f"the kernel's tracks at max_gap=0 differ from link_tracks' on the first {nh} frames")
    dm = time_call(lambda: ops.track_people(xd, **kw), args.reps)
    dl = time_call(lambda: ops.track_people(xd, return_links=True, **kw), args.reps)
    lds = ops.track_people_plan(1, T, G, J, args.max_gap)
    lines = [f"# mvp_track_people, {torch.cuda.get_device_name(0)}, T={T} G={G} J={J} max_gap={args.max_gap}, other "
             f"parameters default, device events, median [min max] of 5 windows of {args.reps} call(s); "
             f"people.link_tracks: perf_counter over {nh} frames with its device-to-host copy, scaled to T",
             "# track_ms [min max] us_per_frame with_links_ms [min max] link_tracks_host_ms host/track tracks "
             "linked_at_lag_above_1 lds_bytes",
             f"{dm[0]:.3f} [{dm[1]:.3f} {dm[2]:.3f}] {dm[0] * 1e3 / T:.4f} {dl[0]:.3f} [{dl[1]:.3f} {dl[2]:.3f}] "
             f"{host_ms:.0f} {host_ms / dm[0]:.0f}x {int(n_tracks)} {int((lag > 1).sum())} {lds}"]
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
