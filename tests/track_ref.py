"""numpy restatement of mvp_track_people (the rules are stated in include/mvpose.h), written from
the statement and not from the kernel: plain loops over frames, lags and groups, the candidates
sorted as tuples.  It also returns, per frame, the smallest relative margin of the comparisons the
kernel's numbers are bound by: every defined cost of an (open observation, present group) pair
against its lag's limit, and every two candidates' costs of the frame against each other (the
closest two are neighbours in the sorted order)."""
import numpy as np


def cost(a, b, min_joints=1):
    """a, b (J, 3) float64 -> the mean joint distance over the joints finite in both, summed in
    ascending joint order, or None when fewer than min_joints are."""
    both = np.isfinite(a).all(-1) & np.isfinite(b).all(-1)
    n = int(both.sum())
    if n < min_joints or n == 0:
        return None
    d = a[both] - b[both]
    s = 0.0
    for v in np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]):
        s += float(v)
    return s / n


def track(xyz, max_gap=5, max_jump=50.0, gap_growth=0.5, min_joints=1):
    """xyz (T, G, J, 3) -> {"track" (T, G) int32, "n_tracks" int, "link_cost" (T, G) float64,
    "link_lag" (T, G) uint8, "margins" (T,) float64 (inf for a frame without comparisons)}."""
    x32 = np.asarray(xyz, dtype=np.float32)
    assert x32.ndim == 4 and x32.shape[3] == 3
    x = x32.astype(np.float64)
    T, G = x.shape[:2]
    K = int(max_gap) + 1
    mj, gg = float(np.float32(max_jump)), float(np.float32(gap_growth))
    present = np.isfinite(x).all(-1).any(-1)
    out = np.full((T, G), -1, np.int32)
    link_cost = np.full((T, G), np.nan)
    link_lag = np.zeros((T, G), np.uint8)
    margins = np.full(T, np.inf)
    latest = {}                                   # track -> (frame, group) of its latest observation
    n_tracks = 0
    for t in range(T):
        cand = []
        for tr, (t0, h) in latest.items():
            k = t - t0
            if not 1 <= k <= K:
                continue
            limit = mj * (1.0 + gg * (k - 1))
            for g in np.flatnonzero(present[t]):
                c = cost(x[t, g], x[t0, h], min_joints)
                if c is None:
                    continue
                margins[t] = min(margins[t], abs(c - limit) / limit)
                if c <= limit:
                    cand.append((c, k, int(h), int(g), tr))
        cand.sort()
        for p, q in zip(cand, cand[1:]):
            margins[t] = min(margins[t], (q[0] - p[0]) / q[0] if q[0] > 0 else 0.0)
        used = set()
        for c, k, h, g, tr in cand:
            if out[t, g] < 0 and tr not in used:
                out[t, g] = tr
                link_cost[t, g] = c
                link_lag[t, g] = k
                used.add(tr)
        for g in np.flatnonzero(present[t]):
            if out[t, g] < 0:
                out[t, g] = n_tracks
                n_tracks += 1
            latest[int(out[t, g])] = (t, int(g))
    return {"track": out, "n_tracks": n_tracks, "link_cost": link_cost, "link_lag": link_lag, "margins": margins}
