"""fp64 numpy restatement of cross-view association, written from include/mvpose.h ("Cross-view
association of 2D skeletons"), not from the kernel.  The ideal pixels, F and the Sampson distance
are sync_ref's.

* ``affinity``: c(n, m) of every node pair of different views, -1 where undefined, and which nodes
  are usable.
* ``group_frame``: complete-linkage agglomeration of one frame, each link evaluated from its
  definition (the maximum over the clusters' cross pairs of the original affinities), with the
  smallest relative margin of any comparison it made.
* ``associate``: both, for all frames.
"""
import numpy as np

import sync_ref


def thresholds(trunc_px, max_cost_px):
    """The C-ABI takes both as float32 and squares them in fp64."""
    return float(np.float32(trunc_px)) ** 2, float(np.float32(max_cost_px)) ** 2


def affinity(kpts, cams, cam_idx, min_conf=0.0, trunc_px=20.0, min_joints=5):
    """kpts (T, P, J, 3, V) -> (aff (T, NP, P, P) float64, usable (T, NV, P) bool, pairs)."""
    kpts = np.asarray(kpts, np.float32)
    T, P, J = kpts.shape[:3]
    nv = len(cam_idx)
    # (NV, T, P, J, 3)
    x = np.stack([sync_ref.ideal_points(kpts[:, p], cams, list(cam_idx), min_conf) for p in range(P)], axis=2)
    usable = (~np.isnan(x[..., 2])).sum(-1) >= min_joints                  # (NV, T, P)
    pairs = [(a, b) for a in range(nv) for b in range(a + 1, nv)]
    tau2 = float(np.float32(trunc_px)) ** 2
    aff = np.full((T, len(pairs), P, P), -1.0)
    for k, (a, b) in enumerate(pairs):
        F = sync_ref.fundamental(cams[cam_idx[a]], cams[cam_idx[b]])
        d2 = sync_ref.sampson2(F, x[a][:, :, None], x[b][:, None, :])      # (T, P, P, J)
        ok = np.isfinite(d2)
        cnt = ok.sum(-1)
        s = np.where(ok, np.minimum(np.where(ok, d2, 0.0), tau2), 0.0).sum(-1)
        aff[:, k] = np.where(cnt >= min_joints, s / np.maximum(cnt, 1), -1.0)
    return aff, np.transpose(usable, (1, 0, 2)), pairs


def group_frame(aff, usable, pairs, thr2):
    """aff (NP, P, P), usable (NV, P) of one frame -> (group (NV, P) int8, count (2,) uint8,
    margin): margin is the smallest relative distance of any comparison made, a link against thr2
    (|l - thr2| / thr2) or the best candidate against the second best ((l2 - l1) / l2)."""
    nv, P = usable.shape
    N = nv * P
    A = np.full((N, N), -1.0)
    for k, (a, b) in enumerate(pairs):
        A[a * P:(a + 1) * P, b * P:(b + 1) * P] = aff[k]
        A[b * P:(b + 1) * P, a * P:(a + 1) * P] = aff[k].T
    members = {n: [n] for n in range(N) if usable[n // P, n % P]}           # keyed by the smallest node
    views = {n: {n // P} for n in members}

    def link(i, j):
        c = A[np.ix_(members[i], members[j])]
        c = c[c >= 0]
        return c.max() if c.size else -1.0

    L = {(i, j): link(i, j) for i in members for j in members if i < j}
    margin = np.inf
    while True:
        cands = []
        for (i, j), l in L.items():
            if views[i] & views[j] or l < 0:
                continue
            margin = min(margin, abs(l - thr2) / thr2)
            if l <= thr2:
                cands.append((l, i, j))
        if not cands:
            break
        cands.sort()
        if len(cands) > 1:
            margin = min(margin, (cands[1][0] - cands[0][0]) / cands[1][0] if cands[1][0] > 0 else 0.0)
        _, i, j = cands[0]
        members[i] += members.pop(j)
        views[i] |= views.pop(j)
        L = {k: v for k, v in L.items() if j not in k}
        for k in members:
            if k != i:
                L[(min(i, k), max(i, k))] = link(min(i, k), max(i, k))
    order = sorted(members, key=lambda n: (-len(views[n]), n))
    group = np.full(N, -1, np.int8)
    for g, n in enumerate(order):
        group[members[n]] = g
    count = np.array([len(order), sum(len(views[n]) >= 2 for n in order)], np.uint8)
    return group.reshape(nv, P), count, margin


def associate(kpts, cams, cam_idx, min_conf=0.0, trunc_px=20.0, max_cost_px=8.0, min_joints=5):
    """-> dict(group (T, NV, P) int8, count (T, 2) uint8, affinity (T, NP, P, P), pairs,
    margins (T,) float64: each frame's smallest comparison margin, inf where none was made)."""
    aff, usable, pairs = affinity(kpts, cams, cam_idx, min_conf, trunc_px, min_joints)
    _, thr2 = thresholds(trunc_px, max_cost_px)
    T = aff.shape[0]
    group = np.empty(usable.shape, np.int8)
    count = np.empty((T, 2), np.uint8)
    margins = np.empty(T)
    for t in range(T):
        group[t], count[t], margins[t] = group_frame(aff[t], usable[t], pairs, thr2)
    return {"group": group, "count": count, "affinity": aff, "pairs": pairs, "margins": margins}
