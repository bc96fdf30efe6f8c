"""Numpy reference of mvp_heatmap_peaks (the peak definition of include/mvpose.h) on
oracle.heatmap_ref's decode arithmetic, and the maps the CPU and GPU tests share."""
import numpy as np

from oracle import heatmap_ref

INPUT_SIZE = (192, 256)      # network input (w, h)
# (N, K, H, W, V): the 16-B staging path with a ragged last workgroup (51 maps); fewer cells than
# lanes; one cell; W no multiple of 4 (HW = 650: scalar staging); three views
SHAPES = [(3, 17, 64, 48, 1), (2, 3, 9, 7, 1), (1, 1, 1, 1, 1), (2, 2, 5, 130, 1), (6, 2, 12, 8, 3)]
THR = 0.1


def decode_cell(hm, i, v, center, scale, input_size=INPUT_SIZE):
    """Cell i (value v) of the (H, W) map as MSRAHeatmap.decode treats its argmax
    (heatmap_ref.msra_decode, for any input size), restored by heatmap_ref.keypoints_to_image."""
    H, W = hm.shape
    k = np.array([i % W, i // W], np.float32)
    if v <= 0.0:
        k[:] = -1
    px, py = int(k[0]), int(k[1])
    if 1 < px < W - 1 and 1 < py < H - 1:
        with np.errstate(invalid="ignore"):
            diff = np.array([hm[py][px + 1] - hm[py][px - 1], hm[py + 1][px] - hm[py - 1][px]])
        k += np.sign(diff) * 0.25
    scale_factor = np.array([input_size[0] / W, input_size[1] / H], np.float32)
    return heatmap_ref.keypoints_to_image((k * scale_factor).astype(np.float32), center, scale, input_size)


def find_peaks(hm, radius, thr):
    """Flat indices of the (H, W) map's peaks, best first (descending value, ties ascending index)."""
    H, W = hm.shape
    idx = np.arange(H * W).reshape(H, W)
    with np.errstate(invalid="ignore"):
        ok = ~np.isnan(hm) & (hm > np.float32(thr))
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                if dy == 0 and dx == 0:
                    continue
                u = np.full((H, W), np.nan, np.float32)       # out of bounds: no constraint, like a NaN
                n = np.zeros((H, W), np.int64)
                ys, yd = slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0))
                xs, xd = slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0))
                u[yd, xd] = hm[ys, xs]
                n[yd, xd] = idx[ys, xs]
                ok &= np.isnan(u) | (hm > u) | ((hm == u) & (idx < n))
    cells = np.flatnonzero(ok)
    vals = hm.reshape(-1)[cells]
    return cells[np.lexsort((cells, -vals.astype(np.float64)))]


class PeakReference:
    """peaks (N/V, K, M, 3, V) float32 and counts (N/V, K, V) int32 of hm (N, K, H, W); the peak
    lists are kept per (radius, thr), so the filters are applied to one detection."""

    def __init__(self, hm, center_scale, input_size=INPUT_SIZE):
        self.hm = np.asarray(hm, np.float32)
        self.cs = np.asarray(center_scale, np.float32)
        self.input_size = input_size
        self._found = {}

    def __call__(self, max_peaks, radius, thr, min_rel, V=1):
        N, K, H, W = self.hm.shape
        key = (radius, float(np.float32(thr)))
        if key not in self._found:
            self._found[key] = [[find_peaks(self.hm[n, k], radius, thr) for k in range(K)] for n in range(N)]
        peaks = np.zeros((N // V, K, max_peaks, 3, V), np.float32)
        peaks[:, :, :, :2] = np.nan
        counts = np.zeros((N // V, K, V), np.int32)
        for n in range(N):
            t, v = divmod(n, V)
            for k in range(K):
                m, flat = self.hm[n, k], self.hm[n, k].reshape(-1)
                cells = self._found[key][n][k]
                if len(cells):
                    floor = np.float32(min_rel) * flat[cells[0]]       # f32 product
                    keep = [c for r, c in enumerate(cells) if r == 0 or flat[c] >= floor][:max_peaks]
                else:
                    keep = []
                counts[t, k, v] = len(keep)
                for r, c in enumerate(keep):
                    peaks[t, k, r, :2, v] = decode_cell(m, int(c), flat[c], self.cs[n, :2], self.cs[n, 2:],
                                                        self.input_size)
                    peaks[t, k, r, 2, v] = flat[c]
        return peaks, counts


def _blob(H, W, cx, cy, amp, sigma):
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float32)
    return (np.float32(amp) * np.exp(-((xs - cx) ** 2 + (ys - cy) ** 2) / np.float32(2 * sigma * sigma))).astype(np.float32)


def make_maps(N, K, H, W, seed):
    """(hm (N, K, H, W) float32, center_scale (N, 4) float32, nan_free (N, K) bool).  Map q = n*K + k
    has content q % 6:
      0  1-6 Gaussian blobs of distinct amplitude, the first ones on a corner and an edge
      1  two blobs of EQUAL amplitude (exact ties) and a constant plateau
      2  6 blobs: more peaks than max_peaks
      3  nothing above THR
      4  a NaN cell beside a peak
      5  a NaN cell at a would-be peak
    over a background of small noise (many local maxima below THR)."""
    rng = np.random.default_rng(seed)
    hm = np.empty((N, K, H, W), np.float32)
    nan_free = np.ones((N, K), bool)
    for q in range(N * K):
        n, k = divmod(q, K)
        kind = q % 6
        m = rng.uniform(0.0, 0.02, (H, W)).astype(np.float32)
        nb = {0: int(rng.integers(1, 7)), 1: 2, 2: 6, 3: 2, 4: 2, 5: 2}[kind]
        amps = np.linspace(0.95, 0.15, 6)[:nb] + rng.uniform(0, 0.05, nb)
        cx = rng.integers(0, W, nb)
        cy = rng.integers(0, H, nb)
        if kind == 0:
            cx[0], cy[0] = (0, 0) if q % 12 == 0 else (W - 1, H - 1)
            if nb > 1:
                cx[1], cy[1] = W // 2, 0
        if kind == 1:
            amps[:] = 0.75
        for b in range(nb):
            m = np.maximum(m, _blob(H, W, cx[b], cy[b], amps[b], 1.5))
        if kind == 1:
            y0, x0 = int(rng.integers(0, max(H - 1, 1))), int(rng.integers(0, max(W - 2, 1)))
            m[y0:y0 + 2, x0:x0 + 3] = np.float32(0.5)
        if kind == 3:
            m *= np.float32(0.09)
        if kind in (4, 5):
            dx = 0 if kind == 5 or W == 1 else (1 if cx[0] + 1 < W else -1)
            m[cy[0], cx[0] + dx] = np.nan
            nan_free[n, k] = False
        hm[n, k] = m
    cs = np.empty((N, 4), np.float32)
    cs[:, 0] = rng.uniform(500, 800, N)
    cs[:, 1] = rng.uniform(300, 420, N)
    cs[:, 2] = rng.uniform(300, 1500, N)
    cs[:, 3] = cs[:, 2] * np.float32(4.0 / 3.0)
    return hm, cs, nan_free
