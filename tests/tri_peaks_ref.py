"""Numpy restatement of mvp_triangulate_peaks (include/mvpose.h) from the oracle's leaves: the
Reference of tests/test_triangulate_robust_gpu.py (OpenCV-semantics undistortion and Jacobi-SVD
DLT from oracle/cv_ref for every solve that reaches the output) extended to several candidates
per view.  The pair hypotheses, which only select, come from np.linalg.svd.

Masks and selections rest on comparisons of fp64 errors that the device evaluates in another
order (~1e-9 px apart), so the reference records the two margins that decide whether those
comparisons are determined whatever the rounding:
    margin  the smallest |error - inlier_px| it ever compared (as the robust Reference), and
    gap     the smallest difference between a view's best and second-best candidate error.
Both are conditions of the INPUT (tests/tri_peaks_cases.py is checked on the CPU to keep them
above MIN_MARGIN), not tolerances on the device."""
import numpy as np

from oracle import cv_ref
from test_triangulate_robust_gpu import INLIER_PX, MIN_MARGIN, Reference  # noqa: F401


class PeaksReference(Reference):
    """Steps A and B over the listed views `ci` of peaks (..., M, 3, V) float32."""

    def __init__(self, cams, ci):
        super().__init__(cams, ci)
        self.gap = np.inf             # smallest best-to-second-best candidate error difference

    def _cand_errors(self, X, und):
        """fp64 reprojection error of every candidate und (NV, M, 2) against homogeneous
        X (..., 4): (..., NV, M), +inf behind the camera (validity is the caller's)."""
        X = np.asarray(X, np.float64)[..., None, :]                      # (..., 1, 4)
        q = [sum(self.P[:, c, k] * X[..., k] for k in range(4)) for c in range(3)]       # (..., NV) each
        with np.errstate(all="ignore"):
            front = (q[2] * X[..., 3]) > 0
            dx = (q[0] / q[2])[..., None] - und[..., 0].astype(np.float64)
            dy = (q[1] / q[2])[..., None] - und[..., 1].astype(np.float64)
            return np.where(front[..., None], np.sqrt(dx * dx + dy * dy), np.inf)

    def _nearest(self, E, cval, top, record=True):
        """Per view the valid candidate with the smallest error, ties to the lower slot:
        (error (..., NV) (+inf where every valid one is behind the camera), slot (..., NV))."""
        Ev = np.where(cval, E, np.inf)
        slot = np.argmin(Ev, -1)                                         # first of equal minima
        slot = np.where(np.take_along_axis(np.broadcast_to(cval, Ev.shape), slot[..., None], -1)[..., 0], slot, top)
        best = np.take_along_axis(Ev, slot[..., None], -1)[..., 0]
        if record and Ev.shape[-1] > 1:
            s = np.sort(Ev, -1)
            fin = np.isfinite(s[..., 1])
            if fin.any():
                self.gap = min(self.gap, float(np.min(s[..., 1][fin] - s[..., 0][fin])))
        return best, slot

    def _within(self, e, valid, inl):
        """valid & (e <= inl) for any leading shape, recording the margin."""
        fin = np.isfinite(e) & valid
        if fin.any():
            self.margin = min(self.margin, float(np.min(np.abs(e[fin] - inl))))
        return valid & (e <= inl)

    def __call__(self, peaks, inlier_px=INLIER_PX, min_conf=0.0):
        peaks = np.asarray(peaks, np.float32)
        lead, M = peaks.shape[:-3], peaks.shape[-3]
        k = peaks.reshape(-1, M, 3, peaks.shape[-1])[..., self.ci]       # (n, M, 3, NV)
        n, nv = k.shape[0], len(self.ci)
        und = np.empty((n, nv, M, 2), np.float32)
        for v, c in enumerate(self.cams):
            pts = np.ascontiguousarray(k[:, :, :2, v].reshape(n * M, 1, 2))
            und[:, v] = cv_ref.undistort_points(pts, c["K"], c["dist"], None, c["K"])[:, 0, :].reshape(n, M, 2)
        x, y, s = (np.moveaxis(k[:, :, c, :], 1, 2) for c in range(3))   # (n, NV, M)
        with np.errstate(invalid="ignore"):
            cval = np.isfinite(x) & np.isfinite(y) & ~np.isnan(s) & (s >= np.float32(min_conf)) & np.isfinite(und).all(-1)
        valid = cval.any(-1)
        top = np.argmax(cval, -1)                                        # lowest valid slot
        xyz = np.full((n, 3), np.nan, np.float32)
        mask = np.zeros((n, nv), bool)
        sel = np.full((n, nv), -1, np.int8)
        err = np.full((n, nv), np.nan, np.float32)
        inl = float(np.float32(inlier_px))
        ar = np.arange(nv)
        for p in range(n):
            vd = valid[p]
            views = list(np.flatnonzero(vd))
            if len(views) < 2:
                continue
            # step A: the top candidates
            ut = und[p, ar, top[p]]
            pt = self._dlt(ut, views)
            e = self._cand_errors(np.array([pt[0], pt[1], pt[2], 1.0]), ut[:, None, :])[:, 0]
            if self._within(e, vd, inl)[vd].all():
                xyz[p], mask[p] = pt, vd
                sel[p] = np.where(vd, top[p], -1)
                err[p] = np.where(vd, e, np.nan).astype(np.float32)
                continue
            # step B: every (a, b, ma, mb) in lexicographic order, solved and scored as one batch
            rows = []
            for ia, a in enumerate(views):
                for b in views[ia + 1:]:
                    for ma in np.flatnonzero(cval[p, a]):
                        for mb in np.flatnonzero(cval[p, b]):
                            r = []
                            for v, m in ((a, ma), (b, mb)):
                                ux, uy = np.float64(und[p, v, m, 0]), np.float64(und[p, v, m, 1])
                                r += [ux * self.P[v][2] - self.P[v][0], uy * self.P[v][2] - self.P[v][1]]
                            rows.append(np.stack(r))
            X = np.linalg.svd(np.stack(rows))[2][:, 3, :]                # (Hn, 4)
            be, bs = self._nearest(self._cand_errors(X, und[p]), cval[p], top[p])        # (Hn, NV)
            m = self._within(be, vd[None, :], inl)
            ssum = np.zeros(len(X), np.float32)
            for v in range(nv):                                          # f32, ascending view position
                ssum = np.where(m[:, v], (ssum + s[p, v, bs[:, v]]).astype(np.float32), ssum)
            cnt = m.sum(-1)
            cand = np.flatnonzero(cnt == cnt.max())
            h = cand[np.flatnonzero(ssum[cand] == ssum[cand].max())[0]]  # most inliers, larger sum, first
            if cnt[h] < 2:
                continue
            bm, slots = m[h], np.where(m[h], bs[h], 0)
            us = und[p, ar, slots]
            pt = self._dlt(us, list(np.flatnonzero(bm)))
            Xf = np.array([pt[0], pt[1], pt[2], 1.0])
            e_sel = self._cand_errors(Xf, us[:, None, :])[:, 0]
            e_near, _ = self._nearest(self._cand_errors(Xf, und[p]), cval[p], top[p], record=False)
            xyz[p], mask[p] = pt, bm
            sel[p] = np.where(bm, slots, -1)
            err[p] = np.where(vd, np.where(bm, e_sel, e_near), np.nan).astype(np.float32)
        return (xyz.reshape(lead + (3,)), mask.reshape(lead + (nv,)), sel.reshape(lead + (nv,)),
                err.reshape(lead + (nv,)))

    def select(self, peaks, mask, sel):
        """out_kpts: slot 0, the masked views' columns replaced by their selected candidates."""
        peaks = np.asarray(peaks, np.float32)
        out = peaks[..., 0, :, :].copy()
        for i, col in enumerate(self.ci):
            chosen = np.take_along_axis(peaks[..., col], np.maximum(sel[..., i], 0)[..., None, None].astype(np.int64),
                                        -2)[..., 0, :]                    # (..., 3)
            out[..., col] = np.where(mask[..., i, None], chosen, out[..., col])
        return out
