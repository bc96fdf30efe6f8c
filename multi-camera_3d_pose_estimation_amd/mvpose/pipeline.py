"""Multi-view 2D -> 3D pipeline on one GPU: the reference's
estimate_pose_from_video / run_pose_est / get_pose_2D / get_pose_3D loop
(pose_estimation.py:157-327) for a whole batch of synchronised frames at once.

process(frames (T, V, H, W, 3) uint8 on GPU) returns, device-resident:
    kpts_2d     (T, 17, 3, V) float32   [x, y, score] per camera   (pose_estimation.py:135)
    heatmaps_2d (T, V, 17, 6) float64   [mx, my, vxx, vxy, vxy, vyy] (mmpose_pose_estimation.py:208-210)
    kpts_3d     (T, 17, 3)    float32   triangulated                 (pose_estimation.py:319-322)
With refine= (no reference counterpart) kpts_3d holds the maximum-likelihood refinement of the
triangulated points and kpts_3d_seed, kpts_3d_cov (T, 17, 3, 3), tri_refine_cost and
tri_refine_status come with it (ops.triangulate_refine).
With mode=ops.TRI_PEAKS (no reference counterpart) up to max_peaks modes of every heatmap are kept
(kpts_2d_peaks) and the triangulation chooses among them (kpts_2d_selected, tri_peak_sel).

process_people(frames, bboxes (T, V, P, 4)) is the same path for several people per camera (no
reference counterpart): the 2D stage per person box, ops.associate_views across the cameras, then
one kpts_2d / kpts_3d per group of skeletons that show the same person.  Group numbers are per
frame; people_trajectories(out) tracks the groups through time (ops.track_people) and returns one
trajectory per person.

process(..., overlap_moments=True) computes heatmaps_2d on a side stream beside the
next batch's backbone (triangulation reads only kpts_2d); call wait(out) before reading
heatmaps_2d on the current stream.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .estimator import BatchPoseEstimator
from .hrnet import N_JOINTS


class MultiViewPipeline:
    def __init__(self, camera_params, estimator: BatchPoseEstimator | None = None, camera_indices=(0, 1),
                 mode: int = ops.TRI_REFERENCE, device="cuda", detector=None, bbox_thr: float = 0.3,
                 tri_solver: str = "tolerance", inlier_px: float = 10.0, min_conf: float = 0.0,
                 refine: str | None = None, cov_floor: float = 1.0, max_peaks: int = 4, peak_thr: float = 0.1,
                 peak_min_rel: float = 0.3, peak_radius: int = 1, **estimator_kw):
        """camera_params: {camera key: [K, R, T, dist]} (utils.get_params_from_name order),
        keys 0..V-1 as the reference assumes (pose_estimation.py:276-280).
        detector: an mvpose.rtmdet.RTMDetector run on every camera-frame before the crops
        (PoseEstimator.predict, mmpose_pose_estimation.py:234-250: its first person box with
        score > bbox_thr, else the whole image), or None (whole-image crops).
        tri_solver: "tolerance" (default: MVP_TRI_TOLERANCE, <= 1e-4 world units against
        OpenCV's rounding sequence, bit-identical on almost every point) or "reference_compat"
        (OpenCV 4.9's fp64 rounding sequence, QR + inverse iteration with the Jacobi
        restatement where that has not converged).
        mode=ops.TRI_ROBUST: ops.triangulate_robust over camera_indices (outlier views rejected
        per point at inlier_px undistorted pixels, views below min_conf ignored); process() then
        also returns tri_inliers (T, 17, NV) bool and tri_reproj_err (T, 17, NV) float32.
        tri_solver does not apply in this mode.
        mode=ops.TRI_PEAKS: up to max_peaks modes of every heatmap (ops.heatmap_peaks with
        peak_thr, peak_min_rel, peak_radius) and ops.triangulate_peaks over camera_indices, which
        chooses one mode per inlier view; process() leaves kpts_2d untouched (the argmax) and also
        returns kpts_2d_peaks (T, 17, M, 3, V), kpts_2d_selected (T, 17, 3, V: kpts_2d with the
        inlier views' columns replaced by the chosen modes — the kpts_2d for every later stage),
        tri_inliers, tri_reproj_err and tri_peak_sel (T, 17, NV) int8.  refine "unit" / "conf" then
        run on kpts_2d_selected over the inliers; "heatmap" raises ValueError (the Gaussian moments
        are those of the whole, possibly bimodal map, not of the chosen mode).  tri_solver does
        not apply.  process_people is unchanged.
        refine: None (default: process() as without it) or "unit" / "conf" / "heatmap": the mode's
        points seed ops.triangulate_refine over camera_indices (TRI_ROBUST: over each point's
        inliers); "heatmap" weighs each view by its own heatmaps_2d Gaussian + cov_floor px².
        process() then returns the refined points as kpts_3d and also kpts_3d_seed, kpts_3d_cov
        (T, 17, 3, 3), tri_refine_cost (T, 17) and tri_refine_status (T, 17) uint8."""
        if refine not in (None, "unit", "conf", "heatmap"):
            raise ValueError(f"refine {refine!r}: None, 'unit', 'conf' or 'heatmap'")
        self.refine = refine
        self.cov_floor = float(cov_floor)
        if tri_solver not in ("tolerance", "reference_compat"):
            raise ValueError(f"tri_solver {tri_solver!r}: 'tolerance' or 'reference_compat'")
        if mode in (ops.TRI_ROBUST, ops.TRI_PEAKS) and tri_solver != "tolerance":
            raise ValueError("tri_solver does not apply to mode=ops.TRI_ROBUST / TRI_PEAKS: leave it at its default")
        if mode == ops.TRI_PEAKS:
            if refine == "heatmap":
                raise ValueError('refine="heatmap" does not apply to mode=ops.TRI_PEAKS: the heatmap moments describe '
                                 "the whole, possibly bimodal map, not the selected mode")
            if not 1 <= int(max_peaks) <= ops.MAX_PEAKS:
                raise ValueError(f"max_peaks={max_peaks}: 1..{ops.MAX_PEAKS}")
        self.peak_kw = {"max_peaks": int(max_peaks), "peak_thr": float(peak_thr), "peak_min_rel": float(peak_min_rel),
                        "peak_radius": int(peak_radius)}
        self.tri_solver = tri_solver
        self.inlier_px = float(inlier_px)
        self.min_conf = float(min_conf)
        self.detector = detector
        self.bbox_thr = bbox_thr
        self._best = None
        self.device = torch.device(device)
        self.n_views = len(camera_params)
        self.cams = torch.tensor(ops.pack_cameras(camera_params), device=self.device)
        self.camera_indices = list(camera_indices)
        self.mode = mode
        self.estimator = estimator or BatchPoseEstimator(device=device, **estimator_kw)

    @property
    def max_frames(self) -> int:
        return self.estimator.max_frames // self.n_views

    def process(self, frames: torch.Tensor, out: dict | None = None, overlap_moments: bool = False,
                bboxes=None) -> dict:
        """bboxes: None (the detector's boxes, or whole-image crops without one), host (T, V, 4)
        xyxy person boxes (NaN row = none), or device rows (T, V, >=4) f32 used as given."""
        T, V = frames.shape[:2]
        if V != self.n_views:
            raise ValueError(f"frames carry {V} views, pipeline has {self.n_views} cameras")
        flat = frames.reshape(T * V, *frames.shape[2:])
        if out is None:
            out = {}
        if "kpts_2d" not in out or tuple(out["kpts_2d"].shape) != (T, N_JOINTS, 3, V):
            out["kpts_2d"] = torch.empty((T, N_JOINTS, 3, V), dtype=torch.float32, device=self.device)
            out.pop("kpts_3d", None)
        thr = None
        if bboxes is None and self.detector is not None:
            bb, thr = self.detect(flat), self.bbox_thr       # device rows: no host round trip
        elif isinstance(bboxes, torch.Tensor) and bboxes.is_cuda:
            bb = bboxes.reshape(T * V, -1)
        else:
            bb = None if bboxes is None else np.asarray(bboxes, np.float64).reshape(T * V, 4)
        r = self.estimator.run(flat, n_views=V, kpts_tkv=out["kpts_2d"], overlap_moments=overlap_moments, bboxes=bb,
                               bbox_thr=thr, **(self.peak_kw if self.mode == ops.TRI_PEAKS else {}))
        out["heatmaps_2d"] = r["gaussians"].reshape(T, V, N_JOINTS, 6)
        if r["moments_done"] is not None:
            out["moments_done"] = r["moments_done"]
        else:
            out.pop("moments_done", None)
        if self.mode == ops.TRI_ROBUST:
            out["kpts_3d"], out["tri_inliers"], out["tri_reproj_err"] = ops.triangulate_robust(
                out["kpts_2d"], self.cams, self.camera_indices, inlier_px=self.inlier_px, min_conf=self.min_conf)
            return self._refine(out, out["tri_inliers"]) if self.refine is not None else out
        if self.mode == ops.TRI_PEAKS:
            out["kpts_2d_peaks"] = r["peaks"]
            (out["kpts_3d"], out["tri_inliers"], out["tri_peak_sel"], out["tri_reproj_err"],
             out["kpts_2d_selected"]) = ops.triangulate_peaks(r["peaks"], self.cams, self.camera_indices,
                                                              inlier_px=self.inlier_px, min_conf=self.min_conf)
            if self.refine is not None:
                return self._refine(out, out["tri_inliers"], kpts=out["kpts_2d_selected"])
            return out
        if self.refine is not None:
            out.pop("kpts_3d", None)       # the previous call's refined points are not a seed buffer
        out["kpts_3d"] = ops.triangulate(out["kpts_2d"], self.cams, self.camera_indices, mode=self.mode,
                                         out=out.get("kpts_3d"), tolerance=self.tri_solver == "tolerance")
        return self._refine(out, None) if self.refine is not None else out

    def _refine(self, out: dict, mask, kpts=None) -> dict:
        if self.refine == "heatmap":
            self.wait(out)                 # overlap_moments: the side stream's heatmaps_2d before they are read
        out["kpts_3d_seed"] = out["kpts_3d"]
        out["kpts_3d"], out["kpts_3d_cov"], out["tri_refine_cost"], out["tri_refine_status"] = ops.triangulate_refine(
            out["kpts_2d"] if kpts is None else kpts, self.cams, self.camera_indices, out["kpts_3d_seed"],
            weights=self.refine, gauss=out["heatmaps_2d"] if self.refine == "heatmap" else None, mask=mask,
            min_conf=self.min_conf if self.mode in (ops.TRI_ROBUST, ops.TRI_PEAKS) else 0.0,
            cov_floor=self.cov_floor)
        return out

    def detect(self, flat: torch.Tensor) -> torch.Tensor:
        """(T*V, H, W, 3) camera-frames -> the detector's per-frame best rows (T*V, 6) f32 on the
        device {x1, y1, x2, y2, score, prior}; BatchPoseEstimator.run applies score > bbox_thr
        and derives the crops there (mvp_bbox_geometry)."""
        n = flat.shape[0]
        if self._best is None or self._best.shape[0] < n:
            self._best = torch.empty((n, 6), dtype=torch.float32, device=self.device)
        mb = self.detector.max_batch
        for i in range(0, n, mb):
            self.detector.detect(flat[i:i + mb], best_out=self._best[i:min(n, i + mb)])
        return self._best[:n]

    def detect_people(self, flat: torch.Tensor, max_people: int) -> np.ndarray:
        """(T*V, H, W, 3) camera-frames -> host (T*V, max_people, 4) float64 xyxy: each frame's
        first max_people detections after NMS (score-descending) with score > bbox_thr, NaN rows
        for the slots left empty."""
        n = flat.shape[0]
        P = int(max_people)
        out = torch.empty((n, P, 4), dtype=torch.float32, device=self.device)
        slot = torch.arange(P, device=self.device)
        mb = self.detector.max_batch
        for i in range(0, n, mb):
            dets, counts = self.detector.nms_device(self.detector.detect(flat[i:i + mb]))
            top = dets[:, :P]
            if top.shape[1] < P:
                top = torch.cat([top, top.new_zeros((top.shape[0], P - top.shape[1], 5))], 1)
            ok = (slot[None, :] < counts[:, None]) & (top[..., 4] > self.bbox_thr)
            out[i:i + mb] = torch.where(ok[..., None], top[..., :4], top.new_full((), float("nan")))
        return out.cpu().numpy().astype(np.float64)

    def process_people(self, frames: torch.Tensor, bboxes=None, max_people: int = 4, max_groups: int | None = None,
                       **assoc_kw) -> dict:
        """Several people per camera (no reference counterpart): the 2D stage on every person box,
        ops.associate_views across camera_indices, then robust triangulation per group.

        frames (T, V, H, W, 3) uint8 on the GPU.  bboxes: host (T, V, P, 4) xyxy person boxes, NaN
        rows for empty slots; the slot order is free and independent per camera-frame.  None: the
        detector's first max_people detections after NMS with score > bbox_thr (P = max_people).
        The 2D stage runs on the non-empty (camera-frame, slot) rows only, in that order, in chunks
        of the estimator's max_frames.  max_groups: the groups kept per frame (default P).
        assoc_kw: trunc_px, max_cost_px, min_joints, min_conf of ops.associate_views (min_conf
        defaults to the pipeline's).  Returns, device-resident:
            kpts_2d_people     (T, P, 17, 3, V) float32   per slot, NaN for empty slots
            heatmaps_2d_people (T, V, P, 17, 6) float64   likewise
            people_group       (T, NV, P) int8            group of (view position, slot), -1 = none
            people_count       (T, 2) uint8               groups, groups seen by >= 2 views
            people_dropped     (T,) int64                 groups beyond max_groups, not returned
            kpts_2d            (T, G, 17, 3, V) float32   per group, NaN where a view has no member
            heatmaps_2d        (T, G, V, 17, 6) float64
            kpts_3d            (T, G, 17, 3) float32      ops.triangulate_robust over camera_indices
            tri_inliers        (T, G, 17, NV) bool, tri_reproj_err (T, G, 17, NV) float32
        and with refine= also kpts_3d_seed, kpts_3d_cov (T, G, 17, 3, 3), tri_refine_cost and
        tri_refine_status (T, G, 17), kpts_3d then holding the refined points (as process())."""
        from . import people
        T, V = frames.shape[:2]
        if V != self.n_views:
            raise ValueError(f"frames carry {V} views, pipeline has {self.n_views} cameras")
        flat = frames.reshape(T * V, *frames.shape[2:])
        if bboxes is None:
            if self.detector is None:
                raise ValueError("process_people needs person boxes: pass bboxes or build the pipeline with a detector")
            boxes = self.detect_people(flat, max_people)
        else:
            boxes = np.asarray(bboxes.cpu() if isinstance(bboxes, torch.Tensor) else bboxes, dtype=np.float64)
            if boxes.ndim != 4 or boxes.shape[:2] != (T, V) or boxes.shape[3] != 4 or boxes.shape[2] < 1:
                raise ValueError(f"bboxes must be (T, V, P, 4) = ({T}, {V}, P, 4), got {boxes.shape}")
        P = boxes.shape[-2]
        boxes = boxes.reshape(T * V, P, 4)
        row_f, row_p = np.nonzero(np.isfinite(boxes).all(-1))       # (camera-frame, slot) order
        kp = torch.full((T * V, P, N_JOINTS, 3), float("nan"), dtype=torch.float32, device=self.device)
        gauss = torch.full((T * V, P, N_JOINTS, 6), float("nan"), dtype=torch.float64, device=self.device)
        step = self.estimator.max_frames
        for i in range(0, len(row_f), step):
            f = torch.as_tensor(row_f[i:i + step], device=self.device)
            p = torch.as_tensor(row_p[i:i + step], device=self.device)
            r = self.estimator.run(flat.index_select(0, f), bboxes=boxes[row_f[i:i + step], row_p[i:i + step]])
            kp[f, p] = torch.cat([r["keypoints"], r["scores"][..., None]], -1)
            gauss[f, p] = r["gaussians"]
        out = {"kpts_2d_people": kp.reshape(T, V, P, N_JOINTS, 3).permute(0, 2, 3, 4, 1).contiguous(),
               "heatmaps_2d_people": gauss.reshape(T, V, P, N_JOINTS, 6)}
        assoc_kw.setdefault("min_conf", self.min_conf)
        out["people_group"], out["people_count"], _, _ = ops.associate_views(
            out["kpts_2d_people"], self.cams, self.camera_indices, **assoc_kw)
        G = P if max_groups is None else int(max_groups)
        out["kpts_2d"], out["heatmaps_2d"], out["people_dropped"] = people.gather_groups(
            out["kpts_2d_people"], out["people_group"], self.camera_indices, G, gauss=out["heatmaps_2d_people"])
        out["kpts_3d"], out["tri_inliers"], out["tri_reproj_err"] = ops.triangulate_robust(
            out["kpts_2d"], self.cams, self.camera_indices, inlier_px=self.inlier_px, min_conf=self.min_conf)
        if self.refine is not None:
            # triangulate_refine takes the heatmap Gaussians per (frame, view, joint): groups fold into frames
            nv = len(self.camera_indices)
            out["kpts_3d_seed"] = out["kpts_3d"]
            xyz, cov, cost, status = ops.triangulate_refine(
                out["kpts_2d"].reshape(T * G, N_JOINTS, 3, V), self.cams, self.camera_indices,
                out["kpts_3d_seed"].reshape(T * G, N_JOINTS, 3), weights=self.refine,
                gauss=out["heatmaps_2d"].reshape(T * G, V, N_JOINTS, 6) if self.refine == "heatmap" else None,
                mask=out["tri_inliers"].reshape(T * G, N_JOINTS, nv), min_conf=self.min_conf, cov_floor=self.cov_floor)
            out["kpts_3d"] = xyz.reshape(T, G, N_JOINTS, 3)
            out["kpts_3d_cov"] = cov.reshape(T, G, N_JOINTS, 3, 3)
            out["tri_refine_cost"] = cost.reshape(T, G, N_JOINTS)
            out["tri_refine_status"] = status.reshape(T, G, N_JOINTS)
        return out

    @staticmethod
    def people_trajectories(out: dict, min_len: int = 1, max_people: int | None = None, with_2d: bool = False,
                            **track_kw) -> dict:
        """One trajectory per person from a process_people result, or from the concatenation along
        time of several chunks' results (group numbers are per frame; this is what gives a person
        one number through the recording).  people.track_people on kpts_3d (track_kw: max_gap,
        max_jump, gap_growth, min_joints), then people.person_trajectories (min_len, max_people).
        Returns, device-resident, people ordered by (-frames present, track number):
            kpts_3d_person   (T, Np, 17, 3) float32   NaN where the person is absent
            person_present   (T, Np) bool
            person_track     (Np,) int64              the tracker's number of each person
        and, when out carries them (refine=), kpts_3d_cov_person (T, Np, 17, 3, 3) and
        tri_refine_status_person (T, Np, 17) uint8 (0 where absent; the NaN points mark those
        frames).  refine.smooth_trajectory takes person p as kpts_3d_person[:, p],
        cov=kpts_3d_cov_person[:, p], status=tri_refine_status_person[:, p], and fills the frames
        the person was not seen in.
        with_2d=True also gathers what refine.fit_trajectory reads: kpts_2d_person
        (T, Np, 17, 3, V), heatmaps_2d_person (T, Np, V, 17, 6) and tri_inliers_person
        (T, Np, 17, NV) bool (its mask), NaN / False where the person is absent."""
        from . import people
        xyz = out["kpts_3d"]
        if xyz.dim() != 4 or xyz.shape[3] != 3:
            raise ValueError(f"out['kpts_3d'] must be (T, G, J, 3) as process_people returns it, got {tuple(xyz.shape)}")
        track, _ = people.track_people(xyz.contiguous(), **track_kw)
        names = ("kpts_3d", "kpts_3d_cov", "tri_refine_status")
        if with_2d:
            names += ("kpts_2d", "heatmaps_2d", "tri_inliers")
        arrays = {k: out[k] for k in names if k in out}
        got, present, chosen = people.person_trajectories(track, arrays, min_len=min_len, max_people=max_people)
        res = {k + "_person": v for k, v in got.items()}
        res["person_present"] = present
        res["person_track"] = chosen
        return res

    @staticmethod
    def wait(out: dict) -> None:
        """Order the current stream after an overlapped process()'s heatmaps_2d."""
        BatchPoseEstimator.wait_moments(out)

    def process_stream(self, frames: torch.Tensor, bboxes=None) -> dict:
        """Arbitrary-length sequence (T, V, H, W, 3): chunked to the estimator's batch."""
        T = frames.shape[0]
        step = self.max_frames
        parts = [self.process(frames[t:t + step], bboxes=None if bboxes is None else bboxes[t:t + step])
                 for t in range(0, T, step)]
        return {k: torch.cat([p[k] for p in parts]) for k in parts[0]}
