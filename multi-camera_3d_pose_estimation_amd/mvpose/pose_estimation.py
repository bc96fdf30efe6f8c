"""GPU mirror of the reference's pose_estimation.py module surface.

* ``get_pose_3D(camera_params, all_kpts_2d, world_trans_rot=None, camera_indices=None,
  ignore_nonlinear_distortions=False)`` (pose_estimation.py:11-65): one batched
  ``mvp_triangulate`` launch instead of T·J ``utils.triangulate_points`` calls;
  same selection quirks, float32 output, optional inv(R_W0) rotation.
* ``get_pose_2D(frames, model, confidence=0.5, pose_keypoints=range(17))`` (:71-151):
  the V cameras' frames of one time step -> ((17, 3, V) f32 [x, y, score], list of V
  (17, 6) heatmap Gaussians); with a GPU estimator the V frames are one batched run.
* ``load_frames(recording_paths, start_end_frames)`` (utils.py:849-909): decoded
  frame stacks, one per camera, sliced ``[start:end]`` (the default ``[0, -1]``
  drops the last frame, quirk F4).  A recording is a ``.npy`` (T, H, W, 3) uint8
  array of frames as a video decoder (BGR) returns them, an MJPEG / uncompressed AVI
  or a directory of frame<N>.jpg files (``mvpose.video``).
* ``run_pose_est`` (:157-244) and ``estimate_pose_from_video`` (:259-327): every
  frame of every camera through the batched GPU pipeline (RTMDet-m person box ->
  crop, HRNet-W32 with flip test, decode, heatmap moments), then get_pose_3D over
  ``camera_indices=[0, 1]`` as the reference hard-codes (:319).  A model name builds
  PoseEstimator(detector, pose model) from model_yaml exactly as :290-297 does.
"""
from __future__ import annotations

import os

import numpy as np
import torch
import yaml

from . import geometry, ops
from . import swaps as label_swaps
from . import sync as frame_sync
from .estimator import BatchPoseEstimator
from .hrnet import N_JOINTS


TRIANGULATION_METHODS = ("reference", "all_views", "robust", "peaks")
REFINE_MODES = (None, "unit", "conf", "heatmap")
SYNC_MODES = (None, "pose")


def _check_refine(refine):
    if refine not in REFINE_MODES:
        raise ValueError(f"refine {refine!r}: one of {REFINE_MODES}")


def get_pose_3D(camera_params, all_kpts_2d, world_trans_rot=None, camera_indices=None,
                ignore_nonlinear_distortions=False, device=None, method="reference", inlier_px=10.0,
                min_conf=0.0, return_info=False, refine=None, heatmaps_2d=None, cov_floor=1.0, peaks=None):
    """camera_params {key: [K, R, T, dist]} (get_params_from_name order), all_kpts_2d
    (T, J, 3, V) -> (T, J, 3) float32 numpy (float64 if world_trans_rot is given).

    method: "reference" (default: the reference's rule, the two highest-confidence listed
    cameras, parameters keyed by selection position), "all_views" (one DLT over every listed
    camera, each with its own parameters) or "robust" (ops.triangulate_robust: all listed
    cameras with per-point outlier-view rejection at inlier_px undistorted pixels, views below
    min_conf ignored).  return_info: also return {"inliers": (T, J, NV) bool — the listed
    views that entered each point's solve (None for "reference": the selection is internal),
    "reproj_err": (T, J, NV) float32 (methods "robust" and "peaks", else None)}.
    method "peaks" (ops.triangulate_peaks) reads peaks (T, J, M, 3, V), the modes of every heatmap
    (get_pose_2D / run_pose_est with max_peaks), instead of all_kpts_2d and chooses one per inlier
    view; info then also holds "sel" (T, J, NV) int8, the slot each inlier view used, and
    "kpts_selected" (T, J, 3, V), slot 0 with the inlier views' columns replaced by the chosen
    modes.  refine then runs on kpts_selected over the inliers ("heatmap" raises ValueError: the
    Gaussians describe the whole map, not the chosen mode).

    refine: None (default) or "unit" / "conf" / "heatmap": the chosen method's points seed
    ops.triangulate_refine (maximum-likelihood refinement over the listed cameras, for "robust"
    over each point's inlier views; "heatmap" weighs every view by its own Gaussian of
    heatmaps_2d (T, V, J, 6), with cov_floor px² added to the variances), and the refined points
    are returned.  info then also holds "cov" (T, J, 3, 3) float32 (rotated with the points when
    world_trans_rot is given), "refine_cost" (T, J), "refine_status" (T, J) uint8 and "seed"
    (T, J, 3), the method's own points."""
    if method not in TRIANGULATION_METHODS:
        raise ValueError(f"method {method!r}: one of {TRIANGULATION_METHODS}")
    _check_refine(refine)
    if method == "peaks":
        if peaks is None:
            raise ValueError('method="peaks" needs peaks, the (T, J, M, 3, V) heatmap modes')
        if refine == "heatmap":
            raise ValueError('refine="heatmap" does not apply to method="peaks": the heatmap Gaussians describe the '
                             "whole map, not the selected mode")
    if refine == "heatmap" and heatmaps_2d is None:
        raise ValueError('refine="heatmap" needs heatmaps_2d, the (T, V, J, 6) heatmap Gaussians')
    dev = torch.device(device if device is not None else "cuda")
    keys = list(camera_params.keys())
    params = {}
    for k in keys:
        K, R, T, dist = camera_params[k]
        params[k] = [K, R, T, np.asarray(dist) * 0 if ignore_nonlinear_distortions else dist]
    if camera_indices is None:
        camera_indices = keys
    positions = [keys.index(c) for c in camera_indices]
    kp = torch.as_tensor(np.ascontiguousarray(np.asarray(all_kpts_2d, dtype=np.float32)), device=dev)
    cams = torch.tensor(ops.pack_cameras(params), device=dev)
    info = {"inliers": None, "reproj_err": None}
    seed_dev = mask_dev = None
    if method == "robust":
        xyz, inliers, err = ops.triangulate_robust(kp, cams, positions, inlier_px=inlier_px, min_conf=min_conf,
                                                   return_err=return_info)
        seed_dev, mask_dev = xyz, inliers
        out = xyz.cpu().numpy()
        info["inliers"] = inliers.cpu().numpy()
        info["reproj_err"] = err.cpu().numpy() if err is not None else None
    elif method == "peaks":
        pk = torch.as_tensor(np.ascontiguousarray(np.asarray(peaks, dtype=np.float32)), device=dev)
        xyz, inliers, sel, err, kp = ops.triangulate_peaks(pk, cams, positions, inlier_px=inlier_px, min_conf=min_conf)
        seed_dev, mask_dev = xyz, inliers
        out = xyz.cpu().numpy()
        info.update({"inliers": inliers.cpu().numpy(), "reproj_err": err.cpu().numpy(), "sel": sel.cpu().numpy(),
                     "kpts_selected": kp.cpu().numpy()})
    elif method == "all_views":
        seed_dev = ops.triangulate(kp, cams, positions, mode=ops.TRI_ALL_VIEWS)
        out = seed_dev.cpu().numpy()
        info["inliers"] = np.ones(out.shape[:-1] + (len(positions),), dtype=bool)
    else:
        seed_dev = ops.triangulate(kp, cams, positions, mode=ops.TRI_REFERENCE)
        out = seed_dev.cpu().numpy()
    if refine is not None:
        gauss = None
        if refine == "heatmap":
            gauss = torch.as_tensor(np.ascontiguousarray(np.asarray(heatmaps_2d, dtype=np.float64)), device=dev)
        xyz, cov, cost, status = ops.triangulate_refine(
            kp, cams, positions, seed_dev, weights=refine, gauss=gauss, mask=mask_dev,
            min_conf=min_conf if method in ("robust", "peaks") else 0.0, cov_floor=cov_floor)
        info.update({"seed": out, "cov": cov.cpu().numpy(), "refine_cost": cost.cpu().numpy(),
                     "refine_status": status.cpu().numpy()})
        out = xyz.cpu().numpy()
    if world_trans_rot is not None:
        R_W0, _ = world_trans_rot
        Ri = np.linalg.inv(R_W0)
        out = np.einsum("ij,tpj->tpi", Ri, out)
        if refine is not None:
            info["seed"] = np.einsum("ij,tpj->tpi", Ri, info["seed"])
            info["cov"] = np.einsum("ij,tpjk,lk->tpil", Ri, info["cov"], Ri)
    return (out, info) if return_info else out


def get_pose_2D(frames, model, confidence=0.5, pose_keypoints=range(17), max_peaks=0, peak_thr=0.1,
                peak_min_rel=0.3, peak_radius=1):
    """pose_estimation.py:71-151.  frames: V frames (H, W, 3) uint8 of one time step.

    model: a BatchPoseEstimator / mvpose PoseEstimator or one's bound predict (the V frames
    go through the GPU in ONE batched run, detector included), or any per-frame callable with the reference's contract
    (model(frame) -> (pred_instances, heatmaps); an onepose-style model's dict output
    with 'points' / 'confidence' is parsed as the reference does, :99-101).
    Returns (results_stacked (17, 3, V) float32, heatmaps list of V arrays).
    confidence and pose_keypoints select only the keypoints the reference DRAWS on the
    frames (:117-131, then discarded with the GUI window), so they do not change the
    output — as in the reference.
    max_peaks > 0 (a GPU estimator only): a third result, peaks (17, max_peaks, 3, V) float32, the
    modes of every heatmap (ops.heatmap_peaks with peak_thr, peak_min_rel, peak_radius)."""
    est = resolve_estimator(model)
    if max_peaks and est is None:
        raise ValueError("max_peaks needs a BatchPoseEstimator / PoseEstimator: a per-frame callable returns no heatmaps")
    if est is not None:
        batch = np.ascontiguousarray(np.stack([np.asarray(f) for f in frames]))
        kw = {} if not max_peaks else {"n_views": len(batch), "max_peaks": int(max_peaks), "peak_thr": peak_thr,
                                       "peak_min_rel": peak_min_rel, "peak_radius": peak_radius}
        r = est.run(torch.from_numpy(batch).to(est.device).contiguous(), **kw)
        pts = r["keypoints"].cpu().numpy()
        conf = r["scores"].cpu().numpy()
        heat = list(r["gaussians"].cpu().numpy())
    else:
        results = [model(frame) for frame in frames]
        if getattr(model, "__module__", "").startswith("onepose"):
            pts = [np.asarray(res["points"]) for res in results]
            conf = [np.asarray(res["confidence"]).squeeze() for res in results]
        else:
            pts = [np.asarray(res[0]["keypoints"]).squeeze() for res in results]
            conf = [np.asarray(res[0]["keypoint_scores"]).squeeze() for res in results]
        try:
            heat = [res[1] for res in results]
        except (IndexError, KeyError, TypeError):
            heat = []
    stacked = np.stack([np.concatenate((p, np.expand_dims(c, 1)), axis=1) for p, c in zip(pts, conf)], axis=2)
    if max_peaks:
        return stacked, heat, r["peaks"][0].cpu().numpy()
    return stacked, heat


def video_device():
    """Where load_frames reconstructs MPEG-4 Part 2 and JPEG (MJPEG AVI, frame<N>.jpg) recordings:
    the GPU (split decode, frames land in HBM) unless MVPOSE_VIDEO_DECODE=host or no GPU is visible."""
    if os.environ.get("MVPOSE_VIDEO_DECODE", "device") == "host" or not torch.cuda.is_available():
        return None
    return torch.device("cuda", torch.cuda.current_device())


def load_frames(recording_paths, start_end_frames=(0, -1), device=None):
    """{camera: (T', H, W, 3) uint8 BGR} sliced [start:end] (utils.py:903-909 ->
    frame_generator :849-900).  A recording is a .npy stack (memory-mapped), an MPEG-4 Part 2
    ('mp4v') MP4 / AVI / raw stream, an MJPEG or uncompressed AVI, a directory of frame<N>.jpg
    files (mvpose.video), or an in-memory array / tensor; other codecs raise
    NotImplementedError (no decoder in this image).  device: mp4v recordings, MJPEG AVIs and
    frame<N>.jpg directories are then split-decoded onto it (host entropy decoding, GPU
    reconstruction) and come back as device tensors, bit-identical to the host decoders' frames;
    a JPEG slice larger than half of the device's free memory stays a host array
    (video.read_recording's max_device_bytes)."""
    from . import video
    if isinstance(recording_paths, (list, tuple)):
        recording_paths = dict(enumerate(recording_paths))
    if not isinstance(recording_paths, dict):
        return None
    a, b = (0, -1) if start_end_frames is None else start_end_frames
    out = {}
    for k, path in recording_paths.items():
        if isinstance(path, (np.ndarray, torch.Tensor)):  # already-decoded frames in memory
            out[k] = path[a:b]
            continue
        out[k] = video.read_recording(path, a, b, device=device)
    return out


def resolve_estimator(model):
    """The GPU estimator behind the reference's `model` argument, or None: a BatchPoseEstimator
    or mvpose PoseEstimator, or one's bound predict (what estimate_pose_from_video passes,
    `model = model_structure.predict`, pose_estimation.py:297)."""
    from .mmpose_pose_estimation import PoseEstimator
    obj = getattr(model, "__self__", model)
    return obj if isinstance(obj, (BatchPoseEstimator, PoseEstimator)) else None


def build_estimator(model, detector_model="coco_base", model_yaml="", frame_hw=(720, 1280), max_frames=256,
                    device=None):
    """The estimator estimate_pose_from_video builds for a model NAME (pose_estimation.py:
    290-297): PoseEstimator(det_cfg, det_ckpt, pose_cfg, pose_ckpt) from model_yaml's
    detectors[detector_model] and pose_estimators[model] entries — a detector always sits in
    front, as in the reference.  Checkpoints must be LOCAL files (weights_only loads);
    MVPOSE_RANDOM_WEIGHTS=1 / MVPOSE_RANDOM_DETECTOR=1 select seeded synthetic weights (the yaml
    may then be absent), MVPOSE_NO_DETECTOR=1 opts out of the detector (whole-image crops).
    An estimator object (or its bound predict) is returned as is.  frame_hw is accepted for
    compatibility: the estimator sizes itself to the first frames it sees."""
    from .mmpose_pose_estimation import PoseEstimator
    est = resolve_estimator(model)
    if est is not None:
        return est
    dev = torch.device(device if device is not None else "cuda")
    det_cfg = det_ckpt = pose_cfg = pose_ckpt = None
    if model_yaml and os.path.exists(model_yaml):
        with open(model_yaml) as f:
            paths = yaml.safe_load(f) or {}
        det_cfg, det_ckpt = paths.get("detectors", {}).get(detector_model, (None, None))
        if model not in paths.get("pose_estimators", {}) and os.environ.get("MVPOSE_RANDOM_WEIGHTS") != "1":
            raise KeyError(f"pose estimator {model!r} not in {model_yaml}'s pose_estimators")
        pose_cfg, pose_ckpt = paths.get("pose_estimators", {}).get(model, (None, None))
    elif os.environ.get("MVPOSE_RANDOM_WEIGHTS") != "1":
        raise FileNotFoundError(f"model_yaml {model_yaml!r} not found (set MVPOSE_RANDOM_WEIGHTS=1 for random "
                                "weights)")
    return PoseEstimator(det_cfg, det_ckpt, pose_cfg, pose_ckpt, device=dev, max_frames=max_frames)


class FrameStreamer:
    """Overlapped host -> GPU frame supply for recorded videos (the reference decodes and
    holds whole videos on the host, utils.py:849-909, then loops frame by frame).

    Per chunk of `batch_frames` synchronised frames: a host thread gathers the V cameras'
    frames into a PINNED staging buffer (numpy copies release the GIL), the H2D copy runs
    on a dedicated copy stream, and the estimator consumes the device buffer on the
    compute stream — so chunk i+1's gather and copy overlap chunk i's kernels.  Two pinned
    and two device buffers (each capped at `max_staging_bytes`); every hand-off is an event
    (no host synchronisation inside the loop).  With a PoseEstimator the detector runs on
    each chunk on the device and its boxes crop the frames (mmpose_pose_estimation.py:
    234-253).  Outputs accumulate on the device and come back with one copy at the end.
    Use as a context manager (or call close()) to release the gather threads."""

    def __init__(self, est, n_views: int, frame_hw, batch_frames: int = 128, gather_threads: int = 8,
                 max_staging_bytes: int = 512 << 20):
        from concurrent.futures import ThreadPoolExecutor
        self.est = est
        self.pool = ThreadPoolExecutor(max_workers=max(1, min(int(gather_threads), os.cpu_count() or 1)))
        self.V = int(n_views)
        self.H, self.W = (int(v) for v in frame_hw)
        per_frame = self.V * self.H * self.W * 3
        self.step = max(1, min(int(batch_frames), est.max_frames // self.V, int(max_staging_bytes) // per_frame))
        shape = (self.step, self.V, self.H, self.W, 3)
        self.device = est.device
        self.host = [torch.empty(shape, dtype=torch.uint8).pin_memory() for _ in range(2)]
        self.dev = [torch.empty(shape, dtype=torch.uint8, device=self.device) for _ in range(2)]
        self.copy_stream = torch.cuda.Stream(self.device)
        self.copied = [None, None]     # copy-stream event: H2D of buffer k done (host buffer reusable)
        self.consumed = [None, None]   # compute-stream event: kernels done reading device buffer k

    def close(self):
        self.pool.shutdown(wait=True)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _gather(self, stacks, t0, t1, k):
        """Chunk [t0, t1) of every camera into pinned buffer k, in pieces of 4 frames over the
        gather threads (numpy releases the GIL for the copies)."""
        h = self.host[k].numpy()
        jobs = [(v, a, min(t1, a + 4)) for v in range(self.V) for a in range(t0, t1, 4)]

        def cp(job):
            v, a, b = job
            np.copyto(h[a - t0:b - t0, v], stacks[v][a:b])
        for _ in self.pool.map(cp, jobs):
            pass

    def run(self, stacks, n_frames=None, **peak_kw):
        """stacks: V arrays (T, H, W, 3) uint8 (memory-mapped .npy or in memory).  Returns
        device tensors kpts_2d (T, 17, 3, V) f32 and heatmaps (T, V, 17, 6) f64; with peak_kw
        (BatchPoseEstimator.run's max_peaks > 0, peak_thr, peak_min_rel, peak_radius) also peaks
        (T, 17, max_peaks, 3, V) f32."""
        from concurrent.futures import ThreadPoolExecutor
        T = min(len(s) for s in stacks) if n_frames is None else int(n_frames)
        dev = self.device
        kp = torch.empty((T, N_JOINTS, 3, self.V), dtype=torch.float32, device=dev)
        hm = torch.empty((T, self.V, N_JOINTS, 6), dtype=torch.float64, device=dev)
        M = int(peak_kw.get("max_peaks", 0))
        pk = torch.empty((T, N_JOINTS, M, 3, self.V), dtype=torch.float32, device=dev) if M else None
        chunks = [(t, min(T, t + self.step)) for t in range(0, T, self.step)]
        main = torch.cuda.current_stream(dev)
        if any(isinstance(s, torch.Tensor) and s.is_cuda for s in stacks):
            # frames already in device memory (split-decoded recordings): no host staging or H2D,
            # each chunk's views interleaved (t, v)-major on the device
            dstacks = [s.to(dev) if isinstance(s, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(s)).to(dev)
                       for s in stacks]
            for t0, t1 in chunks:
                n = t1 - t0
                fr = self.dev[0][:n]
                for v, s in enumerate(dstacks):
                    fr[:, v].copy_(s[t0:t1])
                r = self.est.run(fr.reshape(n * self.V, self.H, self.W, 3), n_views=self.V, kpts_tkv=kp[t0:t1],
                                 **peak_kw)
                hm[t0:t1] = r["gaussians"].reshape(n, self.V, N_JOINTS, 6)
                if M:
                    pk[t0:t1] = r["peaks"]
            return (kp, hm, pk) if M else (kp, hm)
        with ThreadPoolExecutor(max_workers=1) as pool:
            fut = pool.submit(self._gather, stacks, *chunks[0], 0) if chunks else None
            for i, (t0, t1) in enumerate(chunks):
                k = i & 1
                fut.result()                                   # chunk i is in pinned buffer k
                if i + 1 < len(chunks):                        # gather chunk i+1 meanwhile
                    kn = k ^ 1
                    if self.copied[kn] is not None:
                        self.copied[kn].synchronize()          # its previous H2D has left buffer kn
                    fut = pool.submit(self._gather, stacks, *chunks[i + 1], kn)
                n = t1 - t0
                with torch.cuda.stream(self.copy_stream):
                    if self.consumed[k] is not None:
                        self.copy_stream.wait_event(self.consumed[k])
                    self.dev[k][:n].copy_(self.host[k][:n], non_blocking=True)
                    ev = torch.cuda.Event()
                    ev.record(self.copy_stream)
                    self.copied[k] = ev
                main.wait_event(ev)
                fr = self.dev[k][:n].reshape(n * self.V, self.H, self.W, 3)
                r = self.est.run(fr, n_views=self.V, kpts_tkv=kp[t0:t1], **peak_kw)
                hm[t0:t1] = r["gaussians"].reshape(n, self.V, N_JOINTS, 6)
                if M:
                    pk[t0:t1] = r["peaks"]
                ce = torch.cuda.Event()
                ce.record(main)
                self.consumed[k] = ce
        return (kp, hm, pk) if M else (kp, hm)


def run_pose_est(model, confidence=0.5, camera_indices=None, recording_paths=None, start_end_frames=(0, -1),
                 frame_shape=(1080, 1920), batch_frames=128, max_peaks=0, peak_thr=0.1, peak_min_rel=0.3,
                 peak_radius=1):
    """pose_estimation.py:157-244 -> kpts_2d (T, 17, 3, V) float32, heatmaps (T, V, 17, 6)
    float64 (numpy).  recording_paths values may also be in-memory (T, H, W, 3) uint8 arrays.

    model: a PoseEstimator (detector in front) / BatchPoseEstimator or one's bound predict ->
    every frame through the batched GPU path (FrameStreamer); a model name -> build_estimator;
    any other per-frame callable with the reference's contract -> get_pose_2D frame by frame,
    as the reference loops (:184-190).  confidence does not change the output (it only
    selects what the reference draws, :117-131).
    max_peaks > 0 (GPU estimators only): a third result, peaks (T, 17, max_peaks, 3, V) float32, the
    modes of every heatmap (ops.heatmap_peaks with peak_thr, peak_min_rel, peak_radius)."""
    gpu_model = isinstance(model, str) or resolve_estimator(model) is not None
    frames = load_frames(recording_paths, start_end_frames, device=video_device() if gpu_model else None)
    cams = list(frames.keys()) if camera_indices is None else list(camera_indices)
    stacks = [frames[c] for c in cams]
    V = len(stacks)
    H, W = stacks[0].shape[1:3]
    est = build_estimator(model, frame_hw=(H, W)) if isinstance(model, str) else resolve_estimator(model)
    if est is None and max_peaks:
        raise ValueError("max_peaks needs a BatchPoseEstimator / PoseEstimator: a per-frame callable returns no heatmaps")
    if est is None:                                   # a generic per-frame callable
        stacks = [s.cpu().numpy() if isinstance(s, torch.Tensor) else s for s in stacks]
        T = min(len(s) for s in stacks)
        res = [get_pose_2D([s[t] for s in stacks], model, confidence) for t in range(T)]
        return (np.array([r[0] for r in res], dtype=np.float32).reshape(T, N_JOINTS, 3, V),
                np.array([r[1] for r in res]))
    peak_kw = {} if not max_peaks else {"max_peaks": int(max_peaks), "peak_thr": peak_thr, "peak_min_rel": peak_min_rel,
                                        "peak_radius": peak_radius}
    with FrameStreamer(est, V, (H, W), batch_frames) as fs:
        res = fs.run(stacks, **peak_kw)
    return tuple(a.cpu().numpy() for a in res)


def estimate_pose_from_video(camera_names, recording_paths, model, detector_model="coco_base", model_yaml="",
                             start_end_frames=(0, -1), confidence=0, extrinsic_params_dir="",
                             recompute_kpts_2d=True, triangulation="reference", inlier_px=10.0, min_conf=0.0,
                             return_info=False, refine=None, cov_floor=1.0, sync=None, max_lag=60,
                             fix_swaps=None, max_peaks=4, peak_thr=0.1, peak_min_rel=0.3, peak_radius=1):
    """pose_estimation.py:259-327.  recompute_kpts_2d replaces the reference's interactive
    y/n prompt when kpts_2d.npy already exists (:287-289).

    triangulation: "reference" (default) triangulates from cameras [0, 1] as the reference
    hard-codes (:319); "all_views" and "robust" (get_pose_3D's methods, with inlier_px and
    min_conf) list every camera in camera_names.  return_info appends get_pose_3D's info
    dict to the returned tuple.  "peaks" (every camera too) also keeps up to max_peaks modes of
    every heatmap (peak_thr, peak_min_rel, peak_radius: ops.heatmap_peaks) and lets
    ops.triangulate_peaks choose among them; the modes are saved beside kpts_2d.npy as
    kpts_2d_peaks.npy (T, 17, M, 3, V), loaded from there when the 2D stage does not run, and take
    the same per-camera frame offsets as kpts_2d; info holds them as "peaks", with get_pose_3D's
    "sel" and "kpts_selected".  Unlike kpts_2d.npy, which the caller writes, kpts_2d_peaks.npy is
    written here, as the 2D stage returns it (before any frame offsets); the command line then
    writes the returned, aligned peaks over it, as it does for kpts_2d.npy.  "peaks" with fix_swaps raises ValueError (the peak lists are not
    carried through the exchange).  refine / cov_floor: get_pose_3D's maximum-likelihood refinement
    of the triangulated points ("heatmap" reads this run's heatmaps_2d, so it needs the 2D stage
    to run: recompute_kpts_2d, or no kpts_2d.npy yet).

    sync: None (default: frame t of every camera is taken to show the same instant) or "pose":
    after the 2D stage the cameras' frame offsets are estimated from the keypoints
    (sync.estimate_frame_offsets over all cameras in camera_names, lags of -max_lag..max_lag
    frames), kpts_2d and heatmaps_2d are cut to the common instants (sync.apply_frame_offsets) and
    the aligned arrays are triangulated and returned.  ValueError, naming the cameras, when an
    offset cannot be fixed.  info then also holds "frame_offsets" (V,) int64, "frame_first" (each
    camera's first kept frame) and "sync_pairs", estimate_frame_offsets' pair table.

    fix_swaps: None (default: the detector's left/right labels are taken as they are), "limbs" or
    "body" (swaps.PRESETS): after synchronisation and before triangulation, the left/right label
    exchanges of every camera in camera_names are found and undone (swaps.fix_label_swaps) in
    kpts_2d and heatmaps_2d; the fixed arrays are triangulated and returned.  info then also holds
    "label_swaps" (T, U) uint8: bit v set where camera v's labels of unit u were exchanged."""
    if triangulation not in TRIANGULATION_METHODS:
        raise ValueError(f"triangulation {triangulation!r}: one of {TRIANGULATION_METHODS}")
    _check_refine(refine)
    if sync not in SYNC_MODES:
        raise ValueError(f"sync {sync!r}: one of {SYNC_MODES}")
    if fix_swaps is not None and fix_swaps not in label_swaps.PRESETS:
        raise ValueError(f"fix_swaps {fix_swaps!r}: None or one of {tuple(label_swaps.PRESETS)}")
    with_peaks = triangulation == "peaks"
    if with_peaks and fix_swaps is not None:
        raise ValueError('fix_swaps does not apply to triangulation="peaks": the peak lists are not carried through '
                         "the label exchange")
    if with_peaks and refine == "heatmap":
        raise ValueError('refine="heatmap" does not apply to triangulation="peaks"')
    index_name, _origin = geometry.load_camera_names(extrinsic_params_dir)
    name_index = {v: k for k, v in index_name.items()}
    camera_indices = [name_index[n] for n in camera_names]
    camera_params = {}
    for i, name in enumerate(camera_names):
        _, camera_params[i] = geometry.get_params_from_name(name, extrinsic_params_dir=extrinsic_params_dir)
    folder = os.path.dirname(recording_paths[0])
    existing = os.path.join(folder, "kpts_2d.npy")
    existing_peaks = os.path.join(folder, "kpts_2d_peaks.npy")
    heatmaps = peaks = None
    if os.path.exists(existing) and not recompute_kpts_2d:
        kpts_2d = np.load(existing)
        if with_peaks:
            if not os.path.exists(existing_peaks):
                raise FileNotFoundError(f'triangulation="peaks" needs {existing_peaks} beside kpts_2d.npy: run the 2D '
                                        "stage again (recompute_kpts_2d=True)")
            peaks = np.load(existing_peaks)
    else:
        paths = {i: recording_paths[i] for i in camera_indices}   # as :281 indexes them
        gpu_model = isinstance(model, str) or resolve_estimator(model) is not None
        frames = load_frames(paths, start_end_frames,           # decoded once (mp4v: onto the GPU)
                             device=video_device() if gpu_model else None)
        if isinstance(model, str):                             # :290-297: detector + pose model from the yaml
            model = build_estimator(model, detector_model, model_yaml,
                                    frame_hw=tuple(frames[camera_indices[0]].shape[1:3]))
        res = run_pose_est(model, confidence=confidence, camera_indices=camera_indices, recording_paths=frames,
                           start_end_frames=(0, None), max_peaks=max_peaks if with_peaks else 0, peak_thr=peak_thr,
                           peak_min_rel=peak_min_rel, peak_radius=peak_radius)
        kpts_2d, heatmaps = res[:2]
        if with_peaks:
            peaks = res[2]
            np.save(existing_peaks, peaks)
    sync_info = {}
    if sync == "pose":
        offsets, pair_info = frame_sync.estimate_frame_offsets(kpts_2d, camera_params, max_lag=max_lag)
        lost = [camera_names[v] for v in np.flatnonzero(offsets == frame_sync.NO_OFFSET)]
        if lost:
            why = [f"{camera_names[a]}-{camera_names[b]}: {r}"
                   for (a, b), r in zip(pair_info["pairs"], pair_info["reason"]) if r]
            raise ValueError(f"sync='pose': no frame offset for camera(s) {lost} (rejected pairs: {why})")
        (kpts_2d, heatmaps, peaks), first = frame_sync.apply_frame_offsets([kpts_2d, heatmaps, peaks], offsets,
                                                                            (3, 1, 4))
        sync_info = {"frame_offsets": offsets, "frame_first": first, "sync_pairs": pair_info}
    if fix_swaps is not None:
        kpts_2d, heatmaps, swap = label_swaps.fix_label_swaps(kpts_2d, camera_params, units=fix_swaps,
                                                              heatmaps_2d=heatmaps, min_conf=min_conf)
        sync_info["label_swaps"] = swap
    if triangulation == "reference" and refine is None:
        listed = [0, 1]
        kpts_3d = get_pose_3D(camera_params, kpts_2d, camera_indices=listed)
        info = {"inliers": None, "reproj_err": None}
    else:
        listed = [0, 1] if triangulation == "reference" else list(range(len(camera_names)))
        kpts_3d, info = get_pose_3D(camera_params, kpts_2d, camera_indices=listed, method=triangulation,
                                    inlier_px=inlier_px, min_conf=min_conf, return_info=True, refine=refine,
                                    heatmaps_2d=heatmaps, cov_floor=cov_floor, peaks=peaks)
        if with_peaks:
            info["peaks"] = peaks
    info.update(sync_info)
    if return_info:
        return kpts_2d, heatmaps, kpts_3d, info
    return kpts_2d, heatmaps, kpts_3d
