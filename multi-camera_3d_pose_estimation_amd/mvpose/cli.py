"""The reference's two command lines, same flags / YAML / output files, GPU hot path.

* ``record_and_estimate_pose`` (record_and_estimate_pose.py:12-84): for a given
  configuration and recordings, 2D pose per frame + triangulation ->
  ``kpts_2d.npy`` (T,17,3,V) f32, ``heatmaps_2d.npy`` (T,V,17,6) f64,
  ``kpts_3d.npy`` (T,17,3) f32 and ``recording_log.yaml`` in the recordings
  folder.  Camera configuration (GUI), webcam recording and audio-clap
  synchronisation are outside the hot path: the flags are accepted, and asking
  for those steps raises NotImplementedError.
* ``pose_refinement`` (pose_refinement.py:1099-1255): missing arguments filled
  from recording_log.yaml; ``linear_interpolation`` always runs (GPU kernel) and
  is saved when requested; ``SGD`` runs the one-launch GPU refinement with the
  ``SGD`` section of --refinement_params_yaml and saves ``kpts_3d_SGD.npy``;
  ``smooth`` (no reference counterpart) runs the covariance-weighted smoother with the
  ``smooth`` section and saves ``kpts_3d_smooth.npy`` and ``kpts_3d_smooth_resid.npy``, and
  with ``with_cov: true`` in that section ``kpts_3d_smooth_cov.npy``, (T, J, 3, 3).
"""
from __future__ import annotations

import argparse
import inspect
import os
from pathlib import Path

import numpy as np
import torch
import yaml

from . import geometry


def load_config(config_path=None):
    """utils.load_config (utils.py:1376-1381)."""
    if config_path is None:
        return {}
    with open(config_path) as f:
        return yaml.safe_load(f) or {}


def prepare_kwargs(func, user_kwargs):
    """utils.prepare_kwargs (utils.py:1388-1399): function defaults updated by the YAML
    section; ".inf" -> np.inf, betas list -> tuple."""
    kw = {k: v.default for k, v in inspect.signature(func).parameters.items()
          if v.default is not inspect.Parameter.empty}
    kw.update(user_kwargs or {})
    for k, v in kw.items():
        if v == ".inf":
            kw[k] = np.inf
        if k == "betas" and isinstance(v, list):
            kw[k] = tuple(v)
    return kw


# --------------------------------------------------------------------- record + estimate
def record_and_estimate_pose(camera_names, estimator_model="coco_base", detector_model="coco_base",
                             configuration_number=None, recording_paths=None, synchronize_video=True,
                             model_yaml="./model_paths.yaml", calibration_settings_yaml="./calibration_settings.yaml",
                             checkerboard_display_parameter_yaml="./checkerboard_display_parameters.yaml",
                             origin_camera_idx=0, script_path=None, project_dir="", recording_length_seconds=10,
                             keep_unsynced_files=False, triangulation="reference", inlier_px=10.0,
                             min_confidence=0.0, refine=None, cov_floor=1.0, sync_from_pose=False, max_lag=60,
                             fix_label_swaps=None, max_peaks=4, peak_threshold=0.1, peak_min_rel=0.3):
    """triangulation / inlier_px / min_confidence (no reference counterpart): "reference" (default)
    triangulates from cameras [0, 1] and writes exactly the reference's files; "all_views" and
    "robust" use every camera in camera_names (estimate_pose_from_video), record the three
    settings in recording_log.yaml and also write kpts_3d_inliers.npy (T,17,V) bool and, for
    "robust", kpts_3d_reproj_err.npy (T,17,V) f32.  "peaks" (max_peaks, peak_threshold,
    peak_min_rel: estimate_pose_from_video's max_peaks, peak_thr, peak_min_rel) also keeps the
    modes of every heatmap, written as kpts_2d_peaks.npy (T,17,M,3,V) f32, and lets the geometry
    choose among them: kpts_2d_selected.npy (T,17,3,V) f32 and kpts_3d_peak_sel.npy (T,17,V) int8 are
    written beside the "robust" files and the three settings recorded too; kpts_2d.npy stays the argmax.
    refine / cov_floor (no reference counterpart): "unit", "conf" or "heatmap" refines the
    triangulated points by maximum likelihood (get_pose_3D); kpts_3d.npy then holds the refined
    points, and kpts_3d_seed.npy, kpts_3d_cov.npy (T,17,3,3) f32 and kpts_3d_refine_status.npy
    (T,17) uint8 are written too, the two settings recorded in recording_log.yaml.
    sync_from_pose / max_lag (no reference counterpart): the cameras' frame offsets are estimated
    from the 2D keypoints over lags of -max_lag..max_lag frames (estimate_pose_from_video's
    sync="pose"); kpts_2d.npy, heatmaps_2d.npy and everything after them then hold the frames cut
    to the common instants, frame_offsets.npy (V,) int64 is written too, and recording_log.yaml
    records the offsets, max_lag and the rejected pairs under "sync".
    fix_label_swaps (no reference counterpart): "limbs" or "body" finds and undoes the detector's
    per-camera left/right label exchanges (estimate_pose_from_video's fix_swaps) after the
    synchronisation and before the triangulation; kpts_2d.npy, heatmaps_2d.npy and everything
    after them hold the fixed labels, label_swaps.npy (T, U) uint8 is written too, and
    recording_log.yaml records the preset and the number of exchanged (frame, unit, camera)
    entries under "fix_label_swaps"."""
    if refine not in (None, "unit", "conf", "heatmap"):
        raise ValueError(f"refine {refine!r}: None, 'unit', 'conf' or 'heatmap'")
    from .pose_estimation import estimate_pose_from_video
    if project_dir:
        os.chdir(project_dir)
    if configuration_number is None:
        raise NotImplementedError("camera configuration (setup_camera_configuration) is outside the GPU hot "
                                  "path: pass --configuration_number of an existing configuration")
    configuration_dir = f"./configurations/{configuration_number}/"
    if not recording_paths:
        raise NotImplementedError("webcam recording is outside the GPU hot path: pass --recording_paths")
    if synchronize_video:
        raise NotImplementedError("audio-based video synchronisation is outside the GPU hot path: pass "
                                  "already synchronised recordings (omit --synchronize_video), or let --sync_from_pose "
                                  "estimate the cameras' frame offsets from the 2D keypoints")
    recordings_folder = os.path.dirname(recording_paths[0])
    robust_kw = {}
    if triangulation != "reference":
        robust_kw = {"triangulation": triangulation, "inlier_px": inlier_px, "min_conf": min_confidence,
                     "return_info": True}
    if triangulation == "peaks":
        robust_kw.update({"max_peaks": max_peaks, "peak_thr": peak_threshold, "peak_min_rel": peak_min_rel})
    if refine is not None:
        robust_kw.update({"refine": refine, "cov_floor": cov_floor, "return_info": True})
    if sync_from_pose:
        robust_kw.update({"sync": "pose", "max_lag": max_lag, "return_info": True})
    if fix_label_swaps is not None:
        robust_kw.update({"fix_swaps": fix_label_swaps, "return_info": True})
    kpts_2d, heatmaps, kpts_3d, *info = estimate_pose_from_video(
        camera_names, recording_paths, estimator_model, detector_model=detector_model, model_yaml=model_yaml,
        start_end_frames=[0, -1], confidence=0,
        extrinsic_params_dir=os.path.join(configuration_dir, "extrinsic_camera_parameters"), **robust_kw)
    log = {"recording_paths": [str(p) for p in recording_paths],
           "kpts_2d": str(os.path.join(recordings_folder, "kpts_2d.npy")),
           "heatmaps_2d": str(os.path.join(recordings_folder, "heatmaps_2d.npy")),
           "kpts_3d": str(os.path.join(recordings_folder, "kpts_3d.npy")),
           "estimator_model": estimator_model, "detector_model": detector_model}
    extra = {}
    if triangulation != "reference":
        log.update({"triangulation": triangulation, "inlier_px": float(inlier_px),
                    "min_confidence": float(min_confidence)})
        for key, name in (("inliers", "kpts_3d_inliers"), ("reproj_err", "kpts_3d_reproj_err")):
            if info[0][key] is not None:
                log[name] = str(os.path.join(recordings_folder, name + ".npy"))
                extra[name] = info[0][key]
    if triangulation == "peaks":
        log.update({"max_peaks": int(max_peaks), "peak_threshold": float(peak_threshold),
                    "peak_min_rel": float(peak_min_rel)})
        for key, name in (("peaks", "kpts_2d_peaks"), ("kpts_selected", "kpts_2d_selected"), ("sel", "kpts_3d_peak_sel")):
            log[name] = str(os.path.join(recordings_folder, name + ".npy"))
            extra[name] = info[0][key]
    if refine is not None:
        log.update({"refine": refine, "cov_floor": float(cov_floor)})
        for key, name in (("seed", "kpts_3d_seed"), ("cov", "kpts_3d_cov"), ("refine_status", "kpts_3d_refine_status")):
            log[name] = str(os.path.join(recordings_folder, name + ".npy"))
            extra[name] = info[0][key]
    if sync_from_pose:
        pair_info = info[0]["sync_pairs"]
        log["frame_offsets"] = str(os.path.join(recordings_folder, "frame_offsets.npy"))
        extra["frame_offsets"] = info[0]["frame_offsets"]
        log["sync"] = {"method": "pose", "max_lag": int(max_lag),
                       "offsets": [int(o) for o in info[0]["frame_offsets"]],
                       "rejected_pairs": [[camera_names[a], camera_names[b], r]
                                          for (a, b), r in zip(pair_info["pairs"], pair_info["reason"]) if r]}
    if fix_label_swaps is not None:
        swap = info[0]["label_swaps"]
        log["label_swaps"] = str(os.path.join(recordings_folder, "label_swaps.npy"))
        extra["label_swaps"] = swap
        log["fix_label_swaps"] = {"units": fix_label_swaps,
                                  "exchanged": int(np.unpackbits(np.ascontiguousarray(swap)).sum())}
    with open(os.path.join(recordings_folder, "recording_log.yaml"), "w") as f:
        yaml.dump(log, f)
    if kpts_2d is not None:
        np.save(log["kpts_2d"], kpts_2d)
    if heatmaps is not None:
        np.save(log["heatmaps_2d"], heatmaps)
    if kpts_3d is not None:
        np.save(log["kpts_3d"], kpts_3d)
    for name, arr in extra.items():
        np.save(log[name], arr)
    return log


def record_and_estimate_pose_parser(extensions=False):
    """Flags of record_and_estimate_pose.py:63-78; extensions=True (what the command line uses)
    adds the flags beyond the reference's: --triangulation, --inlier_px, --min_confidence,
    --refine, --cov_floor, --sync_from_pose, --max_lag, --fix_label_swaps, --max_peaks,
    --peak_threshold, --peak_min_rel."""
    p = argparse.ArgumentParser()
    p.add_argument("--camera_names", nargs="+", required=True, help="List of camera names")
    p.add_argument("--estimator_model")
    p.add_argument("--detector_model")
    p.add_argument("--configuration_number", type=int)
    p.add_argument("--recording_paths", nargs="*")
    p.add_argument("--synchronize_video", action="store_true")
    p.add_argument("--model_yaml")
    p.add_argument("--calibration_settings_yaml")
    p.add_argument("--checkerboard_display_parameter_yaml")
    p.add_argument("--origin_camera_idx", type=int)
    p.add_argument("--script_path")
    p.add_argument("--project_dir")
    p.add_argument("--recording_length_seconds", type=int)
    p.add_argument("--keep_unsynced_files", action="store_true")
    if extensions:   # N-view triangulation (estimate_pose_from_video's `triangulation`)
        p.add_argument("--triangulation", choices=["reference", "all_views", "robust", "peaks"])
        p.add_argument("--inlier_px", type=float)
        p.add_argument("--min_confidence", type=float)
        p.add_argument("--max_peaks", type=int)             # --triangulation peaks: modes kept per heatmap
        p.add_argument("--peak_threshold", type=float)
        p.add_argument("--peak_min_rel", type=float)
        p.add_argument("--refine", choices=["unit", "conf", "heatmap"])   # maximum-likelihood refinement
        p.add_argument("--cov_floor", type=float)
        p.add_argument("--sync_from_pose", action="store_true")   # frame offsets from the 2D keypoints
        p.add_argument("--max_lag", type=int)
        p.add_argument("--fix_label_swaps", choices=["limbs", "body"])   # undo per-camera left/right exchanges
    return p


def record_and_estimate_pose_main(argv=None):
    args = record_and_estimate_pose_parser(extensions=True).parse_args(argv)
    return record_and_estimate_pose(**{k: v for k, v in vars(args).items() if v is not None})


# --------------------------------------------------------------------- refinement
def pose_refinement_parser(extensions=False):
    """Flags of pose_refinement.py:1100-1116; extensions=True (what the command line uses) adds
    the flags beyond the reference's: --kpts_3d_cov, --kpts_3d_refine_status (inputs of the
    "smooth" refinement type)."""
    p = argparse.ArgumentParser()
    p.add_argument("--run_path", type=str)
    p.add_argument("--refinement_types", nargs="+", default=["linear_interpolation"])
    p.add_argument("--recording_log", type=str)
    p.add_argument("--heatmaps_2d", type=str)
    p.add_argument("--kpts_2d", type=str)
    p.add_argument("--kpts_3d", type=str)
    p.add_argument("--model", type=str)
    p.add_argument("--save_path", type=str)
    p.add_argument("--extrinsic_params_dir", type=str)
    p.add_argument("--intrinsic_params_dir", type=str)
    p.add_argument("--refinement_params_yaml", type=str)
    p.add_argument("--body_part_lengths_yaml", type=str)
    p.add_argument("--body_part_lengths_individual_name_yaml", default="my_lengths", type=str)
    p.add_argument("--ignore_body_lengths", action="store_true")
    p.add_argument("--interpolate_before_SGD", action="store_true")
    if extensions:   # what record_and_estimate_pose --refine writes beside kpts_3d.npy
        p.add_argument("--kpts_3d_cov", type=str)
        p.add_argument("--kpts_3d_refine_status", type=str)
    return p


def _load_if_exists(path):
    return np.load(path) if path is not None and os.path.exists(str(path)) else None


def _camera_params(args):
    """{index: [K, R, T, dist]} of the cameras named in the extrinsic parameter folder."""
    cameras, _origin = geometry.load_camera_names(str(args.extrinsic_params_dir))
    cam_params = {}
    for i in cameras:
        _, cam_params[i] = geometry.get_params_from_name(cameras[i], intrinsic_params_dir=str(
            args.intrinsic_params_dir), extrinsic_params_dir=str(args.extrinsic_params_dir))
    return cam_params


def _body_lengths(args):
    """The individual's {segment name: length} from the body-lengths YAML, or None."""
    if args.ignore_body_lengths:
        return None
    if args.body_part_lengths_yaml is None and os.path.exists("./body_part_lengths.yaml"):
        args.body_part_lengths_yaml = "./body_part_lengths.yaml"
    if args.body_part_lengths_yaml is None:
        return None
    with open(args.body_part_lengths_yaml) as f:
        return yaml.safe_load(f)[args.body_part_lengths_individual_name_yaml]


def pose_refinement_main(argv=None):
    from .refine import SEGMENTS, Optimized_3d_Pose_Estimation, fit_skeleton, linear_interpolation, smooth_trajectory
    args = pose_refinement_parser(extensions=True).parse_args(argv)
    if args.run_path is None:
        args.run_path = os.getcwd()
    if args.save_path is None:
        args.save_path = args.run_path
    if args.extrinsic_params_dir is None:
        args.extrinsic_params_dir = Path(args.run_path).parent.parent / "extrinsic_camera_parameters"
    if args.intrinsic_params_dir is None:
        args.intrinsic_params_dir = os.path.join(os.getcwd(), "intrinsic_camera_parameters")
    log_path = args.recording_log or os.path.join(args.run_path, "recording_log.yaml")
    log = {}
    if os.path.exists(log_path):
        with open(log_path) as f:
            log = yaml.safe_load(f) or {}
    for k, v in vars(args).items():      # fill missing args from the log (:1137-1144)
        if v is None and k in log:
            setattr(args, k, log[k])
    kpts_3d = _load_if_exists(args.kpts_3d)
    heatmaps = _load_if_exists(args.heatmaps_2d)
    params = load_config(args.refinement_params_yaml)
    types = set(args.refinement_types)
    interp = linear_interpolation(kpts_3d, **prepare_kwargs(linear_interpolation, params.get("linear_interpolation")))
    outputs = {}
    if "linear_interpolation" in types:
        path = os.path.join(args.save_path, "kpts_3d_linear_interpolation.npy")
        print(f"saving linear interpolation at {path}")
        np.save(path, interp)
        outputs["linear_interpolation"] = path
        types.discard("linear_interpolation")
    if "SGD" in types:
        cam_params = _camera_params(args)
        my_lengths = _body_lengths(args)
        init = interp if args.interpolate_before_SGD else kpts_3d
        opt = Optimized_3d_Pose_Estimation(torch.tensor(heatmaps), init, decomposed_cam_params_initial=cam_params,
                                           body_lengths=my_lengths)
        kw = prepare_kwargs(opt.sgd_optimize, params.get("SGD"))
        kw.pop("own_camera_gaussians", None)
        opt.sgd_optimize(**kw)
        path = os.path.join(args.save_path, "kpts_3d_SGD.npy")
        print(f"saving SGD at {path}")
        best = opt.best_trajectory
        np.save(path, best.numpy() if best is not None else np.array(None))
        outputs["SGD"] = path
        types.discard("SGD")
    if "smooth" in types:   # whole-recording smoother; sigma0 stands in where no covariance file exists
        kw = prepare_kwargs(smooth_trajectory, params.get("smooth"))
        kw.update({"cov": _load_if_exists(args.kpts_3d_cov), "status": _load_if_exists(args.kpts_3d_refine_status),
                   "return_info": True})
        smooth, info = smooth_trajectory(kpts_3d, **kw)
        path = os.path.join(args.save_path, "kpts_3d_smooth.npy")
        print(f"saving smoothed trajectory at {path}")
        np.save(path, smooth)
        np.save(os.path.join(args.save_path, "kpts_3d_smooth_resid.npy"), info["resid"])
        if "cov" in info:   # with_cov: true in the smooth section
            np.save(os.path.join(args.save_path, "kpts_3d_smooth_cov.npy"), info["cov"])
        outputs["smooth"] = path
        types.discard("smooth")
    if "skeleton_fit" in types:   # the 2D keypoints, the smoothness prior and the bone lengths, from the smoother's seed
        from . import people
        kw = prepare_kwargs(smooth_trajectory, params.get("smooth"))
        kw.update({"cov": _load_if_exists(args.kpts_3d_cov), "status": _load_if_exists(args.kpts_3d_refine_status)})
        seed = smooth_trajectory(kpts_3d, **kw)
        my_lengths = _body_lengths(args)
        if my_lengths is not None:
            seg = {"body_lengths": my_lengths}
        elif args.ignore_body_lengths:   # nobody measured them: the medians of the triangulated frames
            pairs = np.array(list(SEGMENTS.values()), np.int32)
            seg = {"segments": (pairs, people.estimate_bone_lengths(torch.as_tensor(kpts_3d), pairs))}
        else:
            raise ValueError("skeleton_fit needs --body_part_lengths_yaml, or --ignore_body_lengths to estimate the "
                             "lengths from kpts_3d")
        kw = prepare_kwargs(fit_skeleton, params.get("skeleton_fit"))
        kw.update(seg, return_info=True)
        fit, info = fit_skeleton(_load_if_exists(args.kpts_2d), _camera_params(args), seed, **kw)
        path = os.path.join(args.save_path, "kpts_3d_skeleton_fit.npy")
        print(f"saving skeleton fit at {path}")
        np.save(path, fit)
        np.save(os.path.join(args.save_path, "kpts_3d_skeleton_fit_resid.npy"), info["resid"])
        outputs["skeleton_fit"] = path
        types.discard("skeleton_fit")
    if types:
        raise ValueError(f"unknown refinement type(s) {sorted(types)}; expected linear_interpolation, SGD "
                         "and/or smooth, skeleton_fit")
    return outputs
