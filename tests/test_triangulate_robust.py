"""CPU: the robust N-view triangulation's C-ABI entry (mvp_triangulate_robust) is declared and
exported, rejects bad arguments before any device work, and the Python / command-line fronts
accept the new options and reject unknown methods."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "mvpose.h")


def test_header_declares_and_library_exports():
    from mvpose import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+mvp_triangulate_robust\s*\(", src)
    assert hasattr(_lib.lib, "mvp_triangulate_robust")
    assert "mvp_triangulate_robust" in _lib.SIGNATURES


def _call(n, V, n_cams, idx, inlier_px=10.0, min_conf=0.0):
    from mvpose import _lib
    ci = (ctypes.c_int * len(idx))(*idx)
    rc = _lib.lib.mvp_triangulate_robust(None, n, V, None, n_cams, ci, len(idx), inlier_px, min_conf, None, None,
                                         None, None)
    return rc, _lib.last_error()


@pytest.mark.parametrize("kw,msg", [
    (dict(idx=[0]), "n_cam_idx=1"),
    (dict(idx=[0, 1], inlier_px=0.0), "inlier_px"),
    (dict(idx=[0, 1], inlier_px=-3.0), "inlier_px"),
    (dict(idx=[0, 1], inlier_px=float("inf")), "inlier_px"),
    (dict(idx=[0, 1], inlier_px=float("nan")), "inlier_px"),
    (dict(idx=[0, 1], min_conf=float("nan")), "min_conf"),
    (dict(idx=[0, 5]), "cam_idx[1]=5"),
    (dict(idx=[0, -1]), "cam_idx[1]=-1"),
])
def test_bad_arguments_are_reported(kw, msg):
    """Every check runs before any device work (all device pointers are NULL here)."""
    rc, err = _call(10, 2, 2, **kw)
    assert rc == -1
    assert msg in err, err


def test_null_pointers_and_empty_batch():
    rc, err = _call(10, 2, 2, idx=[0, 1])
    assert rc == -1 and "null device pointer" in err
    rc, _ = _call(0, 2, 2, idx=[0, 1])          # n_points == 0 returns OK before the pointer checks
    assert rc == 0
    from mvpose import _lib
    with pytest.raises(_lib.MvposeError):
        ci = (ctypes.c_int * 2)(0, 1)
        _lib.call("mvp_triangulate_robust", None, -1, 2, None, 2, ci, 2, 10.0, 0.0, None, None, None, None)


def test_cli_parser_accepts_the_new_flags():
    from mvpose import cli
    p = cli.record_and_estimate_pose_parser(extensions=True)      # the parser the command line uses
    a = p.parse_args(["--camera_names", "a", "b", "c", "--triangulation", "robust", "--inlier_px", "7.5",
                      "--min_confidence", "0.2"])
    assert (a.triangulation, a.inlier_px, a.min_confidence) == ("robust", 7.5, 0.2)
    assert p.parse_args(["--camera_names", "a", "b", "--triangulation", "all_views"]).triangulation == "all_views"
    d = p.parse_args(["--camera_names", "a", "b"])
    assert d.triangulation is None and d.inlier_px is None and d.min_confidence is None   # function defaults apply
    with pytest.raises(SystemExit):
        p.parse_args(["--camera_names", "a", "b", "--triangulation", "ransac"])
    with pytest.raises(ValueError):       # the function behind the command line checks it too
        cli.record_and_estimate_pose(["a", "b"], configuration_number=1, recording_paths=["x.npy", "y.npy"],
                                     synchronize_video=False, triangulation="ransac")


def test_unknown_methods_raise():
    from mvpose import ops, pipeline, pose_estimation
    with pytest.raises(ValueError):
        pose_estimation.get_pose_3D({}, np.zeros((1, 17, 3, 2), np.float32), method="nope")
    with pytest.raises(ValueError):
        pose_estimation.estimate_pose_from_video(["a", "b"], ["x", "y"], None, triangulation="nope")
    assert ops.TRI_ROBUST not in (ops.TRI_REFERENCE, ops.TRI_ALL_VIEWS)
    assert ops.TRI_ROBUST & (ops.TRI_EXACT_JACOBI | ops.TRI_TOLERANCE) == 0
    with pytest.raises(ValueError):       # tri_solver does not apply to the robust mode
        pipeline.MultiViewPipeline({}, estimator=object(), mode=ops.TRI_ROBUST, tri_solver="reference_compat")
