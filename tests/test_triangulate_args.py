"""CPU: the three triangulation entry points (mvp_triangulate, mvp_triangulate_robust,
mvp_triangulate_refine) share one argument prologue.  Each must reject the same bad arguments with a
message that starts with its own name and names the offending value, return OK for an empty batch
and report null device pointers — all before any device work (every device pointer is NULL here)."""
import ctypes

import pytest

ENTRIES = ["mvp_triangulate", "mvp_triangulate_robust", "mvp_triangulate_refine"]


def _call(fn, n=10, V=2, n_cams=2, idx=(0, 1), n_idx=None):
    """idx=None passes cam_idx = NULL; n_idx overrides the length that is passed."""
    from mvpose import _lib
    ci = None if idx is None else (ctypes.c_int * len(idx))(*idx)
    if n_idx is None:
        n_idx = len(idx)
    head = (None, n, V, None, n_cams, ci, n_idx)
    tail = {
        "mvp_triangulate": (0, None, None, None),                                # mode, outputs, stream
        "mvp_triangulate_robust": (10.0, 0.0, None, None, None, None),           # inlier_px, min_conf, ...
        "mvp_triangulate_refine": (None, None, 0, None, 0, 0.0, 1.0, 10, 1e-7,   # xyz0 .. tol
                                   None, None, None, None, None),
    }[fn]
    rc = getattr(_lib.lib, fn)(*head, *tail)
    return rc, _lib.last_error()


@pytest.mark.parametrize("fn", ENTRIES)
@pytest.mark.parametrize("kw,msg", [
    (dict(n=-1), "n_points < 0"),
    (dict(V=1), "V=1 "),
    (dict(V=65, n_cams=8), "V=65 "),
    (dict(n_cams=0), "n_cams=0 "),
    (dict(n_cams=9), "n_cams=9 "),
    (dict(idx=None, n_idx=2), "cam_idx is NULL"),
    (dict(idx=[0]), "n_cam_idx=1 "),
    (dict(idx=list(range(9)), V=9, n_cams=8), "n_cam_idx=9 "),
    (dict(idx=[0, 2], V=2, n_cams=8), "cam_idx[1]=2 out of range (V=2, n_cams=8)"),
    (dict(idx=[0, 2], V=3, n_cams=2), "cam_idx[1]=2 out of range (V=3, n_cams=2)"),
])
def test_shared_argument_checks(fn, kw, msg):
    rc, err = _call(fn, **kw)
    assert rc == -1
    assert err.startswith(fn + ": "), err
    assert msg in err, err


@pytest.mark.parametrize("fn", ENTRIES)
def test_empty_batch_and_null_pointers(fn):
    rc, _ = _call(fn, n=0)                 # n_points == 0 returns OK before the pointer checks
    assert rc == 0
    rc, err = _call(fn, n=10)
    assert rc == -1
    assert err == fn + ": null device pointer", err
