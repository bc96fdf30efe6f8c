"""GPU: cross-view association (mvp_associate_views) against the numpy restatement
tests/people_ref.py on the inputs of tests/people_cases.py.

group and count must be equal exactly, in every frame: tests/test_people_assoc.py asserts that no
comparison of these inputs is closer than 1e-7, four orders above the kernel's contract of 1e-9.
affinity: the -1 pattern must be equal; the values are fp64 on both sides over the same f32
undistorted pixels, the arithmetic of the lag-cost scan (a term's relative error is about
eps · coordinate scale / d ≈ 1e-13 at d ≈ 1 px, a mean of J terms adds J · eps), so the bound is
that test's rtol of 1e-9.  The measured maximum is printed (DESIGN.md §4.11 quotes it)."""
import numpy as np
import pytest
import torch

import people_cases as cases
from mvpose import synthetic as syn

pytestmark = pytest.mark.gpu
RTOL = 1e-9


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mvpose import ops as _ops
    return _ops


def _device(ops, name, return_affinity=True):
    cams, k, ci, kw = cases.gpu_cases()[name]
    cams_d = torch.tensor(ops.pack_cameras(syn.reference_camera_params(cams)), device="cuda")
    g, c, a, pairs = ops.associate_views(torch.tensor(k, device="cuda"), cams_d, ci, return_affinity=return_affinity,
                                         **kw)
    assert g.dtype == torch.int8 and c.dtype == torch.uint8
    assert tuple(g.shape) == (k.shape[0], len(ci), k.shape[1]) and tuple(c.shape) == (k.shape[0], 2)
    return g.cpu().numpy(), c.cpu().numpy(), None if a is None else a.cpu().numpy(), pairs


@pytest.mark.parametrize("name", sorted(cases.gpu_cases()))
def test_kernel_matches_restatement(ops, name):
    """(nv, P) = (2,1) (2,3) (3,2) (5,3) (4,4) (8,8) (2,32); J = 17, 1, 33 and 60 (the pixels read
    from the workspace); T = 1, 5, 67; V = 5 with cam_idx (3, 0, 4); empty frames, slots below
    min_conf, a node and a node pair short of min_joints; both threshold extremes."""
    r = cases.reference(name)
    g, c, a, pairs = _device(ops, name)
    assert pairs == r["pairs"] and a.dtype == np.float64 and a.shape == r["affinity"].shape
    undefined = r["affinity"] == -1.0
    assert np.array_equal(a == -1.0, undefined)
    d, w = a[~undefined], r["affinity"][~undefined]
    if d.size:
        assert (w > 0).all()
        print(f"{name}: max rel |affinity - ref| = {(np.abs(d - w) / w).max():.3g} over {d.size} values, "
              f"smallest margin {r['margins'].min():.3g}")
        np.testing.assert_allclose(d, w, rtol=RTOL, atol=0)
    assert np.array_equal(g, r["group"])
    assert np.array_equal(c, r["count"])


def test_threshold_extremes(ops):
    g, c, _, _ = _device(ops, "singletons_nv4_P4")
    assert (c[:, 1] == 0).all() and (c[:, 0] == (g >= 0).sum((1, 2))).all()
    for t in range(len(g)):
        lab = g[t][g[t] >= 0]
        assert len(set(lab.tolist())) == lab.size
    for name in ("views_only_nv4_P4", "views_only_nv8_P8"):
        g, c, _, _ = _device(ops, name)
        for t in range(len(g)):
            for q in range(int(c[t, 0])):
                assert ((g[t] == q).sum(1) <= 1).all()      # no group holds two nodes of a view
        assert (c[:, 0] == (g >= 0).sum(2).max(1)).all() and (c[:, 0] > 0).all()


def test_same_bits_on_every_call_and_null_affinity(ops):
    for name in ("nv4_P4_T67", "nv8_P8_T1"):
        a = _device(ops, name)
        b = _device(ops, name)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert np.array_equal(a[2].view(np.int64), b[2].view(np.int64))
        n = _device(ops, name, return_affinity=False)
        assert n[2] is None and np.array_equal(n[0], a[0]) and np.array_equal(n[1], a[1])


def test_argument_errors(ops):
    from mvpose import _lib
    cams, k, ci, _ = cases.gpu_cases()["nv2_P3_T67"]
    cams_d = torch.tensor(ops.pack_cameras(syn.reference_camera_params(cams)), device="cuda")
    kd = torch.tensor(k[:4], device="cuda")
    for kw, what in ((dict(cam_idx=(0,)), "n_cam_idx"), (dict(cam_idx=(0, 2)), "cam_idx"),
                     (dict(cam_idx=(0, 1), max_cost_px=20.0), "max_cost_px"),
                     (dict(cam_idx=(0, 1), max_cost_px=0.0), "max_cost_px"),
                     (dict(cam_idx=(0, 1), trunc_px=float("inf")), "trunc_px"),
                     (dict(cam_idx=(0, 1), min_joints=0), "min_joints"),
                     (dict(cam_idx=(0, 1), min_joints=18), "min_joints"),
                     (dict(cam_idx=(0, 1), min_conf=float("nan")), "min_conf")):
        with pytest.raises(_lib.MvposeError, match=what):
            ops.associate_views(kd, cams_d, **kw)
    with pytest.raises(_lib.MvposeError, match="P="):
        ops.associate_views(torch.zeros((1, 33, 17, 3, 2), device="cuda"), cams_d, (0, 1))
    with pytest.raises(ValueError):
        ops.associate_views(kd[0], cams_d, (0, 1))
    with pytest.raises(TypeError):
        ops.associate_views(kd.double(), cams_d, (0, 1))
    # a short workspace is refused before any launch
    group = torch.full((4, 2, 3), 7, dtype=torch.int8, device="cuda")
    count = torch.full((4, 2), 7, dtype=torch.uint8, device="cuda")
    work = torch.empty(64, dtype=torch.uint8, device="cuda")
    ci2 = (_lib.c_int * 2)(0, 1)
    rc = _lib.lib.mvp_associate_views(kd.data_ptr(), 4, 3, 17, 2, cams_d.data_ptr(), 2, ci2, 2, 0.0, 20.0, 8.0, 5,
                                      work.data_ptr(), 64, group.data_ptr(), count.data_ptr(), None, None)
    torch.cuda.synchronize()
    assert rc == -1 and "workspace_bytes" in _lib.last_error() and (group == 7).all() and (count == 7).all()
