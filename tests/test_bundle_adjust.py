"""CPU: the bundle adjustment's restatement (tests/ba_ref.py) is checked against finite differences
of synthetic.project and against the rig it has to recover; the comparisons its runs make have the
margins that let the GPU tests demand equal trial counts; the C-ABI entries are declared, exported
and refuse bad arguments before any device work."""
import ctypes

import numpy as np
import pytest

import ba_cases
import ba_ref
import tri_refine_ref as tr
from mvpose import synthetic as syn


def rot_err_deg(Ra, Rb):
    return float(np.rad2deg(np.arccos(np.clip((np.trace(Ra @ Rb.T) - 1.0) / 2.0, -1.0, 1.0))))


def test_jacobians_match_central_differences():
    """J_X against X ± h, J_c against the camera perturbed by ± h along each of (dw, du): relative
    1e-6 of the largest entry of the Jacobian's column."""
    cams = syn.make_rig(4, seed=3)
    X = syn.make_poses(3, seed=1).reshape(-1, 3)
    for cam in cams:
        JX, Jc, Pz = ba_ref.jacobians(X, cam)
        assert (Pz > 0).all()
        for k in range(3):
            # truncation h²·|pi'''|/6 and rounding eps·|pi|/h balance near h = 1e-4 (tri_refine's test)
            e = np.zeros(3)
            e[k] = 1e-4
            fd = (syn.project(X + e, cam) - syn.project(X - e, cam)) / 2e-4
            assert np.abs(JX[:, :, k] - fd).max() <= 1e-6 * np.abs(fd).max()
        for k in range(6):
            # rotations move a pixel by ~1000 px/rad: h = 1e-6 rad keeps both error terms ~1e-9 of it
            h = 1e-6 if k < 3 else 1e-4
            e = np.zeros(6)
            e[k] = h
            fd = (syn.project(X, ba_ref.perturb(cam, e)) - syn.project(X, ba_ref.perturb(cam, -e))) / (2 * h)
            assert np.abs(Jc[:, :, k] - fd).max() <= 1e-6 * np.abs(fd).max()


def test_reduced_system_equals_the_dense_normal_equations():
    """S and b of the restatement against the Schur complement of the dense (6F + 3n) normal
    equations built from the stacked Jacobian, on a small case."""
    case = ba_cases.system_case(3, [1, 2], 12, dirty=False)
    used, z, W = tr.views(case["kpts"], case["cam_idx"], None, tr.W_UNIT, None, 0.0, 1.0)
    X = case["xyz"].astype(np.float64)
    act = ba_ref.active_points(X, case["cams"], case["cam_idx"], used)
    assert act.all()
    lin = ba_ref.system(X, case["cams"], case["cams"], case["cam_idx"], case["free"], act, used, z, W, 0.0, 0.0, 0.0)
    n, F = X.shape[0], 2
    Jd = np.zeros((2 * 3 * n, 6 * F + 3 * n))
    r = np.zeros(2 * 3 * n)
    for i, col in enumerate(case["cam_idx"]):
        JX, Jc, _ = ba_ref.jacobians(X, case["cams"][col])
        for p in range(n):
            row = 2 * (i * n + p)
            Jd[row:row + 2, 6 * F + 3 * p:6 * F + 3 * p + 3] = JX[p]
            if i in case["free"]:
                k = 6 * case["free"].index(i)
                Jd[row:row + 2, k:k + 6] = Jc[p]
            r[row:row + 2] = syn.project(X[p:p + 1], case["cams"][col])[0] - z[p, i]
    H, g = Jd.T @ Jd, Jd.T @ r
    A, B, C = H[:6 * F, :6 * F], H[:6 * F, 6 * F:], H[6 * F:, 6 * F:]
    S = A - B @ np.linalg.solve(C, B.T)
    b = -(g[:6 * F] - B @ np.linalg.solve(C, g[6 * F:]))
    np.testing.assert_allclose(lin["S"], S, rtol=0, atol=1e-9 * np.abs(S).max())
    np.testing.assert_allclose(lin["b"], b, rtol=0, atol=1e-9 * np.abs(b).max())


def test_recovers_perturbed_cameras_with_two_fixed():
    """make_rig(4), 120 frames (2 040 points), 0.5 px noise, cameras 2 and 3 off by 1 degree and 3 cm,
    cameras 0 and 1 fixed, seeds triangulated with the perturbed cameras: rotation and translation
    errors after the adjustment are below a tenth of the planted ones.  The committed restatement
    measures 0.018 / 0.025 degrees and 0.12 / 0.14 cm."""
    rc = ba_cases.recovery()
    out = ba_ref.bundle_adjust(rc["kpts"], rc["cams"], [0, 1, 2, 3], [2, 3], rc["xyz0"], max_iter=30, tol=1e-6)
    assert out["info"][4] == 0 and out["info"][6] == 2040
    assert out["info"][1] < out["info"][0]
    for v in (2, 3):
        rot = rot_err_deg(out["cams"][v]["R"], rc["true"][v]["R"])
        tra = float(np.linalg.norm(out["cams"][v]["T"] - rc["true"][v]["T"]))
        print(f"camera {v}: rotation error {rot:.4f} deg (planted 1), translation error {tra:.4f} cm (planted 3)")
        assert rot < 0.1 and tra < 0.3
    for v in (0, 1):
        assert np.array_equal(out["cams"][v]["R"], rc["cams"][v]["R"]) and np.array_equal(out["cams"][v]["T"], rc["cams"][v]["T"])
    assert np.allclose(out["cov"], out["cov"].T, rtol=1e-9, atol=0) and (np.diag(out["cov"]) > 0).all()


def test_single_fixed_camera_with_translation_prior():
    rc = ba_cases.recovery()
    out = ba_ref.bundle_adjust(rc["kpts"], rc["cams"], [0, 1, 2, 3], [1, 2, 3], rc["xyz0"], trans_prior_sigma=3.0,
                               max_iter=30, tol=1e-6)
    assert out["info"][4] == 0
    assert out["info"][1] < out["info"][0]


def test_starved_free_view_and_zero_trials():
    rc = ba_cases.recovery()
    kp = rc["kpts"][:34].copy()
    kp[2:, 0, 3] = np.nan       # view 3 keeps two observations
    out = ba_ref.bundle_adjust(kp, rc["cams"], [0, 1, 2, 3], [2, 3], rc["xyz0"][:34])
    assert out["info"][4] == 3 and out["info"][2] == 0
    assert np.array_equal(out["xyz"], rc["xyz0"][:34])
    out = ba_ref.bundle_adjust(rc["kpts"][:34], rc["cams"], [0, 1, 2, 3], [2, 3], rc["xyz0"][:34], max_iter=0)
    assert out["info"][4] == 1 and out["info"][0] == out["info"][1] and np.array_equal(out["xyz"], rc["xyz0"][:34])


@pytest.mark.parametrize("name", sorted(ba_cases.RUNS))
def test_gpu_runs_have_margins(name):
    """Every accept / reject and stop comparison of the runs the GPU tests compare has a relative
    margin >= 1e-7, and no Huber residual lies within 1e-6 of delta."""
    out = ba_cases.reference_run(name)
    print(name, "margins", ["%.3g" % m for m in out["margins"]], "huber gap", out["huber_gap"])
    assert out["info"][4] == 0 and out["info"][1] < out["info"][0]
    assert min(out["margins"]) >= 1e-7
    assert out["huber_gap"] >= 1e-6


def test_rough_run_rejects_trials_with_margins():
    """The run that exercises rejection (ba_cases.rough): some trials rejected, some seeds inactive,
    every comparison with a relative margin >= 1e-7."""
    out = ba_cases.rough_reference_run()
    print("rough: info", out["info"].tolist(), "smallest margin", min(out["margins"]))
    assert out["info"][2] == 12 and 0 < out["info"][3] < 12 and out["info"][4] == 1
    assert out["info"][6] < 340
    assert min(out["margins"]) >= 1e-7


def test_gpu_system_cases_keep_huber_residuals_off_the_threshold():
    for kw in ba_cases.SYSTEM_CASES:
        if kw.get("hub", 0.0) > 0:
            case = ba_cases.system_case(**ba_cases.case_args(kw))
            gap = ba_cases.reference_system(case, kw.get("lam", 0.0), kw["hub"], kw.get("sigma", 0.0))[5]
            assert gap >= 1e-6, (kw, gap)


def test_entry_points_are_declared_and_refuse_bad_arguments():
    from mvpose import _lib
    for s in ("mvp_bundle_adjust_plan", "mvp_bundle_adjust_system", "mvp_bundle_adjust"):
        assert s in _lib.SIGNATURES and hasattr(_lib.lib, s)
    nbytes = ctypes.c_int64(0)
    _lib.call("mvp_bundle_adjust_plan", 2040, 4, 0b1100, ctypes.byref(nbytes))
    assert nbytes.value > 2040 * 48
    for n, nv, fm, word in ((2040, 4, 0b10000, "free_mask"), (2040, 4, 0b1111, "fixed"), (2040, 4, 0, "free_mask"),
                            (0, 4, 0b10, "n_points"), (10, 9, 0b10, "n_cam_idx")):
        with pytest.raises(_lib.MvposeError, match=word):
            _lib.call("mvp_bundle_adjust_plan", n, nv, fm, ctypes.byref(nbytes))
    ci = (ctypes.c_int * 4)(0, 1, 2, 3)
    base = [None, 100, 4, None, 4, ci, 4, 0b1100, None, None, 0, None, 0, 0.0, 1.0, 0.0, 0.0]
    with pytest.raises(_lib.MvposeError, match="workspace_bytes"):
        _lib.call("mvp_bundle_adjust", *base, 30, 1e-6, None, 16, None, None, None, None, None, None)
    with pytest.raises(_lib.MvposeError, match="max_iter"):
        _lib.call("mvp_bundle_adjust", *base, 64, 1e-6, None, 1 << 30, None, None, None, None, None, None)
    with pytest.raises(_lib.MvposeError, match="tol"):
        _lib.call("mvp_bundle_adjust", *base, 30, float("nan"), None, 1 << 30, None, None, None, None, None, None)
    with pytest.raises(_lib.MvposeError, match="null device pointer"):
        _lib.call("mvp_bundle_adjust", *base, 30, 1e-6, None, 1 << 30, None, None, None, None, None, None)
    bad = list(base)
    bad[15] = float("nan")
    with pytest.raises(_lib.MvposeError, match="huber_delta"):
        _lib.call("mvp_bundle_adjust_system", *bad, 0.0, None, 1 << 30, None, None, None, None, None)
    with pytest.raises(_lib.MvposeError, match="lambda"):
        _lib.call("mvp_bundle_adjust_system", *base, -1.0, None, 1 << 30, None, None, None, None, None)


def test_refine_extrinsics_explains_the_scale():
    from mvpose import calib
    rc = ba_cases.recovery()
    params = syn.reference_camera_params(rc["cams"])
    with pytest.raises(ValueError, match="scale"):
        calib.refine_extrinsics(rc["kpts4"], params)
    with pytest.raises(ValueError, match="stay fixed"):
        calib.refine_extrinsics(rc["kpts4"], params, free=[0, 1, 2, 3], trans_prior_sigma=3.0)
