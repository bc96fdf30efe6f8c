"""CPU: the maximum-likelihood refinement's restatement (tests/tri_refine_ref.py) is checked against
finite differences, scipy's Levenberg-Marquardt and the statistics it promises; the C-ABI entry
(mvp_triangulate_refine) is declared and exported and rejects bad arguments before any device
work; the Python / command-line fronts accept the new options and reject bad ones."""
import ctypes
import os
import re

import numpy as np
import pytest

import tri_refine_ref as ref
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "mvpose.h")


@pytest.fixture(scope="module")
def hetero():
    """The heteroscedastic inputs at V = 4, their DLT seed and the restatement's refinement with
    the true covariances (cov_floor = 0)."""
    cams, gt, kpts, gauss = ref.hetero_inputs(4)
    idx = [0, 1, 2, 3]
    seed = ref.dlt_seed(kpts, cams, idx)
    n = seed.shape[0]
    r = ref.refine(kpts.reshape(n, 3, 4), cams, idx, seed, weights=ref.W_GAUSS, gauss=gauss, cov_floor=0.0)
    return cams, gt, kpts, gauss, seed, r


def test_analytic_jacobian_matches_central_differences():
    from mvpose import synthetic as syn
    cams = syn.make_rig(4, seed=3)
    X = syn.make_poses(3, seed=1).reshape(-1, 3)
    h = 1e-4
    for cam in cams:
        J, Pz = ref.jacobian(X, cam)
        assert (Pz > 0).all()
        for k in range(3):
            e = np.zeros(3)
            e[k] = h
            fd = (syn.project(X + e, cam) - syn.project(X - e, cam)) / (2 * h)
            # truncation h²·|π'''|/6 ~ 1e-8·(f/Z³) and rounding eps·|π|/h ~ 2e-9 px/cm, on |J| ~ 3 px/cm
            np.testing.assert_allclose(J[:, :, k], fd, rtol=0, atol=1e-6)


def test_minimiser_agrees_with_scipy_lm(hetero):
    """scipy.optimize.least_squares(method="lm") on the whitened residuals L_iᵀ r_i (W_i = L_i L_iᵀ),
    from the same seed: the two minimisers agree to 1e-5 world units."""
    from scipy.optimize import least_squares
    from mvpose import synthetic as syn
    cams, gt, kpts, gauss, seed, r = hetero
    n = seed.shape[0]
    used, z, W = ref.views(kpts.reshape(n, 3, 4), [0, 1, 2, 3], None, ref.W_GAUSS, gauss, 0.0, 0.0)
    assert used.all()
    worst = 0.0
    for p in range(0, n, 5):
        Ls = [np.linalg.cholesky(W[p, i]) for i in range(4)]

        def res(X):
            return np.concatenate([Ls[i].T @ (syn.project(X[None], cams[i])[0] - z[p, i]) for i in range(4)])
        sol = least_squares(res, seed[p].astype(np.float64), method="lm", xtol=1e-14, ftol=1e-14, gtol=1e-14)
        worst = max(worst, np.abs(sol.x - r["X"][p]).max())
        np.testing.assert_allclose(0.5 * np.sum(sol.fun ** 2), r["cost"][p], rtol=1e-5)
    print(f"largest |restatement - scipy lm| = {worst:.3g} world units")
    assert worst <= 1e-5


def test_weighted_refinement_beats_the_dlt_on_heteroscedastic_views(hetero):
    """rms error of the refined points < 0.75 x the DLT seed's at V = 4 (204 points, per-view noise
    covariances with eigenvalues in {1, 4, 64} px²).  The committed restatement measures
    1.895 cm -> 0.872 cm, ratio 0.460; every point converges, in at most 4 trials."""
    cams, gt, kpts, gauss, seed, r = hetero
    assert seed.shape[0] == 204
    rms0 = np.sqrt(((seed - gt) ** 2).sum(1).mean())
    rms1 = np.sqrt(((r["X"] - gt) ** 2).sum(1).mean())
    print(f"rms DLT {rms0:.4f} refined {rms1:.4f} ratio {rms1 / rms0:.4f} trials max {(r['status'] & 63).max()}")
    assert (r["status"] & (ref.FAILED | ref.NOT_CONVERGED) == 0).all()
    assert rms1 < 0.75 * rms0


def test_covariance_is_calibrated(hetero):
    """mean (X - gt)ᵀ cov⁻¹ (X - gt) in [2.4, 3.6]: chi² with 3 degrees of freedom, n = 204, standard
    error 0.17.  The committed restatement measures 2.98."""
    cams, gt, kpts, gauss, seed, r = hetero
    d = r["X"] - gt
    m = np.einsum("ni,nij,nj->n", d, r["H"], d).mean()       # cov⁻¹ = H
    print(f"mean Mahalanobis² = {m:.3f}")
    assert 2.4 <= m <= 3.6
    # and the reported cov is H⁻¹, symmetric positive definite
    cov = r["cov"][:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3).astype(np.float64)
    np.testing.assert_allclose(np.einsum("nij,njk->nik", cov, r["H"]), np.broadcast_to(np.eye(3), cov.shape),
                               rtol=0, atol=1e-5)


def test_equal_isotropic_noise_gives_no_gain():
    """With the same isotropic noise in every view the refinement does not beat the DLT by more
    than a few per cent either way: the value is in the weighting, not in 'geometric'."""
    from mvpose import synthetic as syn
    cams = syn.make_rig(4, seed=3)
    gt = syn.make_poses(12, seed=7)
    kpts = syn.make_kpts_2d(gt, cams, seed=5, noise_px=1.0)
    seed = ref.dlt_seed(kpts, cams, [0, 1, 2, 3])
    r = ref.refine(kpts.reshape(-1, 3, 4), cams, [0, 1, 2, 3], seed)
    rms0 = np.sqrt(((seed - gt.reshape(-1, 3)) ** 2).sum(1).mean())
    rms1 = np.sqrt(((r["X"] - gt.reshape(-1, 3)) ** 2).sum(1).mean())
    print(f"isotropic: DLT {rms0:.4f} refined {rms1:.4f}")
    assert abs(rms1 / rms0 - 1) < 0.05


def test_failures_keep_the_seed():
    from mvpose import synthetic as syn
    cams = syn.make_rig(3, seed=3)
    gt = syn.make_poses(1, seed=2)
    kpts = syn.make_kpts_2d(gt, cams, seed=5).reshape(17, 3, 3)
    seed = gt.reshape(17, 3).astype(np.float32)
    kpts[0, 0, 0] = np.nan
    kpts[0, 0, 1] = np.nan                      # one view left
    seed[1] = [0.0, 0.0, -500.0]                # behind camera 0
    seed[2, 1] = np.nan
    r = ref.refine(kpts, cams, [0, 1, 2], seed)
    assert list(r["status"][:3]) == [0x80, 0x80, 0x80]
    assert np.array_equal(r["xyz"][:3].view(np.uint32), seed[:3].view(np.uint32))
    assert np.isnan(r["cov"][:3]).all() and np.isnan(r["cost"][:3]).all()
    assert (r["status"][3:] & 0xC0 == 0).all()
    r0 = ref.refine(kpts, cams, [0, 1, 2], seed, max_iter=0)
    assert (r0["status"][3:] == 0x40).all()
    assert np.array_equal(r0["xyz"], seed, equal_nan=True) and np.isfinite(r0["cov"][3:]).all()


# ------------------------------------------------------------------ the C-ABI entry
def test_header_declares_and_library_exports():
    from mvpose import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+mvp_triangulate_refine\s*\(", src)
    assert hasattr(_lib.lib, "mvp_triangulate_refine")
    assert "mvp_triangulate_refine" in _lib.SIGNATURES
    for name, val in (("MVP_REFINE_W_UNIT", 0), ("MVP_REFINE_W_CONF", 1), ("MVP_REFINE_W_GAUSS", 2)):
        assert re.search(rf"#define\s+{name}\s+{val}\b", src)


def _call(n=10, V=2, n_cams=2, idx=(0, 1), weights=0, gauss=None, J=0, min_conf=0.0, cov_floor=1.0, max_iter=10,
          tol=1e-7):
    from mvpose import _lib
    ci = (ctypes.c_int * len(idx))(*idx)
    rc = _lib.lib.mvp_triangulate_refine(None, n, V, None, n_cams, ci, len(idx), None, None, weights, gauss, J,
                                         min_conf, cov_floor, max_iter, tol, None, None, None, None, None)
    return rc, _lib.last_error()


@pytest.mark.parametrize("kw,msg", [
    (dict(idx=[0]), "n_cam_idx=1"),
    (dict(idx=[0, 5]), "cam_idx[1]=5"),
    (dict(idx=[0, -1]), "cam_idx[1]=-1"),
    (dict(weights=3), "weights=3"),
    (dict(weights=-1), "weights=-1"),
    (dict(weights=2), "needs gauss_dev"),
    (dict(weights=2, gauss=ctypes.c_void_p(64), J=0), "J=0"),
    (dict(weights=2, gauss=ctypes.c_void_p(64), J=3), "J=3"),
    (dict(min_conf=float("nan")), "min_conf"),
    (dict(cov_floor=-1.0), "cov_floor"),
    (dict(cov_floor=float("nan")), "cov_floor"),
    (dict(max_iter=-1), "max_iter=-1"),
    (dict(max_iter=64), "max_iter=64"),
    (dict(tol=0.0), "tol"),
    (dict(tol=float("inf")), "tol"),
    (dict(tol=float("nan")), "tol"),
])
def test_bad_arguments_are_reported(kw, msg):
    """Every check runs before any device work (the device pointers are NULL or never read)."""
    rc, err = _call(**kw)
    assert rc == -1
    assert msg in err, err


def test_null_pointers_and_empty_batch():
    rc, err = _call()
    assert rc == -1 and "null device pointer" in err
    rc, _ = _call(n=0)                           # n_points == 0 returns OK before the pointer checks
    assert rc == 0
    rc, err = _call(n=-1)
    assert rc == -1 and "n_points < 0" in err


# ------------------------------------------------------------------ the fronts
def test_cli_parser_accepts_the_new_flags():
    from mvpose import cli
    p = cli.record_and_estimate_pose_parser(extensions=True)
    a = p.parse_args(["--camera_names", "a", "b", "c", "--refine", "heatmap", "--cov_floor", "0.5"])
    assert (a.refine, a.cov_floor) == ("heatmap", 0.5)
    d = p.parse_args(["--camera_names", "a", "b"])
    assert d.refine is None and d.cov_floor is None          # function defaults apply
    with pytest.raises(SystemExit):
        p.parse_args(["--camera_names", "a", "b", "--refine", "huber"])
    with pytest.raises(SystemExit):                           # the reference's own parser does not know them
        cli.record_and_estimate_pose_parser().parse_args(["--camera_names", "a", "b", "--refine", "unit"])
    with pytest.raises(ValueError):
        cli.record_and_estimate_pose(["a", "b"], configuration_number=1, recording_paths=["x.npy", "y.npy"],
                                     synchronize_video=False, refine="huber")


def test_heatmap_refinement_without_gaussians_raises():
    from mvpose import pose_estimation
    with pytest.raises(ValueError, match="heatmaps_2d"):
        pose_estimation.get_pose_3D({}, np.zeros((1, 17, 3, 2), np.float32), refine="heatmap")


def test_unknown_refine_values_raise():
    from mvpose import ops, pipeline, pose_estimation
    with pytest.raises(ValueError):
        pose_estimation.get_pose_3D({}, np.zeros((1, 17, 3, 2), np.float32), refine="huber")
    with pytest.raises(ValueError):
        pose_estimation.estimate_pose_from_video(["a", "b"], ["x", "y"], None, refine="huber")
    with pytest.raises(ValueError):
        pipeline.MultiViewPipeline({}, estimator=object(), refine="huber")
    assert (ops.REFINE_W_UNIT, ops.REFINE_W_CONF, ops.REFINE_W_GAUSS) == (0, 1, 2)
