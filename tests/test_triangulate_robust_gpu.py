"""GPU: robust N-view triangulation (mvp_triangulate_robust) vs a numpy restatement of its
algorithm built from the oracle's leaves.

The reference follows steps A and B of include/mvpose.h exactly (OpenCV-semantics undistortion
and Jacobi-SVD DLT from oracle/cv_ref for every solve that reaches the output, np.linalg.svd for
the pair hypotheses, which only select).  Masks depend on comparisons `error <= inlier_px`; the
reference records the smallest |error - inlier_px| it ever compares and every test asserts it is
> 1e-6 px: the two fp64 evaluations (device Jacobi vs LAPACK, different summation orders) differ
by ~1e-9 px at these magnitudes, so only then are the masks determined whatever the rounding
order.  Given equal masks the float32 points must be BIT-identical (the final solve is the
oracle's DLT over exactly the masked views) and the errors agree to rtol 1e-6 + atol 1e-6 px
(fp64 evaluation differences ~1e-9 px, the f32 store 6e-8 relative)."""
import numpy as np
import pytest
import torch

from oracle import cv_ref
from mvpose import synthetic as syn

pytestmark = pytest.mark.gpu
INLIER_PX = 10.0
MIN_MARGIN = 1e-6


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mvpose import ops as _ops
    return _ops


# ------------------------------------------------------------------ numpy reference
class Reference:
    """Steps A and B over the listed views `ci` of kpts (..., 3, V) float32."""

    def __init__(self, cams, ci):
        self.ci = list(ci)
        self.cams = [cams[c] for c in self.ci]
        self.P = np.stack([cv_ref.projection_matrix(c["K"], c["R"], c["T"]) for c in self.cams]).astype(np.float64)
        self.margin = np.inf          # smallest |error - inlier_px| ever compared

    def _dlt(self, und, views):
        xs = [np.ascontiguousarray(und[v].reshape(2, 1)) for v in views]
        X4 = cv_ref.triangulate_nview_cv([self.P[v] for v in views], xs)
        return cv_ref.convert_points_from_homogeneous(X4.T).reshape(3)

    def _errors(self, X, und, valid):
        """fp64 reprojection error of every valid view against homogeneous X; NaN for invalid."""
        e = np.full(len(self.ci), np.nan)
        for v in np.flatnonzero(valid):
            q = self.P[v] @ X
            if q[2] * X[3] > 0:
                with np.errstate(all="ignore"):
                    e[v] = np.hypot(q[0] / q[2] - np.float64(und[v, 0]), q[1] / q[2] - np.float64(und[v, 1]))
            else:
                e[v] = np.inf
        return e

    def _inliers(self, e, valid, inlier_px):
        fin = np.isfinite(e) & valid
        if fin.any():
            self.margin = min(self.margin, float(np.min(np.abs(e[fin] - inlier_px))))
        with np.errstate(invalid="ignore"):
            return valid & (e <= inlier_px)

    def __call__(self, kpts, inlier_px=INLIER_PX, min_conf=0.0):
        kpts = np.asarray(kpts, np.float32)
        lead = kpts.shape[:-2]
        k = kpts.reshape(-1, 3, kpts.shape[-1])[:, :, self.ci]          # (n, 3, NV)
        n, nv = k.shape[0], len(self.ci)
        und = np.empty((n, nv, 2), np.float32)
        for v, c in enumerate(self.cams):
            pts = np.ascontiguousarray(k[:, :2, v].reshape(n, 1, 2))
            und[:, v] = cv_ref.undistort_points(pts, c["K"], c["dist"], None, c["K"])[:, 0, :]
        with np.errstate(invalid="ignore"):
            valid = (np.isfinite(k[:, 0]) & np.isfinite(k[:, 1]) & ~np.isnan(k[:, 2]) & (k[:, 2] >= np.float32(min_conf))
                     & np.isfinite(und).all(-1))
        xyz = np.full((n, 3), np.nan, np.float32)
        mask = np.zeros((n, nv), bool)
        err = np.full((n, nv), np.nan, np.float32)
        inl = float(np.float32(inlier_px))
        for p in range(n):
            vd = valid[p]
            views = list(np.flatnonzero(vd))
            if len(views) < 2:
                continue
            # step A
            x = self._dlt(und[p], views)
            e = self._errors(np.array([x[0], x[1], x[2], 1.0], np.float64), und[p], vd)
            if self._inliers(e, vd, inl)[vd].all():
                xyz[p], mask[p], err[p] = x, vd, e.astype(np.float32)
                continue
            # step B
            best = (-1, np.float32(0), None)
            for ia, a in enumerate(views):
                for b in views[ia + 1:]:
                    rows = []
                    for v in (a, b):
                        ux, uy = np.float64(und[p, v, 0]), np.float64(und[p, v, 1])
                        rows += [ux * self.P[v][2] - self.P[v][0], uy * self.P[v][2] - self.P[v][1]]
                    X = np.linalg.svd(np.stack(rows))[2][3]
                    m = self._inliers(self._errors(X, und[p], vd), vd, inl)
                    s = np.float32(0)
                    for v in np.flatnonzero(m):                          # f32, ascending view position
                        s = np.float32(s + k[p, 2, v])
                    cnt = int(m.sum())
                    if cnt > best[0] or (cnt == best[0] and s > best[1]):
                        best = (cnt, s, m)
            if best[0] < 2:
                continue
            x = self._dlt(und[p], list(np.flatnonzero(best[2])))
            e = self._errors(np.array([x[0], x[1], x[2], 1.0], np.float64), und[p], vd)
            xyz[p], mask[p], err[p] = x, best[2], e.astype(np.float32)
        return xyz.reshape(lead + (3,)), mask.reshape(lead + (nv,)), err.reshape(lead + (nv,))


def _bits_equal(out, ref):
    """Bit-identical float32 (NaN where the reference is NaN)."""
    assert out.shape == ref.shape and out.dtype == ref.dtype
    same = (out == ref) | (np.isnan(out) & np.isnan(ref))
    assert same.all(), (f"{(~same).sum()} of {same.size} outputs differ from the reference, max |d| "
                        f"{np.nanmax(np.abs(out - ref)):.3g}")


def _device(ops, cams, k, ci, **kw):
    cams_d = torch.tensor(ops.pack_cameras(syn.reference_camera_params(cams)), device="cuda")
    kd = torch.tensor(np.ascontiguousarray(k), device="cuda")
    xyz, inl, err = ops.triangulate_robust(kd, cams_d, ci, **kw)
    torch.cuda.synchronize()
    assert xyz.dtype == torch.float32 and inl.dtype == torch.bool and err.dtype == torch.float32
    return xyz.cpu().numpy(), inl.cpu().numpy(), err.cpu().numpy()


def _all_views(ops, cams, k, ci):
    cams_d = torch.tensor(ops.pack_cameras(syn.reference_camera_params(cams)), device="cuda")
    kd = torch.tensor(np.ascontiguousarray(k), device="cuda")
    return ops.triangulate(kd, cams_d, ci, mode=ops.TRI_ALL_VIEWS).cpu().numpy()


def _compare(ops, cams, k, ci, **kw):
    """Device vs reference on the same input: margin, masks, bits, errors.  Returns both."""
    ref = Reference(cams, ci)
    rx, rm, re = ref(k, **kw)
    print(f"reference: smallest |error - inlier_px| compared {ref.margin:.3g} px")
    assert ref.margin > MIN_MARGIN, ref.margin
    dx, dm, de = _device(ops, cams, k, ci, **kw)
    assert np.array_equal(dm, rm), f"{(dm != rm).any(-1).sum()} masks differ"
    _bits_equal(dx, rx)
    np.testing.assert_allclose(de, re, rtol=1e-6, atol=1e-6, equal_nan=True)
    return (dx, dm, de), (rx, rm, re)


def contaminated(V, seed, max_bad, frames=30):
    """make_rig(V, seed) / make_poses(frames, seed + 10) / 1 px noise; per point 0..max_bad views
    pushed 80-300 px in a random direction.  Returns cams, kpts (frames, 17, 3, V), truth mask."""
    cams = syn.make_rig(V, seed=seed)
    k = syn.make_kpts_2d(syn.make_poses(frames, seed=seed + 10), cams, seed=seed + 20, noise_px=1.0)
    rng = np.random.default_rng(seed + 30)
    T, J = k.shape[:2]
    truth = np.ones((T, J, V), bool)
    for t in range(T):
        for j in range(J):
            bad = rng.choice(V, size=rng.integers(0, max_bad + 1), replace=False)
            for v in bad:
                r, th = rng.uniform(80.0, 300.0), rng.uniform(0.0, 2 * np.pi)
                k[t, j, 0, v] += np.float32(r * np.cos(th))
                k[t, j, 1, v] += np.float32(r * np.sin(th))
                truth[t, j, v] = False
    return cams, k, truth


# ------------------------------------------------------------------ 1. contaminated rigs
@pytest.mark.parametrize("V,seed", [(3, 1), (4, 2), (8, 3)])
def test_masks_and_bits(ops, V, seed):
    """510 points (two blocks with a tail), 0..m views per point displaced by 80-300 px (m = 1
    for V = 3 and 4, 3 for V = 8).  V = 3: the displaced view's confidence is 0.05, so the pair
    made of the two clean views wins the confidence tie-break over a pair holding the displaced
    one.  Masks equal the reference's and the ground truth, xyz bit-identical, errors within
    rtol 1e-6 + atol 1e-6 px; uncontaminated points equal the all-views DLT bit for bit."""
    cams, k, truth = contaminated(V, seed, max_bad=3 if V == 8 else 1)
    if V == 3:
        k[:, :, 2, :][~truth] = 0.05
    ci = list(range(V))
    (dx, dm, de), _ = _compare(ops, cams, k, ci, inlier_px=INLIER_PX)
    assert np.array_equal(dm, truth)
    assert np.isfinite(dx).all()
    clean = truth.all(-1)
    assert 0 < clean.sum() < clean.size
    _bits_equal(dx[clean], _all_views(ops, cams, k, ci)[clean])
    assert (de[truth] <= INLIER_PX).all() and (de[~truth] > INLIER_PX).all()


# ------------------------------------------------------------------ 2. V = 2
def test_two_views(ops):
    cams = syn.make_rig(2, seed=5)
    k = syn.make_kpts_2d(syn.make_poses(30, seed=6), cams, seed=7, noise_px=1.0)
    (dx, dm, de), _ = _compare(ops, cams, k, [0, 1])
    assert np.isfinite(dx).all() and dm.all()
    _bits_equal(dx, _all_views(ops, cams, k, [0, 1]))


def test_listed_subset_in_any_order(ops):
    """View i reads column cam_idx[i] with camera cam_idx[i]'s parameters."""
    cams, k, truth = contaminated(5, 9, max_bad=1, frames=8)
    ci = [4, 0, 2, 3]
    (dx, dm, _), _ = _compare(ops, cams, k, ci)
    assert np.array_equal(dm, truth[..., ci])


# ------------------------------------------------------------------ 3. validity
def test_validity(ops):
    cams, k, truth = contaminated(4, 11, max_bad=1, frames=16)     # 272 points: a block and a tail
    k[..., 2, :] = np.maximum(k[..., 2, :], 0.6)  # every confidence above min_conf = 0.5, except:
    k[0, 0, 0, 1] = np.nan                       # NaN x
    k[0, 1, 1, 2] = np.inf                       # Inf y
    k[0, 2, 2, 3] = np.nan                       # NaN confidence
    k[1, :, 2, 0] = 0.25                         # below min_conf
    k[2, 0, 0, :3] = np.nan                      # one valid view left
    k[2, 1, 2, :] = 0.1                          # none
    (dx, dm, de), _ = _compare(ops, cams, k, [0, 1, 2, 3], inlier_px=INLIER_PX, min_conf=0.5)
    assert not dm[0, 0, 1] and not dm[0, 1, 2] and not dm[0, 2, 3] and not dm[1, :, 0].any()
    assert np.isnan(de[0, 0, 1]) and np.isnan(de[1, :, 0]).all()
    for t, j in ((2, 0), (2, 1)):
        assert np.isnan(dx[t, j]).all() and not dm[t, j].any() and np.isnan(de[t, j]).all()
    assert np.isfinite(dx[3:]).all()


@pytest.mark.parametrize("n", [0, 1, 257])
def test_sizes(ops, n):
    cams, k, _ = contaminated(4, 13, max_bad=1, frames=16)
    k = np.ascontiguousarray(k.reshape(-1, 3, 4)[:n])
    if n == 0:
        dx, dm, de = _device(ops, cams, k, [0, 1, 2, 3])
        assert dx.shape == (0, 3) and dm.shape == (0, 4) and de.shape == (0, 4)
        return
    _compare(ops, cams, k, [0, 1, 2, 3])


# ------------------------------------------------------------------ 4. behind the camera
def test_behind_the_camera(ops):
    """3D points placed behind one or two cameras of a distortion-free rig: the pinhole projection
    mirrors them through the principal point, so the DLT over all views is algebraically
    consistent; those views are not inliers and report +inf."""
    cams = syn.make_rig(4, seed=21, distortion=False)
    rng = np.random.default_rng(22)
    pts = []
    for v in (1, 2, 3):
        c = -cams[v]["R"].T @ cams[v]["T"].reshape(3)
        for t in rng.uniform(0.1, 0.6, 40):
            pts.append(c + t * (c - syn.SUBJECT_CENTER) + rng.normal(0, 20.0, 3))
    pts = np.array(pts)
    depth = np.stack([(pts @ c["R"].T + c["T"].reshape(3))[:, 2] for c in cams], -1)      # (n, 4)
    keep = (np.abs(depth) > 30).all(-1) & ((depth > 0).sum(-1) >= 2) & ((depth < 0).sum(-1) >= 1)
    pts, depth = pts[keep], depth[keep]
    assert len(pts) >= 8
    k = np.empty((len(pts), 3, 4), np.float32)
    for v, c in enumerate(cams):
        k[:, :2, v] = syn.project(pts, c, distortion=False)
    k[:, 2, :] = 0.9
    (dx, dm, de), _ = _compare(ops, cams, k, [0, 1, 2, 3])
    assert np.array_equal(dm, depth > 0)
    assert np.isposinf(de[depth < 0]).all() and (de[depth > 0] < 0.1).all()
    np.testing.assert_allclose(dx, pts, rtol=0, atol=0.05)


# ------------------------------------------------------------------ 5. pipeline and drop-in
def test_get_pose_3D_methods(ops):
    from mvpose import pose_estimation as pe
    cams, k, truth = contaminated(4, 31, max_bad=1, frames=6)
    cp = syn.reference_camera_params(cams)
    dx, dm, de = _device(ops, cams, k, [0, 1, 2, 3], inlier_px=8.0, min_conf=0.1)
    out, info = pe.get_pose_3D(cp, k, camera_indices=[0, 1, 2, 3], method="robust", inlier_px=8.0, min_conf=0.1,
                               return_info=True)
    _bits_equal(out, dx)
    assert np.array_equal(info["inliers"], dm)
    np.testing.assert_array_equal(info["reproj_err"], de)
    _bits_equal(pe.get_pose_3D(cp, k, camera_indices=[0, 1, 2, 3], method="robust", inlier_px=8.0, min_conf=0.1), dx)
    av, av_info = pe.get_pose_3D(cp, k, camera_indices=[0, 1, 2, 3], method="all_views", return_info=True)
    _bits_equal(av, _all_views(ops, cams, k, [0, 1, 2, 3]))
    assert av_info["inliers"].all() and av_info["reproj_err"] is None
    # the default call is unchanged
    _bits_equal(pe.get_pose_3D(cp, k, camera_indices=[0, 1]), cv_ref.get_pose_3D(cp, k, camera_indices=[0, 1]))


@pytest.fixture(scope="module")
def project4(tmp_path_factory):
    """A project directory like tests/test_cli_gpu.py's, four cameras, with a pre-written
    kpts_2d.npy in the recordings folder (no backbone run needed)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mvpose import geometry
    root = tmp_path_factory.mktemp("proj4")
    cams, k, truth = contaminated(4, 41, max_bad=1, frames=6)
    ext = root / "configurations" / "1" / "extrinsic_camera_parameters"
    intr = root / "intrinsic_camera_parameters"
    names = ["camA", "camB", "camC", "camD"]
    for name, c in zip(names, cams):
        geometry.write_camera_parameters(name, c["K"], c["dist"], str(intr))
        geometry.write_rotation_translation(name, c["R"], c["T"], str(ext))
    geometry.save_camera_names(str(ext), dict(enumerate(names)), "camA")
    rec = root / "configurations" / "1" / "recordings" / "0"
    rec.mkdir(parents=True)
    np.save(rec / "kpts_2d.npy", k)
    paths = [str(rec / f"camera{v}.npy") for v in range(4)]
    return root, names, paths, k, truth


def _project_params(root, names):
    from mvpose import geometry
    ext = str(root / "configurations" / "1" / "extrinsic_camera_parameters")
    return ext, {i: geometry.get_params_from_name(n, extrinsic_params_dir=ext)[1] for i, n in enumerate(names)}


def test_estimate_pose_from_video(ops, project4, monkeypatch):
    from mvpose import pose_estimation as pe
    root, names, paths, k, truth = project4
    monkeypatch.chdir(root)
    ext, cp = _project_params(root, names)
    cams_d = torch.tensor(ops.pack_cameras(cp), device="cuda")
    kd = torch.tensor(k, device="cuda")
    k2, hm, k3, info = pe.estimate_pose_from_video(names, paths, None, extrinsic_params_dir=ext,
                                                   recompute_kpts_2d=False, triangulation="robust",
                                                   return_info=True)
    xyz, inl, err = ops.triangulate_robust(kd, cams_d, [0, 1, 2, 3])
    assert hm is None and np.array_equal(k2, k)
    _bits_equal(k3, xyz.cpu().numpy())
    assert np.array_equal(info["inliers"], inl.cpu().numpy()) and np.array_equal(info["inliers"], truth)
    np.testing.assert_array_equal(info["reproj_err"], err.cpu().numpy())
    r = pe.estimate_pose_from_video(names, paths, None, extrinsic_params_dir=ext, recompute_kpts_2d=False,
                                    triangulation="robust")
    assert len(r) == 3
    _bits_equal(r[2], k3)
    # the default method: cameras [0, 1], the reference's rule — what it returned before
    d = pe.estimate_pose_from_video(names, paths, None, extrinsic_params_dir=ext, recompute_kpts_2d=False)
    assert len(d) == 3
    _bits_equal(d[2], ops.triangulate(kd, cams_d, [0, 1]).cpu().numpy())
    _bits_equal(d[2], cv_ref.get_pose_3D(cp, k, camera_indices=[0, 1]))


def test_cli_writes_the_extra_files(ops, project4, monkeypatch):
    """record_and_estimate_pose --triangulation robust on four recordings (random weights, no
    detector): the reference's files plus kpts_3d_inliers.npy / kpts_3d_reproj_err.npy, equal to
    ops.triangulate_robust of the written kpts_2d.npy; the settings are in recording_log.yaml."""
    import yaml
    from mvpose import cli
    root, names, _, _, _ = project4
    monkeypatch.setenv("MVPOSE_RANDOM_WEIGHTS", "1")
    monkeypatch.setenv("MVPOSE_NO_DETECTOR", "1")
    monkeypatch.chdir(root)
    rec = root / "configurations" / "1" / "recordings" / "cli"
    rec.mkdir(parents=True)
    rng = np.random.default_rng(3)
    paths = []
    for v in range(4):
        np.save(rec / f"camera{v}.npy", rng.integers(0, 256, (3, 360, 640, 3), dtype=np.uint8))
        paths.append(str(rec / f"camera{v}.npy"))
    log = cli.record_and_estimate_pose_main(["--camera_names", *names, "--configuration_number", "1",
                                             "--recording_paths", *paths, "--triangulation", "robust",
                                             "--inlier_px", "25", "--min_confidence", "0.01"])
    with open(rec / "recording_log.yaml") as f:
        saved = yaml.safe_load(f)
    assert (saved["triangulation"], saved["inlier_px"], saved["min_confidence"]) == ("robust", 25.0, 0.01)
    k2 = np.load(log["kpts_2d"])
    assert k2.shape == (2, 17, 3, 4)
    _, cp = _project_params(root, names)
    xyz, inl, err = ops.triangulate_robust(torch.tensor(k2, device="cuda"),
                                           torch.tensor(ops.pack_cameras(cp), device="cuda"), [0, 1, 2, 3],
                                           inlier_px=25.0, min_conf=0.01)
    _bits_equal(np.load(log["kpts_3d"]), xyz.cpu().numpy())
    assert np.array_equal(np.load(log["kpts_3d_inliers"]), inl.cpu().numpy())
    np.testing.assert_array_equal(np.load(log["kpts_3d_reproj_err"]), err.cpu().numpy())


def test_pipeline_mode(ops):
    from mvpose import pipeline
    cams = syn.make_rig(3, seed=51)
    cp = syn.reference_camera_params(cams)
    p = pipeline.MultiViewPipeline(cp, camera_indices=(0, 1, 2), mode=ops.TRI_ROBUST, inlier_px=15.0, min_conf=0.05,
                                   max_frames=3, seed=0)
    frames = torch.tensor(syn.make_frames(3, seed=52).reshape(1, 3, 720, 1280, 3), device="cuda")
    out = p.process(frames)
    xyz, inl, err = ops.triangulate_robust(out["kpts_2d"], p.cams, [0, 1, 2], inlier_px=15.0, min_conf=0.05)
    assert out["kpts_3d"].shape == (1, 17, 3) and out["tri_inliers"].shape == (1, 17, 3)
    _bits_equal(out["kpts_3d"].cpu().numpy(), xyz.cpu().numpy())
    assert torch.equal(out["tri_inliers"], inl)
    np.testing.assert_array_equal(out["tri_reproj_err"].cpu().numpy(), err.cpu().numpy())


# ------------------------------------------------------------------ 6. stream
def test_non_default_stream(ops):
    cams, k, _ = contaminated(4, 61, max_bad=1, frames=16)
    cams_d = torch.tensor(ops.pack_cameras(syn.reference_camera_params(cams)), device="cuda")
    kd = torch.tensor(k, device="cuda")
    a = ops.triangulate_robust(kd, cams_d, [0, 1, 2, 3])
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        b = ops.triangulate_robust(kd, cams_d, [0, 1, 2, 3])
    st.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.uint8) if x.dtype != torch.bool else x,
                           y.view(torch.uint8) if y.dtype != torch.bool else y)
