"""The fit scene of the trajectory-covariance tests (tests/test_trajectory_cov.py,
tests/test_trajectory_cov_gpu.py), from mvpose.synthetic.  Nothing here touches the device."""
import functools

import numpy as np

import traj_fit_cases as tc
import tri_refine_ref as tr  # noqa: F401  (the tests read the weight constants through this module)
from mvpose import synthetic as syn

FIT_T = 40
FIT_JOINTS = (0, 5, 9, 15)     # of make_poses; the scene's chains 0..3
FIT_LOST = (2, 3)              # chains camera 1 loses ...
FIT_GAP = (14, 26)             # ... in these frames
FIT_LAMBDA = 0.25              # fit_trajectory's docstring: the prior under which the depth "wanders"
FIT_HUBERS = (0.0, 3.0)
FIT_EDGE = 2                   # stretch frames this close to a two-view frame have their depth held by it


@functools.lru_cache(maxsize=None)
def fit_scene():
    """The two-camera rig of traj_fit_cases.gap_scene at 40 frames and four joints, 1 px noise;
    camera 1 loses chains FIT_LOST over FIT_GAP.  Returns dict: cams, kpts (T, 4, 3, 2) f32, gauss
    (T, 2, 4, 6), xyz0 (T, 4, 3) f32 (the truth with 2 cm of noise), truth."""
    cams = syn.make_rig(2)
    truth = syn.make_poses(FIT_T, seed=0, jitter=0.0)[:, list(FIT_JOINTS)]
    kpts = syn.make_kpts_2d(truth, cams, seed=1, noise_px=1.0)
    rng = np.random.default_rng(5)
    gauss = tc.make_gauss(kpts, rng)
    gauss[..., 2:] *= 0.25       # sharp peaks, variances 0.25..2.25 px²: the views weigh about what "conf" gives them
    kpts[FIT_GAP[0]:FIT_GAP[1], list(FIT_LOST), :2, 1] = np.nan
    gauss[FIT_GAP[0]:FIT_GAP[1], 1, list(FIT_LOST)] = 0.0        # an empty heatmap's record
    xyz0 = (truth + rng.normal(0.0, 2.0, truth.shape)).astype(np.float32)
    return {"cams": cams, "kpts": np.ascontiguousarray(kpts), "gauss": gauss, "xyz0": xyz0, "truth": truth}


def stretch_figures(diag, xyz, cam):
    """Of one chain's Σ_tt (T, 3, 3) at the state xyz (T, 3): per frame of FIT_GAP the angle in degrees
    between the largest axis and the camera's ray through the joint, and the largest eigenvalue over
    the largest of all two-view frames."""
    w, v = np.linalg.eigh(np.asarray(diag, np.float64))
    centre = -(cam["R"].T @ cam["T"].reshape(3))
    a, b = FIT_GAP
    two = max(w[:a, 2].max(), w[b:, 2].max())
    ray = np.asarray(xyz, np.float64)[a:b] - centre
    ray /= np.linalg.norm(ray, axis=1, keepdims=True)
    cosine = np.abs(np.einsum("ti,ti->t", v[a:b, :, 2], ray))
    return np.degrees(np.arccos(np.minimum(cosine, 1.0))), w[a:b, 2] / two
