"""GPU: tracking people through time (mvp_track_people) against the numpy restatement
tests/track_ref.py on the inputs of tests/track_cases.py, and the path from a process_people
result to per-person trajectories.

track, n_tracks and link_lag must be equal exactly, in every frame: tests/test_people_track.py
asserts that no comparison of these inputs is closer than 1e-7, four orders above the kernel's
contract of 1e-9.  link_cost: the NaN pattern must be equal; a value is a mean of at most 255
distances, each sqrt(dx² + dy² + dz²) in fp64 from exactly representable differences of f32
inputs, so the two sides differ by the FMA contraction of the sum of squares (under 1 ulp of it,
half that after the square root) and by the rounding of the running sum, a few ulp of 2.2e-16 in
all: the bound is rtol 1e-12."""
import numpy as np
import pytest
import torch

import track_cases as cases

pytestmark = pytest.mark.gpu
RTOL = 1e-12


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mvpose import ops as _ops
    return _ops


def _device(ops, xyz, kw, return_links=True):
    track, n, cost, lag = ops.track_people(torch.tensor(xyz, device="cuda"), return_links=return_links, **kw)
    assert track.dtype == torch.int32 and n.dtype == torch.int32
    assert tuple(track.shape) == xyz.shape[:-2] and tuple(n.shape) == xyz.shape[:-4]
    if not return_links:
        assert cost is None and lag is None
        return track.cpu().numpy(), n.cpu().numpy(), None, None
    assert cost.dtype == torch.float64 and lag.dtype == torch.uint8 and cost.shape == track.shape == lag.shape
    return track.cpu().numpy(), n.cpu().numpy(), cost.cpu().numpy(), lag.cpu().numpy()


def _compare(name, got, r):
    track, n, cost, lag = got
    linked = r["link_lag"] > 0
    if linked.any():
        rel = np.abs(cost[linked] - r["link_cost"][linked]) / r["link_cost"][linked]
        print(f"{name}: {r['n_tracks']} tracks, {int(linked.sum())} links, largest lag {r['link_lag'].max()}, "
              f"max rel |cost - ref| = {np.nanmax(rel):.3g}, smallest margin {r['margins'].min():.3g}")
    assert np.array_equal(track, r["track"])
    assert int(n) == r["n_tracks"]
    assert np.array_equal(lag, r["link_lag"])
    assert np.array_equal(np.isnan(cost), np.isnan(r["link_cost"]))
    np.testing.assert_allclose(cost, r["link_cost"], rtol=RTOL, atol=0, equal_nan=True)


@pytest.mark.parametrize("name", sorted(cases.gpu_cases()))
def test_kernel_matches_restatement(ops, name):
    """T = 1; T = 2 with G = J = 1; the designed scene at max_gap 0, 1, 3, 5; G = 8 at max_gap = 15
    (1 024 combinations, 16 per lane); J = 255 at the LDS limit; min_joints = 5 with 3-joint groups;
    T = 130; no present group anywhere; M = 3 sequences in one call, each also against its own call."""
    xyz, kw = cases.gpu_cases()[name]
    r = cases.reference(name)
    got = _device(ops, xyz, kw)
    if xyz.ndim == 4:
        _compare(name, got, r)
        return
    for m in range(xyz.shape[0]):
        _compare(f"{name}[{m}]", tuple(a[m] for a in got), r[m])
        alone = _device(ops, xyz[m], kw)
        for a, b in zip(got, alone):
            assert np.array_equal(a[m].view(np.int64) if a.dtype == np.float64 else a[m],
                                  b.view(np.int64) if b.dtype == np.float64 else b)


def test_same_bits_on_every_call_and_null_links(ops):
    for name in ("scene_gap3", "G8_gap15_T40", "M3_G5_gap7"):
        xyz, kw = cases.gpu_cases()[name]
        a, b = _device(ops, xyz, kw), _device(ops, xyz, kw)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])
        assert np.array_equal(a[2].view(np.int64), b[2].view(np.int64))
        n = _device(ops, xyz, kw, return_links=False)
        assert np.array_equal(n[0], a[0]) and np.array_equal(n[1], a[1])


def test_max_gap_0_is_link_tracks(ops):
    from mvpose import people
    xyz = cases.designed_scene()[0]
    xd = torch.tensor(xyz, device="cuda")
    track, n = people.track_people(xd, max_gap=0)
    assert track.is_cuda and n.is_cuda and n.dim() == 0
    want = people.link_tracks(xd)
    assert np.array_equal(track.cpu().numpy(), want) and int(n) == want.max() + 1 == 5
    assert int(people.track_people(xd, max_gap=3)[1]) == 3


def test_argument_errors(ops):
    from mvpose import _lib
    xd = torch.tensor(cases.designed_scene()[0][:4], device="cuda")
    for kw, what in ((dict(max_gap=-1), "max_gap"), (dict(max_gap=16), "max_gap"), (dict(max_jump=0.0), "max_jump"),
                     (dict(max_jump=float("nan")), "max_jump"), (dict(gap_growth=-1.0), "gap_growth"),
                     (dict(gap_growth=float("inf")), "gap_growth"), (dict(min_joints=0), "min_joints"),
                     (dict(min_joints=18), "min_joints")):
        with pytest.raises(_lib.MvposeError, match=what):
            ops.track_people(xd, **kw)
    with pytest.raises(_lib.MvposeError, match="G="):
        ops.track_people(torch.zeros((2, 9, 17, 3), device="cuda"))
    with pytest.raises(_lib.MvposeError, match="LDS"):
        ops.track_people(torch.zeros((2, 8, 255, 3), device="cuda"), max_gap=1)
    with pytest.raises(ValueError):
        ops.track_people(xd[0])
    with pytest.raises(ValueError):
        ops.track_people(xd[..., :2].contiguous())
    with pytest.raises(TypeError):
        ops.track_people(xd.double())
    # a refused call writes nothing
    track = torch.full((4, 4), 7, dtype=torch.int32, device="cuda")
    n = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    rc = _lib.lib.mvp_track_people(xd.data_ptr(), 1, 4, 4, 17, 5, 50.0, 0.5, 18, track.data_ptr(), n.data_ptr(), None,
                                   None, None)
    torch.cuda.synchronize()
    assert rc == -1 and "min_joints" in _lib.last_error() and (track == 7).all() and (n == 7).all()


def test_process_people_result_to_smoothed_person(ops):
    """A process_people-shaped result on synthetic kpts_3d, no backbone: two people in shuffled
    groups, one of them missing for 3 frames.  people_trajectories gives that person one row whose
    `present` is False exactly on the gap, and refine.smooth_trajectory fills the gap."""
    from mvpose import refine
    from mvpose.pipeline import MultiViewPipeline
    T, G = 30, 3
    tracks = [cases.walk(T, 17, 21, (-100.0, 0.0, 0.0), (2.0, 0.0, 0.0)),
              cases.walk(T, 17, 22, (100.0, 0.0, 50.0), (0.0, 0.0, 1.0))]
    xyz, truth = cases.groups(tracks, [[(0, 12), (15, T)], [(0, T)]], G, seed=23)
    cov = np.where(np.isfinite(xyz).all(-1)[..., None, None], 4.0 * np.eye(3, dtype=np.float32), np.float32("nan"))
    status = np.where(np.isfinite(xyz).all(-1), 0, 0x80).astype(np.uint8)
    out = {"kpts_3d": torch.tensor(xyz, device="cuda"), "kpts_3d_cov": torch.tensor(cov.astype(np.float32), device="cuda"),
           "tri_refine_status": torch.tensor(status, device="cuda")}
    # as the concatenation of two chunks' results
    out = {k: torch.cat([v[:13], v[13:]]) for k, v in out.items()}
    res = MultiViewPipeline.people_trajectories(out, max_gap=3)
    assert sorted(res) == ["kpts_3d_cov_person", "kpts_3d_person", "person_present", "person_track",
                           "tri_refine_status_person"]
    pts, present = res["kpts_3d_person"], res["person_present"]
    assert pts.is_cuda and tuple(pts.shape) == (T, 2, 17, 3) and tuple(present.shape) == (T, 2)
    assert tuple(res["kpts_3d_cov_person"].shape) == (T, 2, 17, 3, 3) and res["tri_refine_status_person"].dtype == torch.uint8
    assert res["person_track"].tolist() == [1, 0] or res["person_track"].tolist() == [0, 1]
    present = present.cpu().numpy()
    assert present[:, 0].all()                                     # the person seen in every frame ranks first
    gap = np.zeros(T, bool)
    gap[12:15] = True
    assert np.array_equal(~present[:, 1], gap)
    # row p is the person: its observed frames are that person's groups
    for p, person in ((0, 1), (1, 0)):
        for t in np.flatnonzero(present[:, p]):
            g = int(np.flatnonzero(truth[t] == person)[0])
            assert np.array_equal(pts[t, p].cpu().numpy(), xyz[t, g], equal_nan=True)
    assert torch.isnan(pts[12:15, 1]).all() and (res["tri_refine_status_person"][12:15, 1] == 0).all()
    sm = refine.smooth_trajectory(pts[:, 1], cov=res["kpts_3d_cov_person"][:, 1],
                                  status=res["tri_refine_status_person"][:, 1])
    assert tuple(sm.shape) == (T, 17, 3) and torch.isfinite(sm).all()
    # without gap tolerance the same person is two rows
    split = MultiViewPipeline.people_trajectories(out, max_gap=0)
    assert split["kpts_3d_person"].shape[1] == 3
