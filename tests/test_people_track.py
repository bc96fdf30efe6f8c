"""CPU: tracking people through time (mvp_track_people) — the restatement tests/track_ref.py
against people.link_tracks and against ground truth, the comparison margins of the inputs the GPU
test uses, the plan call's figure and refusals, the ops front's checks, and
people.person_trajectories."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import track_cases as cases
import track_ref as ref

MIN_MARGIN = 1e-7      # the kernel's track numbers are bound to the restatement's above 1e-9 (mvpose.h)


def test_entry_points_declared():
    from mvpose import _lib
    header = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "mvpose.h")
    src = open(header).read()
    for name in ("mvp_track_people_plan", "mvp_track_people"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src)
        assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES


# ------------------------------------------------------------------ the restatement
def _walk(T, start, step):
    body = np.random.default_rng(1).normal(0.0, 20.0, (17, 3))
    return start + np.arange(T)[:, None, None] * np.asarray(step, float) + body


def _crossing():
    """test_people_assoc.py::test_link_tracks_crossing's input."""
    T = 40
    a, b = _walk(T, np.array([-150.0, 0, 0]), (8.0, 0, 0)), _walk(T, np.array([150.0, 0, 60.0]), (-8.0, 0, 0))
    flip = np.random.default_rng(2).uniform(size=T) < 0.5
    xyz = np.full((T, 3, 17, 3), np.nan)
    xyz[~flip, 0], xyz[~flip, 2] = a[~flip], b[~flip]
    xyz[flip, 0], xyz[flip, 2] = b[flip], a[flip]
    xyz[5, :, 3] = np.nan
    return xyz


def _vanishing():
    """test_people_assoc.py::test_link_tracks_vanishing's input."""
    T = 30
    a, b = _walk(T, np.array([-100.0, 0, 0]), (1.0, 0, 0)), _walk(T, np.array([100.0, 0, 0]), (0, 1.0, 0))
    xyz = np.stack([a, b], 1)
    xyz[10:15, 1] = np.nan
    xyz[20:, 0] += np.array([0.0, 0.0, 70.0])
    return xyz


@pytest.mark.parametrize("make,max_jump", [(_crossing, 50.0), (_vanishing, 50.0), (_vanishing, 80.0)])
def test_restatement_equals_link_tracks(make, max_jump):
    """max_gap = 0, min_joints = 1: frame-to-frame greedy linking, people.link_tracks' numbers."""
    from mvpose import people
    xyz = make()
    r = ref.track(xyz, max_gap=0, max_jump=max_jump)
    want = people.link_tracks(xyz, max_jump=max_jump)
    assert np.array_equal(r["track"], want) and r["n_tracks"] == want.max() + 1
    linked = r["link_lag"] > 0
    assert (r["link_lag"][linked] == 1).all() and np.isfinite(r["link_cost"][linked]).all()
    assert np.isnan(r["link_cost"][~linked]).all()


def test_restatement_bridges_what_link_tracks_splits():
    """The person of test_link_tracks_vanishing, absent for frames 10-14, keeps one number once
    max_gap covers the 5 missing frames; the 70 cm jump still starts a new track."""
    xyz = _vanishing()
    r = ref.track(xyz, max_gap=5)
    assert (r["track"][:10, 1] == 1).all() and (r["track"][15:, 1] == 1).all() and r["link_lag"][15, 1] == 6
    assert (r["track"][:20, 0] == 0).all() and (r["track"][20:, 0] == 2).all() and r["n_tracks"] == 3
    assert ref.track(xyz, max_gap=4)["n_tracks"] == 4


def _tracks_of(track, truth, person):
    return sorted(set(track[truth == person].tolist()))


def test_designed_scene_recovers_ground_truth():
    """Two people crossing, a 3-frame and a 2-frame dropout, one person entering and leaving, slots
    permuted per frame, lost joints, noise: max_gap = 3 gives one track per person, max_gap = 1
    splits each of the two dropouts."""
    xyz, truth = cases.designed_scene()
    assert xyz.shape == (60, 4, 17, 3) and (truth >= 0).sum() == 60 - 3 + 60 - 2 + 40
    r = ref.track(xyz, max_gap=3)
    print(f"max_gap=3: {r['n_tracks']} tracks, smallest margin {r['margins'].min():.3g}")
    assert r["n_tracks"] == 3 and np.array_equal(r["track"] >= 0, truth >= 0)
    ids = [_tracks_of(r["track"], truth, p) for p in range(3)]
    assert all(len(i) == 1 for i in ids) and len({i[0] for i in ids}) == 3
    assert r["link_lag"].max() == 4 and (r["link_lag"] == 4).sum() == 1 and (r["link_lag"] == 3).sum() == 1
    r1 = ref.track(xyz, max_gap=1)
    print(f"max_gap=1: {r1['n_tracks']} tracks, smallest margin {r1['margins'].min():.3g}")
    assert r1["n_tracks"] == 5
    assert [len(_tracks_of(r1["track"], truth, p)) for p in range(3)] == [2, 2, 1]


@pytest.mark.parametrize("name", sorted(cases.gpu_cases()))
def test_gpu_case_margins(name):
    """A condition on the inputs: no frame of a GPU case has a comparison closer than 1e-7, so the
    GPU test compares every frame."""
    r = cases.reference(name)
    m = np.concatenate([q["margins"] for q in (r if isinstance(r, list) else [r])])
    print(f"{name}: smallest margin {m.min():.3g}")
    assert m.min() >= MIN_MARGIN


def test_gpu_cases_hold_what_they_name():
    c = cases.gpu_cases()
    r = cases.reference("T2_G1_J1")
    assert r["track"].tolist() == [[0], [0]] and r["link_lag"].tolist() == [[0], [1]]
    assert [cases.reference(f"scene_gap{g}")["n_tracks"] for g in (0, 1, 3, 5)] == [5, 5, 3, 3]
    x, kw = c["G8_gap15_T40"]
    r = cases.reference("G8_gap15_T40")
    assert x.shape[1] == 8 and kw["max_gap"] == 15 and (kw["max_gap"] + 1) * 64 == 1024
    assert r["link_lag"].max() >= 10 and (r["track"] >= 0).sum(1).max() == 7
    x, kw = c["J255_G7_gap1"]
    assert x.shape[1:3] == (7, 255) and _lds(7, 255, kw["max_gap"]) == 64736 <= 65536
    assert _plan(G=7, J=255, max_gap=1)[0] == 0 and _plan(G=7, J=255, max_gap=2)[0] == _plan(G=8, J=255, max_gap=1)[0] == -1
    x, kw = c["min_joints5_G6_gap9"]
    r = cases.reference("min_joints5_G6_gap9")
    seen = np.isfinite(x).all(-1).sum(-1)
    short = np.argwhere(seen == 3)
    assert len(short) == 3 and kw["min_joints"] == 5
    for t, g in short:                                        # a new track, and its successor another
        assert r["link_lag"][t, g] == 0 and r["track"][t, g] >= 0
        assert r["track"][t, g] not in r["track"][t + 1:]
    r = cases.reference("all_nan")
    assert (r["track"] == -1).all() and r["n_tracks"] == 0 and np.isinf(r["margins"]).all()
    rs = cases.reference("M3_G5_gap7")
    assert len(rs) == 3 and len({q["n_tracks"] for q in rs}) > 1
    # every number of combinations per lane the kernel is compiled for: K·G² in (0, 64], (64, 128], ... (512, 1024]
    combos = sorted((kw.get("max_gap", 5) + 1) * x.shape[-3] ** 2 for x, kw in c.values())
    for lo, hi in ((0, 64), (64, 128), (128, 256), (256, 512), (512, 1024)):
        assert any(lo < e <= hi for e in combos), (lo, hi, combos)


# ------------------------------------------------------------------ the plan call and the ops front
def _plan(M=1, T=10, G=4, J=17, max_gap=5):
    from mvpose import _lib
    lds = ctypes.c_int(0)
    rc = _lib.lib.mvp_track_people_plan(M, T, G, J, max_gap, ctypes.byref(lds))
    return rc, lds.value, _lib.last_error()


def _lds(G, J, max_gap):
    return (max_gap + 2) * G * (12 * J + 4) + (max_gap + 1) * G * G * 4

def test_plan_reports_and_refuses():
    rc, lds, _ = _plan()
    # the ring of max_gap + 2 frames, the track table over it, the list of the (max_gap + 1)·G² combinations
    assert rc == 0 and lds == 7 * 4 * 17 * 12 + 7 * 4 * 4 + 6 * 16 * 4 == _lds(4, 17, 5)
    assert _plan(G=8, max_gap=15)[:2] == (0, _lds(8, 17, 15))
    assert _plan(T=1, G=1, J=1, max_gap=0)[:2] == (0, 2 * 16 + 4)
    assert _plan(G=7, J=255, max_gap=1)[:2] == (0, 64736) and _plan(G=3, J=255, max_gap=5)[0] == 0
    assert _plan(M=2 ** 20, T=2 ** 10, G=1, J=1)[0] == 0
    from mvpose import _lib
    assert _lib.lib.mvp_track_people_plan(1, 10, 4, 17, 5, None) == 0
    for kw, what in ((dict(M=0), "M="), (dict(T=0), "T="), (dict(G=0), "G="), (dict(G=9), "G="), (dict(J=0), "J="),
                     (dict(J=256), "J="), (dict(max_gap=-1), "max_gap"), (dict(max_gap=16), "max_gap"),
                     (dict(M=2 ** 20, T=2 ** 11, G=1, J=1), "M*T*G*J"), (dict(M=2 ** 16, T=2 ** 16), "M*T*G*J"),
                     (dict(T=2 ** 27, G=4, J=17), "M*T*G*J"),
                     (dict(G=2, J=255, max_gap=9), "LDS"), (dict(G=8, J=255, max_gap=1), "LDS")):
        rc, _, msg = _plan(**kw)
        assert rc == -1 and what in msg and "mvp_track_people_plan" in msg, (kw, rc, msg)


def test_call_refuses_before_any_device_work():
    """Null pointers throughout: every refusal comes before the first use of one."""
    from mvpose import _lib

    def run(M=1, T=10, G=4, J=17, max_gap=5, max_jump=50.0, gap_growth=0.5, min_joints=1):
        rc = _lib.lib.mvp_track_people(None, M, T, G, J, max_gap, max_jump, gap_growth, min_joints, None, None, None,
                                       None, None)
        return rc, _lib.last_error()

    inf, nan = float("inf"), float("nan")
    for kw, what in ((dict(M=0), "M="), (dict(T=0), "T="), (dict(G=9), "G="), (dict(J=256), "J="),
                     (dict(max_gap=16), "max_gap"), (dict(max_jump=0.0), "max_jump"), (dict(max_jump=-1.0), "max_jump"),
                     (dict(max_jump=inf), "max_jump"), (dict(max_jump=nan), "max_jump"),
                     (dict(gap_growth=-0.1), "gap_growth"), (dict(gap_growth=inf), "gap_growth"),
                     (dict(gap_growth=nan), "gap_growth"), (dict(min_joints=0), "min_joints"),
                     (dict(min_joints=18), "min_joints"), (dict(T=2 ** 27), "M*T*G*J"),
                     (dict(G=8, J=255, max_gap=1, min_joints=1), "LDS"), (dict(), "null device pointer")):
        rc, msg = run(**kw)
        assert rc == -1 and what in msg and "mvp_track_people:" in msg, (kw, rc, msg)


def test_ops_front_checks_before_any_launch():
    from mvpose import ops, people
    with pytest.raises(ValueError, match="GPU"):
        ops.track_people(torch.zeros((4, 2, 17, 3)))
    with pytest.raises(ValueError, match="GPU"):
        ops.track_people(torch.zeros((2, 4, 2, 17, 3)), max_gap=2)
    with pytest.raises(TypeError):
        ops.track_people(torch.zeros((4, 2, 17, 3), dtype=torch.float64))
    with pytest.raises(TypeError):
        ops.track_people(np.zeros((4, 2, 17, 3), np.float32))
    with pytest.raises(ValueError):
        people.track_people(np.zeros((4, 2, 17, 3), np.float32))
    with pytest.raises(ValueError):
        people.track_people(torch.zeros((2, 4, 2, 17, 3)))
    assert ops.track_people_plan(1, 10, 4, 17) == _lds(4, 17, 5)
    assert ops.track_people_plan(3, 10, 4, 17, max_gap=0) == _lds(4, 17, 0)


# ------------------------------------------------------------------ people.person_trajectories
def test_person_trajectories():
    from mvpose import people
    #            t: 0   1   2   3   4   5
    track = torch.tensor([[0, 0, 1, 1, 1, 1],        # slot 0
                          [1, -1, 0, 2, 3, -1],      # slot 1
                          [-1, 1, -1, -1, 2, 2]], dtype=torch.int32).T.contiguous()
    T, G = track.shape
    # frames present: track 0: 3, track 1: 6, track 2: 3, track 3: 1
    rng = np.random.default_rng(0)
    xyz = torch.tensor(rng.normal(size=(T, G, 5, 3)).astype(np.float32))
    status = torch.tensor(rng.integers(1, 200, (T, G, 5)).astype(np.uint8))
    flag = torch.ones((T, G), dtype=torch.bool)
    got, present, chosen = people.person_trajectories(track, {"xyz": xyz, "status": status, "flag": flag})
    assert chosen.tolist() == [1, 0, 2, 3] and chosen.dtype == torch.int64          # (-frames, number)
    assert present.dtype == torch.bool and present.sum(0).tolist() == [6, 3, 3, 1]
    assert got["xyz"].shape == (T, 4, 5, 3) and got["status"].shape == (T, 4, 5) and got["flag"].shape == (T, 4)
    assert got["xyz"].dtype == torch.float32 and got["status"].dtype == torch.uint8 and got["flag"].dtype == torch.bool
    for p, tr in enumerate(chosen.tolist()):
        for t in range(T):
            g = np.flatnonzero(track[t].numpy() == tr)
            assert bool(present[t, p]) == (len(g) == 1)
            if len(g):
                assert torch.equal(got["xyz"][t, p], xyz[t, g[0]]) and torch.equal(got["status"][t, p], status[t, g[0]])
                assert bool(got["flag"][t, p])
            else:
                assert torch.isnan(got["xyz"][t, p]).all() and (got["status"][t, p] == 0).all()
                assert not bool(got["flag"][t, p])
    _, _, ch = people.person_trajectories(track, {}, min_len=3)
    assert ch.tolist() == [1, 0, 2]
    _, _, ch = people.person_trajectories(track, {}, min_len=2, max_people=2)
    assert ch.tolist() == [1, 0]
    got, present, ch = people.person_trajectories(track, {"xyz": xyz}, min_len=7)
    assert ch.tolist() == [] and present.shape == (T, 0) and got["xyz"].shape == (T, 0, 5, 3)
    got, present, ch = people.person_trajectories(torch.full((4, 2), -1, dtype=torch.int32), {"xyz": xyz[:4, :2]})
    assert ch.tolist() == [] and got["xyz"].shape == (4, 0, 5, 3)
    with pytest.raises(ValueError):
        people.person_trajectories(track, {"xyz": xyz[:, :2]})
    with pytest.raises(ValueError):
        people.person_trajectories(track.float(), {})
    with pytest.raises(ValueError):
        people.person_trajectories(track, {}, min_len=0)
