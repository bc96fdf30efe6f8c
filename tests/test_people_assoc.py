"""CPU: cross-view association (mvp_associate_views) — the restatement tests/people_ref.py against
ground truth, the comparison margins of the inputs the GPU test uses, the plan call's argument
refusals, and mvpose.people's gather_groups and link_tracks."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import people_cases as cases
import people_ref as ref

MIN_MARGIN = 1e-7      # the kernel's group numbers are bound to the restatement's above 1e-9 (mvpose.h)


def test_entry_points_declared():
    from mvpose import _lib
    header = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "mvpose.h")
    src = open(header).read()
    for name in ("mvp_associate_views_plan", "mvp_associate_views"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src)
        assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES


@pytest.mark.parametrize("n_people,n_cams,P,noise", [(3, 4, 4, 1.0), (4, 4, 4, 2.0), (2, 2, 3, 1.0)])
def test_restatement_recovers_ground_truth(n_people, n_cams, P, noise):
    """Default thresholds; every frame's groups are the people."""
    T = 100
    cams, k, truth = cases.scene(n_people, n_cams, P, T, seed=20 + n_people + n_cams, noise_px=noise)
    r = ref.associate(k, cams, list(range(n_cams)))
    wrong = [t for t in range(T) if not cases.same_partition(r["group"][t], truth[t])]
    print(f"{n_people} people, {n_cams} cameras: {len(wrong)} wrong frames of {T}, "
          f"smallest margin {r['margins'].min():.3g}")
    assert wrong == []
    # the numbering: groups seen by more views first, then by smallest node
    for t in range(T):
        g = r["group"][t]
        n_groups = int(r["count"][t, 0])
        assert sorted(set(g[g >= 0].tolist())) == list(range(n_groups))
        views = [int((g == q).any(1).sum()) for q in range(n_groups)]
        first = [int(np.flatnonzero(g.ravel() == q)[0]) for q in range(n_groups)]
        assert [(-v, f) for v, f in zip(views, first)] == sorted((-v, f) for v, f in zip(views, first))
        assert int(r["count"][t, 1]) == sum(v >= 2 for v in views)
        assert all(((g == q).sum(1) <= 1).all() for q in range(n_groups))


@pytest.mark.parametrize("name", sorted(cases.gpu_cases()))
def test_gpu_case_margins(name):
    """A condition on the inputs: no frame of a GPU case has a comparison closer than 1e-7, so the
    GPU test compares every frame."""
    m = cases.reference(name)["margins"]
    print(f"{name}: smallest margin {m.min():.3g}")
    assert m.min() >= MIN_MARGIN


def test_data_case_holds_what_it_names():
    r = cases.reference("data")
    cams, k, ci, kw = cases.gpu_cases()["data"]
    assert (r["group"][0] == -1).all() and r["count"][0].tolist() == [0, 0]
    aff, usable, pairs = ref.affinity(k, cams, list(ci), **kw)
    assert (~usable[1, 0]).sum() == 2                       # the empty slot and the 3-joint node
    assert (usable[2].sum(1) == 3).all()                    # 3 people in 4 slots, all usable
    # frame 2: the two 10-joint nodes of person 1 in views 0 and 1 have 3 joints in common
    x = np.isfinite(k[2, :, :, 0, :2])                      # (P, J, 2 views)
    a = int(np.flatnonzero(x[:, :, 0].sum(1) <= 10)[0])
    b = int(np.flatnonzero(x[:, :, 1].sum(1) <= 10)[0])
    assert aff[2, pairs.index((0, 1)), a, b] == -1.0 and (x[a, :, 0] & x[b, :, 1]).sum() < 5
    assert (~usable[3, 2]).sum() == 2                       # the empty slot and the one below min_conf
    assert (r["count"][1:, 0] >= 3).all()


def test_thresholds_cases_do_what_they_name():
    r = cases.reference("singletons_nv4_P4")
    assert (r["count"][:, 1] == 0).all() and (r["count"][:, 0] == (r["group"] >= 0).sum((1, 2))).all()
    for name in ("views_only_nv4_P4", "views_only_nv8_P8"):
        r = cases.reference(name)
        g = r["group"]
        # nothing but the one-node-per-view rule stops the merging: as many groups as the fullest view
        assert (r["count"][:, 0] == (g >= 0).sum(2).max(1)).all()


# ------------------------------------------------------------------ the plan call's refusals
def _plan(T=10, P=4, J=17, nv=4, min_conf=0.0, trunc_px=20.0, max_cost_px=8.0, min_joints=5):
    from mvpose import _lib
    lds, nbytes = ctypes.c_int(0), ctypes.c_int64(0)
    rc = _lib.lib.mvp_associate_views_plan(T, P, J, nv, min_conf, trunc_px, max_cost_px, min_joints,
                                           ctypes.byref(lds), ctypes.byref(nbytes))
    return rc, lds.value, nbytes.value, _lib.last_error()


def test_plan_reports_and_refuses():
    rc, lds, nbytes, _ = _plan()
    assert rc == 0
    assert lds == 16 * 17 * 8 + 6 * 72 + 16 * 17 * 8        # link (row stride N | 1), F, pixels
    assert nbytes >= 4 * 10 * 4 * 17 * 8 + 6 * 72
    rc, lds, _, _ = _plan(P=8, nv=8, J=255)                  # N = 64: the pixels stay in the workspace
    assert rc == 0 and lds == 64 * 65 * 8 + 28 * 72
    assert _plan(P=32, nv=2)[0] == 0 and _plan(P=1, nv=2, J=1, min_joints=1)[0] == 0
    inf, nan = float("inf"), float("nan")
    for kw, what in ((dict(T=0), "T="), (dict(nv=1), "n_cam_idx"), (dict(nv=9, P=1), "n_cam_idx"),
                     (dict(P=0), "P="), (dict(P=17), "P="), (dict(P=33, nv=2), "P="), (dict(J=0), "J="),
                     (dict(J=256), "J="), (dict(min_joints=0), "min_joints"), (dict(min_joints=18), "min_joints"),
                     (dict(max_cost_px=0.0), "max_cost_px"), (dict(max_cost_px=-1.0), "max_cost_px"),
                     (dict(max_cost_px=20.0), "max_cost_px"), (dict(max_cost_px=25.0), "max_cost_px"),
                     (dict(trunc_px=inf), "trunc_px"), (dict(max_cost_px=nan), "max_cost_px"),
                     (dict(trunc_px=nan), "trunc_px"), (dict(min_conf=nan), "min_conf"),
                     (dict(T=2 ** 30, P=16), "T*P*J")):
        rc, _, _, msg = _plan(**kw)
        assert rc == -1 and what in msg and "mvp_associate_views_plan" in msg, (kw, rc, msg)


def test_ops_front_checks_before_any_launch():
    from mvpose import ops
    with pytest.raises(ValueError, match="GPU"):
        ops.associate_views(torch.zeros((2, 2, 17, 3, 2)), torch.zeros((2, 40), dtype=torch.float64), (0, 1))
    with pytest.raises(TypeError):
        ops.associate_views(np.zeros((2, 2, 17, 3, 2), np.float32), None, (0, 1))
    assert ops.associate_views_plan(10, 4, 17, 4)[0] == 16 * 17 * 8 + 6 * 72 + 16 * 17 * 8


# ------------------------------------------------------------------ mvpose.people
def test_gather_groups():
    from mvpose import people
    rng = np.random.default_rng(0)
    T, P, J, V = 3, 3, 4, 4
    ci = (2, 0, 3)
    k = torch.tensor(rng.normal(size=(T, P, J, 3, V)).astype(np.float32))
    gauss = torch.tensor(rng.normal(size=(T, V, P, J, 6)))
    group = torch.full((T, 3, P), -1, dtype=torch.int8)
    group[0, 0] = torch.tensor([1, 0, -1])        # view position 0 = column 2
    group[0, 1] = torch.tensor([0, 2, 1])
    group[0, 2] = torch.tensor([-1, -1, 0])
    group[2, 1] = torch.tensor([3, 0, 1])         # groups 0, 1 and 3: 3 is beyond max_groups = 3
    kg, gg, dropped = people.gather_groups(k, group, ci, 3, gauss=gauss)
    assert kg.shape == (T, 3, J, 3, V) and gg.shape == (T, 3, V, J, 6) and dropped.tolist() == [0, 0, 1]
    want = np.full((T, 3, J, 3, V), np.nan, np.float32)
    want_g = np.full((T, 3, V, J, 6), np.nan)
    for t in range(T):
        for i, c in enumerate(ci):
            for p in range(P):
                g = int(group[t, i, p])
                if 0 <= g < 3:
                    want[t, g, :, :, c] = k[t, p, :, :, c].numpy()
                    want_g[t, g, c] = gauss[t, c, p].numpy()
    np.testing.assert_array_equal(kg.numpy(), want)
    np.testing.assert_array_equal(gg.numpy(), want_g)
    assert np.isnan(kg[..., 1].numpy()).all()      # a column that cam_idx does not list
    kg2, none, _ = people.gather_groups(k, group, ci, 5)
    assert none is None and kg2.shape[1] == 5 and torch.equal(kg2[:, :3].nan_to_num(7.0), kg.nan_to_num(7.0))
    assert torch.isfinite(kg2[2, 3, :, :, 0]).all() and torch.isnan(kg2[:, 4]).all()
    with pytest.raises(ValueError):
        people.gather_groups(k, group[:, :2], ci, 3)
    with pytest.raises(ValueError):
        people.gather_groups(k, group, ci, 0)


def _walk(T, start, step):
    body = np.random.default_rng(1).normal(0.0, 20.0, (17, 3))
    return start + np.arange(T)[:, None, None] * np.asarray(step, float) + body


def test_link_tracks_crossing():
    """Two people walk through each other's x position, 60 cm apart in z, 8 cm per frame; the
    group order flips at random.  Each keeps its track."""
    from mvpose import people
    T = 40
    a, b = _walk(T, np.array([-150.0, 0, 0]), (8.0, 0, 0)), _walk(T, np.array([150.0, 0, 60.0]), (-8.0, 0, 0))
    rng = np.random.default_rng(2)
    flip = rng.uniform(size=T) < 0.5
    xyz = np.full((T, 3, 17, 3), np.nan)
    xyz[~flip, 0], xyz[~flip, 2] = a[~flip], b[~flip]
    xyz[flip, 0], xyz[flip, 2] = b[flip], a[flip]
    xyz[5, :, 3] = np.nan                                     # a joint lost in one frame
    tr = people.link_tracks(xyz)
    assert tr.dtype == np.int32 and tr.shape == (T, 3) and (tr[:, 1] == -1).all()
    is_a = np.where(flip, tr[:, 2], tr[:, 0])
    is_b = np.where(flip, tr[:, 0], tr[:, 2])
    assert (is_a == is_a[0]).all() and (is_b == is_b[0]).all() and {int(is_a[0]), int(is_b[0])} == {0, 1}
    assert np.array_equal(people.link_tracks(torch.tensor(xyz)), tr)


def test_link_tracks_vanishing():
    """A person absent for frames 10-14 comes back as a new track; a jump of more than max_jump
    starts a new track; the other person's track is untouched."""
    from mvpose import people
    T = 30
    a, b = _walk(T, np.array([-100.0, 0, 0]), (1.0, 0, 0)), _walk(T, np.array([100.0, 0, 0]), (0, 1.0, 0))
    xyz = np.stack([a, b], 1)
    xyz[10:15, 1] = np.nan
    xyz[20:, 0] += np.array([0.0, 0.0, 70.0])
    tr = people.link_tracks(xyz, max_jump=50.0)
    assert (tr[:20, 0] == 0).all() and (tr[:10, 1] == 1).all() and (tr[10:15, 1] == -1).all()
    assert (tr[15:, 1] == 2).all() and (tr[20:, 0] == 3).all()
    assert (people.link_tracks(xyz, max_jump=80.0)[:, 0] == 0).all()
    assert people.link_tracks(np.full((2, 2, 17, 3), np.nan)).tolist() == [[-1, -1], [-1, -1]]
    with pytest.raises(ValueError):
        people.link_tracks(np.zeros((3, 17, 3)))
