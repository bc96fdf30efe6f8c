"""The kernel each launch of the person detector runs is pinned: for every case of
det_launch_kernel_cases.py (the default switches, each non-default value of each switch and
MVPOSE_DET_DWPW=0, at size 128 with 3 frames and at 640 with 2) RTMDetector.launch_kernels must
match tests/golden/det_launch_kernels.json.  The fixture does not come from launch_kernels:
tools/record_launch_kernels.py --det read it off kernel traces of one forward per case, template
arguments included, so it says what ran, and this test checks that the detector reports that:
each reported variant names the traced kernel function and the template arguments the variant fixes
(det_launch_kernel_cases.VARIANTS).  Detector construction only: no forward runs, except in the
last test, which checks that the choice is made at construction and stays."""
import json

import numpy as np
import pytest
import torch

import det_launch_kernel_cases as dlc
from mvpose import _lib, rtmdet as D

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pinned():
    with open(dlc.FIXTURE) as f:
        return json.load(f)["cases"]


def test_fixture_has_every_case(pinned):
    assert sorted(pinned) == sorted(c.name for c in dlc.cases())


def test_table_has_every_variant():
    names, k = [], 1
    while _lib.lib.mvp_det_kernel_name(k):
        names.append(_lib.lib.mvp_det_kernel_name(k).decode())
        k += 1
    assert sorted(names) == sorted(dlc.VARIANTS)


def test_traced_names_keep_their_template_arguments(pinned):
    for name, launches in pinned.items():
        for traced in launches:
            base, args = dlc.parse(traced)  # asserts the form: nothing cut off
            assert any(base == b for b, _ in dlc.VARIANTS.values()), (name, traced)


@pytest.mark.parametrize("case", dlc.cases(), ids=[c.name for c in dlc.cases()])
def test_launch_kernels_are_pinned(pinned, case):
    with dlc.built(case) as det:
        got = det.launch_kernels()
    want = pinned[case.name]
    assert len(got) == len(want)
    for i, (k, w) in enumerate(zip(got, want)):
        assert dlc.matches(k, w), f"launch {i}: the detector reports {k} {dlc.VARIANTS[k]}, the trace has {w}"


def test_switches_are_read_at_create_only(monkeypatch):
    """A switch changed under a live detector changes nothing: same kernels, bit-identical
    candidates; a detector created afterwards runs what the switches then say."""
    for k in dlc.CLEARED:
        monkeypatch.delenv(k, raising=False)
    n, size = 2, 128
    frames = torch.from_numpy(np.random.default_rng(41).integers(0, 256, (n, size * 9 // 8, 2 * size, 3),
                                                                 dtype=np.uint8)).cuda()
    det = D.RTMDetector(dlc.state_dict(), max_batch=n, size=size)
    kernels = det.launch_kernels()
    assert "pers_gemm" in kernels and "halo_pers_lt3" in kernels
    cand = det.detect(frames)["cand"].clone()
    torch.cuda.synchronize()
    monkeypatch.setenv("MVPOSE_DET_PERS", "0")
    monkeypatch.setenv("MVPOSE_DET_HALO_PERS", "0")
    again = det.detect(frames)["cand"]
    torch.cuda.synchronize()
    assert det.launch_kernels() == kernels
    assert torch.equal(again.view(torch.int32), cand.view(torch.int32))
    det.close()
    late = D.RTMDetector(dlc.state_dict(), max_batch=n, size=size)
    now = late.launch_kernels()
    late.close()
    assert "gemm" in now and "halo_live3" in now and "halo" in now
    assert not {"pers_gemm", "fold_up", "fold_ca", "halo_pers_lt2", "halo_pers_lt3", "halo_pers_lt4"} & set(now)
