"""The kernel each launch of the HRNet graph runs is pinned: for every case of
launch_kernel_cases.py (launch_plan_cases.py's graphs under each fusion switch, and the BasicBlock
planes of test_conv_planes_gpu.py under its three kernel modes at batch 7, with and without
MVPOSE_CROP_STREAM=1) ConvGraph.launch_kernels must equal tests/golden/launch_kernels.json.  The
fixture does not come from launch_kernels: tools/record_launch_kernels.py read it off kernel traces
of one forward per case, so it says what ran, and this test checks that the graph reports that.
Graph construction only: no forward runs."""
import json

import pytest
import torch

import launch_kernel_cases as lkc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pinned():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    with open(lkc.FIXTURE) as f:
        return json.load(f)["cases"]


def test_fixture_has_every_case(pinned):
    assert sorted(pinned) == sorted(c.name for c in lkc.cases())


@pytest.mark.parametrize("case", lkc.cases(), ids=[c.name for c in lkc.cases()])
def test_launch_kernels_are_pinned(pinned, case):
    with lkc.built(case) as g:
        got = g.launch_kernels(case.batch)
        assert len(got) == len(g.launch_plan(case.batch))
    want = pinned[case.name]
    assert len(got) == len(want)
    for i, (k, w) in enumerate(zip(got, want)):
        assert k == w, f"launch {i}: the graph reports {k}, the trace has {w}"


def test_last_micro_batch_chooses_for_its_own_size(monkeypatch):
    """A segment's smaller last micro-batch falls below one crop per CU while the full ones do
    not: its records show the tile kernels, the full ones the crop-streaming kernels."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mvpose import hrnet
    for k in lkc.CLEARED:
        monkeypatch.delenv(k, raising=False)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    spec = hrnet.GraphSpec()
    spec.segment(cus)
    sd = hrnet.basic_block_spec(32, 64, 48, seed=3)[3]
    x = spec.tensor(64, 48, 32)
    h = spec.conv(sd, "b0.conv1", "b0.bn1", x, 1, True)
    y = spec.conv(sd, "b0.conv2", "b0.bn2", h, 1, True, res=x)
    g = hrnet.ConvGraph(spec, x, y, max_batch=cus + 3)
    try:
        assert g.launch_plan(cus + 3)[:, 2].tolist() == [cus, 3]
        assert g.launch_kernels(cus + 3) == ["tblock32s_kernel", "tblock32_kernel"]
        assert g.launch_kernels(cus) == ["tblock32s_kernel"]
    finally:
        g.close()
