"""The HRNet graph's compiled launch plan is pinned: for every configuration of
launch_plan_cases.py (both micro-batch layouts under each fusion switch, and the transition /
sibling kernel-test graphs) mvp_graph_plan's records and the arena size must equal
tests/golden/launch_plans.json exactly.  The fixture is regenerated (tools/record_launch_plans.py)
only by a change that alters a fusion on purpose.  Graph construction only: no forward runs."""
import json

import pytest
import torch

import launch_plan_cases as lpc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pinned():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    with open(lpc.FIXTURE) as f:
        return json.load(f)["cases"]


def test_fixture_has_every_case(pinned):
    assert sorted(pinned) == sorted(name for name, _, _ in lpc.cases())


@pytest.mark.parametrize("name,graph,env", lpc.cases(), ids=[c[0] for c in lpc.cases()])
def test_launch_plan_is_pinned(pinned, name, graph, env):
    got = lpc.record(graph, env)
    want = pinned[name]
    assert got["arena_bytes"] == want["arena_bytes"]
    assert len(got["plan"]) == len(want["plan"])
    for i, (g, w) in enumerate(zip(got["plan"], want["plan"])):
        assert g == w, f"launch {i}: {{op, route, crops, MACs}} {g} != pinned {w}"
