"""The graph configurations whose kernel per launch is pinned in tests/golden/launch_kernels.json:
shared by the recorder (tools/record_launch_kernels.py, which reads the kernels off a kernel
trace of one forward) and by tests/test_launch_kernels_gpu.py (which asks the graph,
ConvGraph.launch_kernels, and runs no forward).  The cases are those of launch_plan_cases.py plus
the BasicBlock planes of test_conv_planes_gpu.py under its three kernel modes, each at batch 7 as
the launchers' own rule has it and with MVPOSE_CROP_STREAM=1."""
import collections
import contextlib
import functools
import os

import launch_plan_cases as lpc

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_kernels.json")

PLANES = [(32, 64, 48), (64, 32, 24), (128, 16, 12), (256, 8, 6), (64, 64, 48)]  # test_conv_planes_gpu.PLANES
MODES = {  # test_conv_planes_gpu.MODES, as the switches each leaves set to "1" / "0"
    "generic": {"MVPOSE_NO_TCONV": "1", "MVPOSE_NO_TBLOCK": "1"},
    "tconv": {"MVPOSE_NO_TCONV": "0", "MVPOSE_NO_TBLOCK": "0"},
    "tconv64": {"MVPOSE_NO_TCONV": "0", "MVPOSE_NO_TBLOCK": "0", "MVPOSE_TCONV16": "0"},
}
PLANE_BATCH = 7

# every switch a case may meet set in the caller's environment; cleared before a case's own are set
CLEARED = lpc.CLEARED + ("MVPOSE_NO_TCONV", "MVPOSE_TCONV16", "MVPOSE_NO_S2CONV", "MVPOSE_CROP_STREAM",
                         "MVPOSE_STEM2_TILE", "MVPOSE_S2_TILE")

# group: the cases one traced process of the recorder runs
Case = collections.namedtuple("Case", "name group graph env max_batch batch")


def cases():
    out = []
    for name, graph, env in lpc.cases():
        group = graph if graph.startswith("hrnet") else "small"
        out.append(Case(name, group, graph, {k: "1" for k in env}, *lpc.GRAPHS[graph]))
    for c, h, w in PLANES:
        for mode, env in MODES.items():
            for stream in (False, True):
                e = dict(env, MVPOSE_CROP_STREAM="1") if stream else dict(env)
                name = f"block/{c}x{h}x{w}/{mode}" + ("+CROP_STREAM" if stream else "")
                out.append(Case(name, "block", (c, h, w), e, PLANE_BATCH, PLANE_BATCH))
    return out


@functools.lru_cache(maxsize=None)
def spec(graph):
    """(GraphSpec, input id, output id), folded once per graph and shared by its cases."""
    if isinstance(graph, str):
        return lpc.spec(graph)
    from mvpose import hrnet
    return hrnet.basic_block_spec(*graph, seed=3)[:3]


@contextlib.contextmanager
def built(case):
    """The case's ConvGraph, constructed (and, for the recorder, run) under its switches; the
    environment is restored afterwards."""
    from mvpose import hrnet
    saved = {k: os.environ.pop(k, None) for k in CLEARED}
    g = None
    try:
        os.environ.update(case.env)
        g = hrnet.ConvGraph(*spec(case.graph), max_batch=case.max_batch)
        yield g
    finally:
        if g is not None:
            g.close()
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
