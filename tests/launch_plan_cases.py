"""The graph configurations whose launch plan and arena size are pinned in
tests/golden/launch_plans.json: shared by the recorder (tools/record_launch_plans.py) and
by tests/test_launch_plan_gpu.py.  A case is (name, graph, environment); building it is
graph construction only (mvp_graph_create allocates, so it needs a device), no forward."""
import functools
import os

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_plans.json")

SPLIT = {"stem": 3, "branch0": 2, "branch1": 5, "branch2": 3}  # test_micro_batched_segments_bitwise_equal's

# every switch a case sets; all of them (and the micro-batch override) are cleared first
SWITCHES = ("MVPOSE_NO_FUSE", "MVPOSE_NO_CATFUSE", "MVPOSE_NO_PAIRFUSE", "MVPOSE_NO_BNECK", "MVPOSE_NO_STEMFUSE",
            "MVPOSE_NO_TRANSFUSE", "MVPOSE_NO_SIBFUSE", "MVPOSE_NO_HEADFUSE", "MVPOSE_NO_TBLOCK", "MVPOSE_NO_TBLOCK64")
CLEARED = SWITCHES + ("MVPOSE_NO_HEAD1X1", "MVPOSE_NO_TBLOCK32S", "MVPOSE_MICRO_BATCH")

ENVS = ([()] + [(s,) for s in SWITCHES[:8]] +
        [("MVPOSE_NO_TBLOCK", "MVPOSE_NO_TBLOCK64"), ("MVPOSE_NO_BNECK", "MVPOSE_NO_CATFUSE")])

# graph -> (max_batch, batch)
GRAPHS = {"hrnet": (8, 7), "hrnet_split": (8, 7), "transition": (2, 2), "sibling3": (2, 2), "sibling2": (2, 2)}


def cases():
    """[(name, graph, env names set to "1")]"""
    out = []
    for graph in ("hrnet", "hrnet_split"):
        for env in ENVS:
            tag = "+".join(e[len("MVPOSE_"):] for e in env) or "default"
            out.append((f"{graph}/{tag}", graph, env))
    out += [(g, g, ()) for g in ("transition", "sibling3", "sibling2")]
    return out


@functools.lru_cache(maxsize=None)
def spec(graph):
    """(GraphSpec, input id, output id), folded once per graph and shared by its cases."""
    from mvpose import hrnet
    if graph == "hrnet":
        return hrnet.build_hrnet_w32(hrnet.random_state_dict(7), dict(hrnet.DEFAULT_MICRO_BATCH))
    if graph == "hrnet_split":
        return hrnet.build_hrnet_w32(hrnet.random_state_dict(7), dict(SPLIT))
    if graph == "transition":
        return hrnet.transition_spec()[:3]
    return hrnet.sibling_spec(n=int(graph[-1]))[:3]


def record(graph, env):
    """Build `graph` with the switches `env` set (the environment is restored afterwards) and
    return {"plan": [[op, route, crops, MACs], ...], "arena_bytes": n}."""
    from mvpose import hrnet
    saved = {k: os.environ.pop(k, None) for k in CLEARED}
    try:
        for k in env:
            os.environ[k] = "1"
        max_batch, batch = GRAPHS[graph]
        g = hrnet.ConvGraph(*spec(graph), max_batch=max_batch)
        out = {"plan": g.launch_plan(batch).tolist(), "arena_bytes": int(g.arena_bytes)}
        g.close()
        return out
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
