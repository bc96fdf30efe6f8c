"""Record the pinned launch plans (tests/golden/launch_plans.json):
    python tools/record_launch_plans.py [OUT.json] [COMMIT]
(COMMIT: the commit the built library comes from, when the tree is not a git checkout.)
For every case of tests/launch_plan_cases.py: the graph's launch plan (mvp_graph_plan: launching
op, route, crops, MACs per launch) and its arena size.  tests/test_launch_plan_gpu.py requires the
built library to reproduce the file exactly, so run this only at a commit whose plans are the
intended ones (a pull request that adds or changes a fusion on purpose), and say which in the
commit message.  Needs a device (mvp_graph_create allocates); runs no forward."""
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [os.path.join(ROOT, "multi-camera_3d_pose_estimation_amd"), os.path.join(ROOT, "tests")]
import launch_plan_cases as lpc  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else lpc.FIXTURE
if len(sys.argv) > 2:
    commit = sys.argv[2]
else:
    try:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True,
                                         stderr=subprocess.DEVNULL).strip()
    except (OSError, subprocess.CalledProcessError):
        commit = None
lines = []
for name, graph, env in lpc.cases():
    rec = lpc.record(graph, env)
    print(f"{name}: {len(rec['plan'])} launches, arena {rec['arena_bytes']} bytes", flush=True)
    lines.append(f"  {json.dumps(name)}: {json.dumps(rec, separators=(',', ':'))}")
with open(out, "w") as f:
    f.write('{\n "recorded_at_commit": %s,\n "cases": {\n%s\n }\n}\n' % (json.dumps(commit), ",\n".join(lines)))
print("wrote", out)
