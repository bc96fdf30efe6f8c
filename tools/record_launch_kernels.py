"""Record the pinned kernel per launch (tests/golden/launch_kernels.json) from kernel traces:
    python tools/record_launch_kernels.py [OUT.json] [COMMIT] [GROUP ...]
For every case of tests/launch_kernel_cases.py, the kernels ONE forward actually launches, read
off a `rocprofv3 --kernel-trace` of it (no counters): each Kernel_Name reduced by
tools/fwd_breakdown.py's fam() and then to the function's base name (template arguments dropped).
The cases of a group run in one traced child process, one graph and one forward each, the groups
one process at a time, each under its own time limit.  Nothing here asks the library which
kernel it chose, so the file is evidence for tests/test_launch_kernels_gpu.py, which does: run
this at a commit whose kernels are the intended ones and say which in the commit message.
    python tools/record_launch_kernels.py --forward GROUP LENS.json    (the traced child)
    python tools/record_launch_kernels.py --det [OUT.json] [COMMIT]
The person detector's cases (tests/det_launch_kernel_cases.py -> tests/golden/
det_launch_kernels.json, for tests/test_det_launch_kernels_gpu.py) the same way, one traced child
per size; here each name keeps its template arguments (the detector reports the variant within a
kernel family), and a case's launches are the trace's up to its det_select_kernel, the last launch
of a detector forward, so the recording needs nothing from the library but the forward.
    python tools/record_launch_kernels.py --det-forward GROUP ORDER.json    (the traced child)"""
import csv
import glob
import json
import os
import re
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [os.path.join(ROOT, "multi-camera_3d_pose_estimation_amd"), os.path.join(ROOT, "tests")]
import launch_kernel_cases as lkc  # noqa: E402


def fam(r):  # tools/fwd_breakdown.py
    n = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "")
    return re.sub(r"\(.*", "", n).replace("mvp::", "")[:64]


def forward_launches(trace_csv):
    """The trace's forward launches in start order: the library's kernels but for the weight
    packing of graph construction (inputs come from torch, weight copies from the runtime)."""
    rows = sorted(csv.DictReader(open(trace_csv)), key=lambda r: int(r["Start_Timestamp"]))
    return [r for r in rows if "mvp::" in r["Kernel_Name"] and "_pack_kernel" not in r["Kernel_Name"]]


def child(group, lens_out):
    import torch
    from mvpose import hrnet
    lens = {}
    for case in (c for c in lkc.cases() if c.group == group):
        spec, xi, yo = lkc.spec(case.graph)
        h, w, c, _ = spec.tensors[xi]
        oh, ow, oc, odt = spec.tensors[yo]
        with lkc.built(case) as g:
            x = torch.randn((case.batch, h, w, c), device="cuda").bfloat16()
            out = torch.empty(case.batch * oh * ow * oc * (2 if odt == hrnet.DT_BF16 else 4), dtype=torch.uint8,
                              device="cuda")
            g.run(x, out)
            torch.cuda.synchronize()
            lens[case.name] = len(g.launch_plan(case.batch))
    json.dump(lens, open(lens_out, "w"))


def traced_child(d, *child_args):
    """Runs this script's child mode under a kernel trace in directory d; the trace's csv."""
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "log.txt"), "w") as log:
        subprocess.run(["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--output-format", "csv",
                        "-d", d, "-o", "run", "--", sys.executable, os.path.abspath(__file__), *child_args],
                       stdout=log, stderr=subprocess.STDOUT, check=True)
    (trace,) = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    return trace


def head_commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True,
                                       stderr=subprocess.DEVNULL).strip()
    except (OSError, subprocess.CalledProcessError):
        return None


def write_fixture(out, commit, lines):
    with open(out, "w") as f:
        f.write('{\n "recorded_by": "tools/record_launch_kernels.py (rocprofv3 --kernel-trace of one forward per case)",\n'
                ' "recorded_at_commit": %s,\n "cases": {\n%s\n }\n}\n' % (json.dumps(commit), ",\n".join(lines)))
    print("wrote", out)


def det_child(group, order_out):
    import numpy as np
    import torch
    import det_launch_kernel_cases as dlc
    order = []
    for case in (c for c in dlc.cases() if c.group == group):
        frames = torch.from_numpy(np.random.default_rng(5).integers(0, 256, (case.n, case.size * 9 // 8, 2 * case.size, 3),
                                                                    dtype=np.uint8)).cuda()
        with dlc.built(case) as det:
            det.detect(frames)
            torch.cuda.synchronize()
        order.append(case.name)
    json.dump(order, open(order_out, "w"))


def det_main(args):
    import det_launch_kernel_cases as dlc
    out = args[0] if args else dlc.FIXTURE
    commit = args[1] if len(args) > 1 else head_commit()
    work = os.path.splitext(out)[0] + "_traces"
    lines = []
    for group in sorted({c.group for c in dlc.cases()}, key=int):
        d = os.path.join(work, group)
        order_file = os.path.join(d, "order.json")
        trace = traced_child(d, "--det-forward", group, order_file)
        order = json.load(open(order_file))
        rows = [r for r in forward_launches(trace) if "det_pack_" not in r["Kernel_Name"]]
        ends = [i for i, r in enumerate(rows) if "det_select_kernel" in r["Kernel_Name"]]
        assert len(ends) == len(order) and ends[-1] == len(rows) - 1, f"{group}: {len(ends)} forwards, {len(order)} cases"
        at = 0
        for name, end in zip(order, ends):
            names = [fam(r) for r in rows[at:end + 1]]
            for r, k in zip(rows[at:end + 1], names):  # fam() cuts at 64 characters: the template arguments must survive it
                assert k.count("<") == k.count(">") and len(k) < 64, r["Kernel_Name"]
            at = end + 1
            print(f"{name}: {len(names)} launches, {len(set(names))} kernels", flush=True)
            lines.append(f"  {json.dumps(name)}: {json.dumps(names, separators=(',', ':'))}")
    write_fixture(out, commit, lines)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else lkc.FIXTURE
    commit = sys.argv[2] if len(sys.argv) > 2 else head_commit()
    groups = sys.argv[3:] or sorted({c.group for c in lkc.cases()})
    work = os.path.splitext(out)[0] + "_traces"
    lines = []
    for group in groups:
        d = os.path.join(work, group)
        lens_file = os.path.join(d, "lens.json")
        trace = traced_child(d, "--forward", group, lens_file)
        lens = json.load(open(lens_file))
        rows = forward_launches(trace)
        assert len(rows) == sum(lens.values()), f"{group}: {len(rows)} traced launches, plans have {sum(lens.values())}"
        at = 0
        for name, n in lens.items():  # in the order the child ran them
            names = [fam(r).split("<")[0] for r in rows[at:at + n]]
            at += n
            print(f"{name}: {n} launches, {len(set(names))} kernels", flush=True)
            lines.append(f"  {json.dumps(name)}: {json.dumps(names, separators=(',', ':'))}")
    write_fixture(out, commit, lines)


if __name__ == "__main__":
    if sys.argv[1:2] == ["--forward"]:
        child(sys.argv[2], sys.argv[3])
    elif sys.argv[1:2] == ["--det-forward"]:
        det_child(sys.argv[2], sys.argv[3])
    elif sys.argv[1:2] == ["--det"]:
        det_main(sys.argv[2:])
    else:
        main()
