"""bench.py's command line: a plain run prints the headline line only and --dump-outputs writes
what the last timed step returned; everything else sits behind --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

BENCH = os.path.join(ROOT, "bench.py")
FULL_ONLY = ("roofline", "stages", "roofline_triangulate", "roofline_triangulate_v4", "sgd", "sgd_extrinsic",
             "host_ingest", "video_decode", "detector", "cpu_baseline")


def test_options_parse_without_a_gpu():
    r = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for opt in ("--full", "--dump-outputs", "--steps", "--warmup", "--gpus"):
        assert opt in r.stdout
    r = subprocess.run([sys.executable, BENCH, "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    T, V = 4, 2
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--frames", str(T),
                        "--views", str(V), "--dump-outputs", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["warmup"] == 1
    assert line["unit"] == "frames/s" and line["higher_is_better"] is True and line["dtype"] == "bf16"
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(T / (line["ms_per_step"] * 1e-3), rel=1e-9)
    assert not [k for k in FULL_ONLY if k in line]
    shapes = {"kpts_2d": ((T, 17, 3, V), np.float32), "heatmaps_2d": ((T, V, 17, 6), np.float64),
              "kpts_3d": ((T, 17, 3), np.float32)}
    assert sorted(os.listdir(out)) == sorted(n + ".npy" for n in shapes)
    for name, (shape, dtype) in shapes.items():
        a = np.load(out / (name + ".npy"))
        assert a.shape == shape and a.dtype == dtype
        assert np.isfinite(a).all()
