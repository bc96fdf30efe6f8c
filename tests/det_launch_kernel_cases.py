"""The detector configurations whose kernel per launch is pinned in
tests/golden/det_launch_kernels.json: shared by the recorder (tools/record_launch_kernels.py --det,
which reads the kernels off a kernel trace of one forward) and by
tests/test_det_launch_kernels_gpu.py (which asks the detector, RTMDetector.launch_kernels, and
runs no forward).  The cases: the default switches, each non-default value of each of the nine
library switches (csrc/det_select.h DetSwitches) and MVPOSE_DET_DWPW=0, at size 128 with 3 frames
(ragged planes, the halo kernels' narrow tiles) and at 640 with 2 (the smallest size with both the
80x80 and the 40x40 band planes)."""
import collections
import contextlib
import functools
import os
import re

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "det_launch_kernels.json")

SIZES = [(128, 3), (640, 2)]  # (size, frames)
SETTINGS = [
    {},
    {"MVPOSE_DET_XCD": "0"},
    {"MVPOSE_DET_BAND": "0"},
    {"MVPOSE_DET_BAND": "4"},
    {"MVPOSE_DET_PERS": "0"},
    {"MVPOSE_DET_PERS": "3"},
    {"MVPOSE_DET_PERS_OCC": "1"},
    {"MVPOSE_DET_FOLD": "0"},
    {"MVPOSE_DET_HALO_PERS": "0"},
    {"MVPOSE_DET_HALO_ROWS": "2"},
    {"MVPOSE_DET_LIVE": "0"},
    {"MVPOSE_DET_HEAD_DIRECT": "1"},
    {"MVPOSE_DET_DWPW": "0"},
]
# every switch a case may meet set in the caller's environment; cleared before a case's own are set
CLEARED = tuple(sorted({k for s in SETTINGS for k in s}))

# variant (mvp_det_kernel_name of a mvp_det_kernels id) -> the kernel function's base name as a
# kernel trace shows it, and the template arguments (position: value) the variant fixes; the other
# arguments (cout tile, input chunks, taps, stride, plane width) are functions of the op's shape
VARIANTS = {
    "letterbox": ("letterbox_kernel", {}),
    "stem": ("det_stem_kernel", {0: "false"}),
    "letterbox_stem": ("det_stem_kernel", {0: "true"}),
    "band_8w": ("det_conv_band_kernel", {2: "8"}),           # <W, TR, NWV>
    "band_4w": ("det_conv_band_kernel", {2: "4"}),
    "halo_2row": ("det_conv_halo_kernel", {2: "2", 3: "0"}),  # <BN, NCK, TR, LT>
    "halo": ("det_conv_halo_kernel", {2: "4", 3: "0"}),
    "halo_live3": ("det_conv_halo_kernel", {2: "4", 3: "3"}),
    "halo_pers_lt2": ("det_conv_halo_pers_kernel", {2: "2"}),  # <BN, NCK, LT>
    "halo_pers_lt3": ("det_conv_halo_pers_kernel", {2: "3"}),
    "halo_pers_lt4": ("det_conv_halo_pers_kernel", {2: "4"}),
    "fold_up": ("det_conv1x1_pers_kernel", {3: "1", 4: "1", 5: "1"}),  # <BN, PW, NBUF, KS, STR, FM>
    "fold_ca": ("det_conv1x1_pers_kernel", {3: "1", 4: "1", 5: "2"}),
    "pers_gemm": ("det_conv1x1_pers_kernel", {5: "0"}),
    "gemm": ("det_conv_gemm_kernel", {}),
    "head_staged": ("det_head_staged_kernel", {}),
    "head_direct": ("det_head_kernel", {}),
    "dw5": ("dw5_kernel", {}),
    "dwpw": ("dwpw_kernel", {}),
    "ca_pool": ("ca_pool_kernel", {}),
    "ca_fc": ("ca_fc_kernel", {}),
    "ca_scale": ("ca_scale_kernel", {}),
    "spp": ("spp_kernel", {}),
    "up2": ("up2_kernel", {}),
    "select": ("det_select_kernel", {}),
}

# group: the cases one traced process of the recorder runs
Case = collections.namedtuple("Case", "name group size n env")


def cases():
    out = []
    for size, n in SIZES:
        for env in SETTINGS:
            tag = ",".join(f"{k[len('MVPOSE_DET_'):]}={v}" for k, v in env.items()) or "default"
            out.append(Case(f"{size}x{n}/{tag}", str(size), size, n, env))
    return out


def parse(traced):
    """A traced kernel name -> (base name, template arguments as strings)."""
    m = re.fullmatch(r"([A-Za-z_0-9]+)(?:<(.*)>)?", traced)
    assert m, traced
    return m.group(1), [a.strip() for a in m.group(2).split(",")] if m.group(2) else []


def matches(variant, traced):
    base, fixed = VARIANTS[variant]
    name, args = parse(traced)
    return name == base and all(i < len(args) and args[i] == v for i, v in fixed.items())


@functools.lru_cache(maxsize=None)
def state_dict():
    from mvpose import rtmdet
    return rtmdet.random_state_dict(0)


@contextlib.contextmanager
def built(case):
    """The case's RTMDetector, constructed (and, for the recorder, run) under its switches; the
    environment is restored afterwards."""
    from mvpose import rtmdet
    saved = {k: os.environ.pop(k, None) for k in CLEARED}
    det = None
    try:
        os.environ.update(case.env)
        det = rtmdet.RTMDetector(state_dict(), max_batch=case.n, size=case.size)
        yield det
    finally:
        if det is not None:
            det.close()
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
