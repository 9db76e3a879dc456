"""The producer side of the streamed gather (csrc/interp_stream.hip): the wrapped loads of the edge column pencils, the
bit mask of the planes a sweep stages, the two alternating tiles.

The streamed gather is chosen for big work items only; NFFT_HIP_STREAM_MIN=1 puts it on problems the float64 oracle can
check (as tests/test_gpu_parity.py does), in a child process because the switches are read once.  The 64^3 grid (N = 32)
takes the narrow tiling below 30 000 points, which has no streamed gather: NFFT_HIP_SMALL_NARROW=0 keeps it on the
matrix-core kernels.  Shapes: N = 32 (two column pencils of 64 padded columns on a row of 64: every pencil is an edge
pencil) with m = 1, 4, 7 (chunks of 13, 7 and 1 slabs), and N = 80 with m = 4 (three column pencils, the last one
partial), about 4 000 points each.

Two children run every shape once -- the default launch and NFFT_HIP_WORK_LIST=1 (the persistent form) -- and report
whether five repeated calls gave identical bits and a digest of the output bits; the first one also reports the error of
nfft_forward against oracle/nfft_ref over exactly the points of each set (the second one's outputs must equal the
first's bit for bit, so its error is the same).  The tests below read the two reports.
"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

T1W = 2e-6  # tests/test_gpu_parity.py: matrix-core kernels against the float64 restatement of the algorithm
SHAPES = [(32, 1), (32, 4), (32, 7), (80, 4)]
SETS = ["wrap_last", "wrap_middle", "wrap_both", "two_slab_ranges"]

CHILD = r'''
import hashlib, json, os, sys
import numpy as np, torch
sys.path.insert(0, %(root)r)
import torch_nfft_amd as tn
from torch_nfft_amd import ops
from oracle import nfft_ref

def point_set(kind, rng, N, m, n):
    M = 2 * N
    pos = (rng.random((n, 3)) - 0.5).astype(np.float32)
    def near_boundary(k):
        # within (m + 1) / M of +-0.5: the window of 2m + 2 taps wraps around the axis
        d = rng.random(k) * (m + 1) / M
        return np.where(rng.integers(0, 2, k) == 0, -0.5 + d, 0.5 - d).astype(np.float32)
    if kind in ("wrap_last", "wrap_both"):
        pos[:, 2] = near_boundary(n)
    if kind in ("wrap_middle", "wrap_both"):
        pos[:, 1] = near_boundary(n)
    if kind == "two_slab_ranges":
        # two ranges of three slabs, far apart along the first axis: most planes of a sweep are needed by no chunk
        cell = np.where(rng.integers(0, 2, n) == 0, 5, M // 2 + 7) + rng.integers(0, 3, n)
        pos[:, 0] = ((cell + rng.random(n)) / M - 0.5).astype(np.float32)
    return np.clip(pos, -0.5, np.nextafter(np.float32(0.5), np.float32(0))).astype(np.float32)

report = {}
for N, m in %(shapes)r:
    rng = np.random.default_rng(1000 * N + m)
    n = 4000
    xh = (rng.standard_normal((1, N, N, N)) + 1j * rng.standard_normal((1, N, N, N))).astype(np.complex64)
    xt = torch.from_numpy(xh).cuda()
    for kind in %(sets)r:
        pos = point_set(kind, rng, N, m, n)
        pt = torch.from_numpy(pos).cuda()
        ys = [tn.nfft_forward(xt, pt, None, cutoff=m) for _ in range(5)]
        ops.check_status()
        y = ys[0].cpu().numpy()
        err = None
        if os.environ.get("STAGING_TEST_ORACLE") == "1":
            ref = nfft_ref.nfft_forward(xh, pos, None, m=m)
            err = float(np.linalg.norm(y - ref) / np.linalg.norm(ref))
        print("CASE", N, m, kind, err, flush=True)
        report["%%d,%%d,%%s" %% (N, m, kind)] = {
            "err": err, "repeatable": all(bool(torch.equal(ys[0], t)) for t in ys[1:]),
            "digest": hashlib.sha256(np.ascontiguousarray(y).tobytes()).hexdigest()}
print("REPORT " + json.dumps(report))
'''


def _run_child(extra_env):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = CHILD % {"root": root, "shapes": SHAPES, "sets": SETS}
    env = dict(os.environ, NFFT_HIP_STREAM_MIN="1", NFFT_HIP_SMALL_NARROW="0", **extra_env)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:] + out.stdout[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("REPORT ")]
    assert line, out.stdout[-2000:]
    return json.loads(line[0][7:])


@pytest.fixture(scope="module")
def reports():
    # (the oracle runs in the first child only: the second one's outputs are compared with the first's bit for bit)
    return {"default": _run_child({"STAGING_TEST_ORACLE": "1"}), "work_list": _run_child({"NFFT_HIP_WORK_LIST": "1"})}


@pytest.mark.parametrize("N,m", SHAPES)
@pytest.mark.parametrize("kind", SETS[:3])
def test_windows_that_wrap_in_the_pencil_axes(reports, N, m, kind):
    """(a) Every window wraps in the last axis, in the middle axis, or in both: the halves of a tile that begin beyond
    column M - 1, the halves put together from both ends of a row, the wrapped rows."""
    assert reports["default"]["%d,%d,%s" % (N, m, kind)]["err"] < T1W


@pytest.mark.parametrize("N,m", SHAPES)
def test_sweeps_that_skip_most_planes(reports, N, m):
    """(b) The points occupy two short slab ranges far apart: the plane mask of a sweep has long gaps, and the device
    reports no fault (the child calls ops.check_status() after every set)."""
    assert reports["default"]["%d,%d,two_slab_ranges" % (N, m)]["err"] < T1W


@pytest.mark.parametrize("N,m", SHAPES)
def test_repeated_calls_and_both_launch_forms_give_identical_bits(reports, N, m):
    """(c) Five calls in a row give the same bits, and so do the per-entry launch and the persistent one."""
    for kind in SETS:
        key = "%d,%d,%s" % (N, m, kind)
        assert reports["default"][key]["repeatable"] and reports["work_list"][key]["repeatable"], key
        assert reports["default"][key]["digest"] == reports["work_list"][key]["digest"], key
