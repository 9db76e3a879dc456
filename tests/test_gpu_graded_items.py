"""Work items of the matrix-core kernels (csrc/common.h, plan layout): every wide plan cuts its pencils into items from
the pencil's own slab offsets -- equal ranges of slabs by default, or (NFFT_HIP_GRADE) fewer items for light pencils and a
graded tail -- and every launch reads them from the plan's list in launch order.

* results against oracle.nfft_ref at the matrix-core tolerance, on shapes that reach every cut (1-4 items per pencil,
  grids that are no multiple of the chunk length, chunk lengths 11 / 7 / 3, empty items and windows across the periodic
  boundary, two point sets of very different size, the scatter / paired / wave-per-column kernels), each on the default
  route, with the streamed gather forced, from the persistent launch, and each of these with the graded cut
  (NFFT_HIP_GRADE=2: at sizes the oracle can check a launch is one round of workgroups, which =1 leaves to the equal cut);
* the gather's values do not depend on the cut: bitwise equal across cuts;
* the list itself: an exact tiling of every pencil, at most 128 slabs per item, launch order, capacity -- and for the
  flagship plan (N = 256, 10^7 uniform points) the scheduling simulation of scripts/item_schedule_sim.py.
"""
import concurrent.futures
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T1W = 2e-6  # the matrix-core tolerance of tests/test_gpu_parity.py (relative L2)

# name: (N, m, points per set, real columns, kind).  The oracle costs ~0.25 us per point, tap and column on the host, so only
# the first case holds the full 6e4 points; the others are the smallest that still give every pencil several chunks.
CASES = {
    "n64_m4_uniform": (64, 4, (60000,), 1, "uniform"),   # M = 128: 6 x 3 pencils, light edge pencils (1-4 items each when
                                                         # the plan is cut as for a launch of several rounds)
    "n48_m4": (48, 4, (20000,), 1, "uniform"),           # M = 96: not a multiple of the chunk length 7
    "n64_m2_pair": (64, 2, (20000,), 2, "uniform"),      # chunk length 11; two real columns: paired owner-computes kernel
    "n64_m6": (64, 6, (8000,), 1, "uniform"),            # chunk length 3, the 16-owner layout
    "n64_m4_band": (64, 4, (20000,), 1, "band"),         # empty items, windows that wrap the periodic boundary
    "n64_m4_two_sets": (64, 4, (12000, 500), 2, "uniform"),
    "n64_m4_six_cols": (64, 4, (5000,), 6, "uniform"),   # wave-per-column gather
}
VARIANTS = {
    "default": {},
    "stream": {"NFFT_HIP_STREAM_MIN": "1"},
    "work_list": {"NFFT_HIP_WORK_LIST": "1"},
    "graded": {"NFFT_HIP_GRADE": "2"},
    "graded_stream": {"NFFT_HIP_GRADE": "2", "NFFT_HIP_STREAM_MIN": "1"},
    "graded_work_list": {"NFFT_HIP_GRADE": "2", "NFFT_HIP_WORK_LIST": "1"},
}


def _make_case(name):
    """Inputs and float64 references of a case (host only)."""
    sys.path.insert(0, ROOT)
    from oracle import nfft_ref
    N, m, sizes, cols, kind = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 100)
    n = sum(sizes)
    pos = (rng.random((n, 3)) - 0.5).astype(np.float32)
    if kind == "band":  # slabs (axis 0) in [0.3, 0.5) and [-0.5, -0.4) only
        u = rng.random(n)
        pos[:, 0] = np.where(u < 2.0 / 3.0, 0.3 + 0.3 * u, -0.5 + 0.3 * (u - 2.0 / 3.0)).astype(np.float32)
        pos[:, 0] = np.clip(pos[:, 0], -0.5, np.nextafter(np.float32(0.5), np.float32(0)))
    batch = np.repeat(np.arange(len(sizes)), sizes).astype(np.int64)
    x = rng.standard_normal((n, cols) if cols > 1 else (n,)).astype(np.float32)
    ya = nfft_ref.nfft_adjoint(x, pos, batch, N=N, m=m)
    spec = ya.astype(np.complex64)
    fw = nfft_ref.nfft_forward(spec, pos, batch, m=m)
    return name, dict(pos=pos, batch=batch, x=x, adjoint=ya, spec=spec, forward=fw)


@pytest.fixture(scope="module")
def case_dir(tmp_path_factory):
    """The cases' inputs and references, computed once (in parallel on the host) and shared by every variant."""
    d = tmp_path_factory.mktemp("graded_items")
    with concurrent.futures.ProcessPoolExecutor(max_workers=min(len(CASES), os.cpu_count() or 1)) as ex:
        for name, arrays in ex.map(_make_case, sorted(CASES)):
            np.savez(os.path.join(str(d), name + ".npz"), **arrays)
    return str(d)


# Conditions on a plan's ordered list, shared by the worker processes and the in-process test of the flagship plan
LIST_CHECK = r'''
import ctypes
import numpy as np


def read_work_list(lib, prob, plan, which, stream):
    """(info, set headers [sets, 2], entries [work_cap, 4]) of a plan through the debug entry nfft_dbg_work_list."""
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    lib.nfft_dbg_work_list.argtypes = [ctypes.c_void_p, vp, ctypes.c_int, vp, vp, vp, i64, vp]
    lib.nfft_dbg_work_list.restype = ctypes.c_int
    info = np.zeros(8, dtype=np.int64)
    hdr = np.zeros((int(prob.batch_size), 2), dtype=np.int32)
    cap = 1 << 20
    entries = np.zeros((cap, 4), dtype=np.int32)
    rc = lib.nfft_dbg_work_list(ctypes.byref(prob), vp(plan.data_ptr()), which, vp(info.ctypes.data), vp(hdr.ctypes.data),
                                vp(entries.ctypes.data), cap, stream)
    assert rc == 0, rc
    return info, hdr, entries[:min(cap, int(info[2]))]


def check_work_list(info, hdr, entries, set_points, ordered):
    """The items of every (set, pencil) tile [0, M) exactly once; no item exceeds 128 slabs; the entry count is within
    work_cap and the sets' parts follow each other.  `ordered`: sizes are non-increasing by the ordering kernel's size classes
    within a set -- the graded cut and every plan of the persistent launch; else the list is in grid order: a balanced plan
    of the default equal cut is NOT put biggest first, because with (nearly) equal items that order measured slower than
    neighbouring ranges side by side (profiles/r08_graded_items.md)."""
    total, listed, cap, per_entry, pencils, nsets, M, runs = (int(v) for v in info)
    assert 0 < total <= cap, (total, cap)
    assert int(hdr[:, 0].sum()) == total, (hdr, total)
    start = 0
    for b in range(nsets):
        cnt, first = int(hdr[b, 0]), int(hdr[b, 1])
        assert first == start, (b, first, start)
        start += cnt
        e = entries[first:first + cnt]
        assert ((e[:, 0] >= b * pencils) & (e[:, 0] < (b + 1) * pencils)).all()
        slabs = e[:, 2] - e[:, 1]
        assert (slabs >= 1).all() and (slabs <= 128).all(), (slabs.min(), slabs.max())
        assert (e[:, 3] >= 0).all() and int(e[:, 3].sum()) == int(set_points[b]), (int(e[:, 3].sum()), set_points[b])
        for p in range(b * pencils, (b + 1) * pencils):
            q = e[e[:, 0] == p]
            q = q[np.argsort(q[:, 1])]
            assert len(q) >= 1 and q[0, 1] == 0 and q[-1, 2] == M and (q[1:, 1] == q[:-1, 2]).all(), (p, q)
        # work_order_kernel: class = 15 - min(15, int(float(points) * (16.0f / largest))), 0 = biggest, in float32
        scale = np.float32(16.0) / np.float32(max(1, int(e[:, 3].max())))
        cls = 15 - np.minimum(15, (e[:, 3].astype(np.float32) * scale).astype(np.int32))
        grid_order = (e[:, 0] * M + e[:, 1]).astype(np.int64)
        if ordered:
            assert (np.diff(cls) >= 0).all(), cls
        else:
            assert (np.diff(grid_order) > 0).all()
        # a balanced plan runs one workgroup per entry: the launch must have one for every entry of the set
        assert listed or cnt <= per_entry, (cnt, per_entry)
    return total
'''

WORKER = LIST_CHECK + r'''
import json, os, sys
sys.path.insert(0, %(root)r)
import torch
import torch_nfft_amd as tn
from torch_nfft_amd import ops, _lib

lib = _lib.load()
cases = json.loads(%(cases)r)
out = {}
for name, (N, m, sizes, cols, kind) in sorted(cases.items()):
    a = np.load(os.path.join(%(case_dir)r, name + ".npz"))
    pos, batch = torch.from_numpy(a["pos"]).cuda(), torch.from_numpy(a["batch"]).cuda()
    y = tn.nfft_adjoint(torch.from_numpy(a["x"]).cuda(), pos, batch, bandwidth=N, cutoff=m)
    spec = torch.from_numpy(a["spec"]).cuda()
    f = tn.nfft_forward(spec, pos, batch, cutoff=m)
    fr = tn.nfft_forward(spec, pos, batch, cutoff=m, real_output=True)
    ops.check_status()
    rel = lambda got, ref: float(np.linalg.norm((got - ref).ravel()) / np.linalg.norm(ref.ravel()))
    errs = [rel(y.cpu().numpy(), a["adjoint"]), rel(f.cpu().numpy(), a["forward"]), rel(fr.cpu().numpy(), a["forward"].real)]
    # the plan's list, for the gather's plan and the spreading kernel's
    n = int(pos.shape[0])
    prob = _lib.Problem(3, n, cols, len(sizes), N, m)
    plan = torch.empty(lib.nfft_hip_plan_bytes(ctypes.byref(prob)), dtype=torch.uint8, device="cuda")
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.nfft_hip_plan_points(ctypes.byref(prob), ctypes.c_void_p(pos.data_ptr()), ctypes.c_void_p(batch.data_ptr()),
                                        ctypes.c_void_p(plan.data_ptr()), plan.numel(), s))
    items = []
    for which in (0, 1):
        info, hdr, entries = read_work_list(lib, prob, plan, which, s)
        if which == 0:
            set_points = sizes
        else:  # (the owned plan has an entry per tile a point's window touches)
            set_points = [int(entries[int(hdr[b, 1]):int(hdr[b, 1]) + int(hdr[b, 0]), 3].sum()) for b in range(len(sizes))]
            assert all(p >= q for p, q in zip(set_points, sizes))
        # launch order: biggest first for the graded cut and for every plan of the persistent launch (info[1]); a balanced
        # plan of the equal cut stays in grid order
        items.append(check_work_list(info, hdr, entries, set_points, ordered=bool(%(graded)r or info[1])))
        per_pencil = np.bincount(entries[:items[-1], 0], minlength=int(info[4]) * int(info[5]))
        items.append([int(per_pencil.min()), int(per_pencil.max()), int(info[1])])
    ops.check_status()
    # the gathers of the two forward transforms (2 cols and cols real planes per point set) by api.hip plan_route
    gathers = [_lib.route(prob, 2 * cols).gather, _lib.route(prob, cols).gather]
    out[name] = {"errors": errs, "items": items, "gathers": gathers}
print("RESULT " + json.dumps(out))
'''


def _run(code, env_extra, timeout=600):
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env_extra), capture_output=True, text=True,
                         timeout=timeout)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-3000:])
    return [l for l in out.stdout.splitlines() if l.startswith("RESULT ")][0][len("RESULT "):]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_results_and_lists(case_dir, variant):
    """Adjoint and forward (complex and real output) of every case against oracle.nfft_ref at T1W, a clean device status
    afterwards, and the conditions on the plans' lists (check_work_list), in a process of its own per route."""
    code = WORKER % {"root": ROOT, "cases": json.dumps(CASES), "case_dir": case_dir, "graded": "NFFT_HIP_GRADE" in VARIANTS[variant]}
    res = json.loads(_run(code, VARIANTS[variant]))
    assert sorted(res) == sorted(CASES)
    for name in sorted(res):
        print(variant, name, "adjoint %.2e forward %.2e forward(real) %.2e" % tuple(res[name]["errors"]), "items", res[name]["items"])
    for name in sorted(res):
        assert max(res[name]["errors"]) < T1W, (name, res[name])
    # which gather ran: from four real planes per point set up the wave-per-column kernel whatever the switches say, below that
    # the streamed one where NFFT_HIP_STREAM_MIN forces it, else the plane ring -- so with two columns (n64_m2_pair,
    # n64_m4_two_sets) only the real-output transform reaches the streamed gather, and n64_m4_six_cols never does
    few = "stream" if "NFFT_HIP_STREAM_MIN" in VARIANTS[variant] else "ring"
    for name in sorted(res):
        cols = CASES[name][3]
        assert res[name]["gathers"] == ["cols" if 2 * cols >= 4 else few, "cols" if cols >= 4 else few], (name, res[name]["gathers"])
    # the equal cut: four items for every pencil; the graded cut (NFFT_HIP_GRADE=2): light edge pencils get fewer items,
    # not smaller ones
    lo, hi, _ = res["n64_m4_uniform"]["items"][1]
    assert (lo, hi) == ((1, 4) if "NFFT_HIP_GRADE" in VARIANTS[variant] else (4, 4)), (lo, hi)


# ---- the gather does not depend on the cut -------------------------------------------------------------------------------
# The flagship shape (N = 256, 10^7 uniform points, forward only: a millisecond of gather): 230 pencils of 6 ranges, several
# rounds of workgroups, no range near 1.5 x the target -- a BALANCED plan, run by the one-workgroup-per-entry launch, with
# the finer last pencils, and the streamed gather.  (At N = 64 every dense plan is cut by points and runs persistently.)
GATHER = LIST_CHECK + r'''
import hashlib, json, sys
sys.path.insert(0, %(root)r)
import torch
import torch_nfft_amd as tn
from torch_nfft_amd import ops, _lib
lib = _lib.load()
N, m, n = 256, 4, 10000000
gen = torch.Generator(device="cuda").manual_seed(5)
pos = torch.rand((n, 3), generator=gen, device="cuda") - 0.5
spec = torch.randn((1, N, N, N, 2), generator=gen, device="cuda")
f = tn.nfft_forward(torch.view_as_complex(spec), pos, None, cutoff=m)
ops.check_status()
prob = _lib.Problem(3, n, 1, 1, N, m)
plan = torch.empty(lib.nfft_hip_plan_bytes(ctypes.byref(prob)), dtype=torch.uint8, device="cuda")
s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
_lib.check(lib.nfft_hip_plan_points(ctypes.byref(prob), ctypes.c_void_p(pos.data_ptr()), None, ctypes.c_void_p(plan.data_ptr()),
                                    plan.numel(), s))
info, hdr, entries = read_work_list(lib, prob, plan, 0, s)
total = check_work_list(info, hdr, entries, [n], ordered=%(ordered)r)
ranges = entries[:total, :3]
ranges = ranges[np.lexsort((ranges[:, 1], ranges[:, 0]))]  # the cut itself, whatever its launch order
print("RESULT " + json.dumps({"gather": hashlib.sha256(torch.view_as_real(f).cpu().numpy().tobytes()).hexdigest(),
                              "cut": hashlib.sha256(ranges.tobytes()).hexdigest(), "items": total, "persistent": int(info[1])}))
'''
# name: (environment, list biggest first, persistent launch)
GATHER_VARIANTS = {
    "default": ({}, False, 0),                                     # equal cut, finer last pencils, grid order
    "no_fine_tail": ({"NFFT_HIP_FINE_TAIL": "0"}, False, 0),       # 6 ranges for every pencil
    "graded": ({"NFFT_HIP_GRADE": "1"}, True, 0),                  # items by points, graded tails, biggest first
    "items_per_cu_3": ({"NFFT_HIP_ITEMS_PER_CU": "3.0"}, False, 0),  # 4 ranges per pencil
    "work_list": ({"NFFT_HIP_WORK_LIST": "1"}, True, 1),           # the default cut from the persistent launch
    "graded_work_list": ({"NFFT_HIP_GRADE": "1", "NFFT_HIP_WORK_LIST": "1"}, True, 1),
}


def _gather(variant):
    env, ordered, _ = GATHER_VARIANTS[variant]
    return json.loads(_run(GATHER % {"root": ROOT, "ordered": ordered}, env))


@pytest.fixture(scope="module")
def gather_default():
    return _gather("default")


@pytest.mark.gpu
@pytest.mark.parametrize("variant", sorted(GATHER_VARIANTS))
def test_gather_bitwise_independent_of_the_cut(gather_default, variant):
    """A point's value depends on its chunk and plane tiles, not on which item swept it: for one spectrum and point set
    nfft_forward is bitwise equal under the default cut (run one workgroup per list entry), without the finer last pencils,
    under the graded cut, with another item size, and from the persistent launch.  The plans' lists say which launch ran
    and that the cuts really differ.  (On the parent commit NFFT_HIP_ITEMS_PER_CU = 5.4 and 9.0 give equal bits too.)"""
    got = gather_default if variant == "default" else _gather(variant)
    print(variant, got)
    assert got["persistent"] == GATHER_VARIANTS[variant][2]
    assert got["gather"] == gather_default["gather"]
    same_cut = variant in ("default", "work_list")
    assert (got["cut"] == gather_default["cut"]) == same_cut, (got["items"], gather_default["items"])
    if variant == "default":
        assert got["items"] == (230 + 22) * 6  # ceil(256 / 12) = 22 pencils of 12 ranges


# ---- the flagship plan's list ---------------------------------------------------------------------------------------------
FLAGSHIP = LIST_CHECK + r'''
import importlib.util, json, os, sys
sys.path.insert(0, %(root)r)
import torch
from torch_nfft_amd import _lib
spec = importlib.util.spec_from_file_location("item_schedule_sim", os.path.join(%(root)r, "scripts", "item_schedule_sim.py"))
sim = importlib.util.module_from_spec(spec)
spec.loader.exec_module(sim)
lib = _lib.load()
n, N, m = 10_000_000, 256, 4
gen = torch.Generator(device="cuda").manual_seed(1)
pos = torch.rand((n, 3), generator=gen, device="cuda") - 0.5
prob = _lib.Problem(3, n, 1, 1, N, m)
plan = torch.empty(lib.nfft_hip_plan_bytes(ctypes.byref(prob)), dtype=torch.uint8, device="cuda")
s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
_lib.check(lib.nfft_hip_plan_points(ctypes.byref(prob), ctypes.c_void_p(pos.data_ptr()), None, ctypes.c_void_p(plan.data_ptr()),
                                    plan.numel(), s))
info, hdr, entries = read_work_list(lib, prob, plan, 0, s)
total = check_work_list(info, hdr, entries, [n], ordered=%(ordered)r)
_lib.check_status()
span, ideal, util = sim.simulate_list(entries[:total], 256)
print("RESULT " + json.dumps({"items": total, "listed": int(info[1]), "span": span, "ideal": ideal}))
'''


@pytest.mark.gpu
@pytest.mark.parametrize("cut", ["equal", "graded"])
def test_flagship_list(cut):
    """N = 256, m = 4, 10^7 uniform points (plan only): the conditions on the list, and the committed list-scheduling
    simulation with its cost constants (0.624 us per K-block, 16 us per item) on 256 CUs gives a span of at most 1.03 x its
    ideal: for the default cut (equal ranges of slabs in grid order, twice as many for the last 22 pencils: 1.021; without
    them 1.086) and for the graded cut (NFFT_HIP_GRADE=1: 1.012)."""
    env = {"NFFT_HIP_GRADE": "1"} if cut == "graded" else {}
    res = json.loads(_run(FLAGSHIP % {"root": ROOT, "ordered": cut == "graded"}, env))
    print(cut, "items %d (%.2f per CU), span %.1f us, ideal %.1f us, span / ideal %.4f"
          % (res["items"], res["items"] / 256, res["span"], res["ideal"], res["span"] / res["ideal"]))
    assert res["listed"] == 0  # a uniform input is balanced: one workgroup per entry
    assert res["span"] <= 1.03 * res["ideal"], res
    if cut == "equal":
        assert res["items"] == (230 + 22) * 6, res
