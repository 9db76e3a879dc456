"""The point plan's sort (csrc/binning.hip) on every route and at its capacity edges, at the level of its tables.

Every case of tests/plan_cases.py (small point sets, built to stand on a boundary; tests/test_plan_ref.py asserts without
a GPU that they do) builds its plan through nfft_hip_plan_points and checks the tables exactly against the numpy reference
of tests/plan_ref.py -- offsets, the points of every bin, bit-equal records, the column-group words -- for the plan at the
start of the buffer and for the owned plan behind it, then verifies the seal on the unchanged arrays.  Plans with a second
level also show which one ran: sort2_route_kernel leaves its decision in the first word of the cursors.  Cases under a
process switch (column-group order for small inputs, the owned plan for one column) run together in one child per
environment, since the switches are read once per process.

`fuse` false (more than 4 096 fine keys in a first-level bin) is not reached: only the sub-block plan of
NFFT_HIP_SPREAD=reg multiplies the keys, by 8 at m <= 5 and by 2 beyond, on the narrow tiling; 4 096 keys then need a grid
of more than 3 584 (6 144) cells per axis, whose (M / 16) x (M / 32) pencils are far more than the 8 192 first-level bins a
two-level sort takes -- such a plan is sorted by the single level.

Seal cases then change the points behind the plan -- a mantissa bit of the first, the last (alone in its slice) and a
middle point, two adjacent entries of the batch vector, two whole points exchanged -- and expect "stale point plan"
from the status word every time, and a clean verification after the word is put back.  Six cases also run nfft_adjoint and
nfft_forward against the oracle at this file's gate for those operators, rel_l2 < 2e-5 (tests/test_gpu_plan_sort.py).
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import plan_cases
import plan_ref
from conftest import rel_l2

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = [n for n, c in plan_cases.CASES.items() if not c.env]
SWITCHED = sorted({c.env_key for c in plan_cases.CASES.values() if c.env})


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


class Built:
    """A case's plan on the device: the problem, the device arrays it was built from and the plan buffer."""

    def __init__(self, case):
        import torch
        from torch_nfft_amd import _lib
        self.lib, self._lib, self.case = _lib.load(), _lib, case
        self.pos_h, self.batch_h = case.make()
        self.n = self.pos_h.shape[0]
        self.prob = _lib.Problem(case.d, self.n, case.C, case.B, case.N, case.m)
        self.main, self.own = _lib.plan_layout(self.prob, 0)
        self.pos = torch.from_numpy(self.pos_h).cuda()
        self.batch = torch.from_numpy(self.batch_h).cuda() if self.batch_h is not None else None
        nbytes = self.lib.nfft_hip_plan_bytes(ctypes.byref(self.prob))
        assert nbytes > 0
        self.plan = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        self.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(self.lib.nfft_hip_plan_points(ctypes.byref(self.prob), _ptr(self.pos), _ptr(self.batch), _ptr(self.plan),
                                                 nbytes, self.stream))
        _lib.check_status()

    def verify(self):
        """nfft_hip_plan_verify on the arrays as they are now; raises through check_status when the seal does not match."""
        self._lib.check(self.lib.nfft_hip_plan_verify(ctypes.byref(self.prob), _ptr(self.pos), _ptr(self.batch), _ptr(self.plan),
                                                      self.stream))
        self._lib.check_status()

    def verify_stale(self, what):
        with pytest.raises(RuntimeError, match="stale point plan"):
            self.verify()
            pytest.fail("the seal missed " + what)
        self._lib.check_status()  # (the report cleared the flag)


def check_tables(b):
    """check_plan on the main plan and on the owned plan; the route word against the reference's first-level counts."""
    buf = b.plan.cpu().numpy()
    row = dict(case=b.case.name, n=b.n)
    for L in (b.main, b.own):
        if L is None:
            continue
        tables = plan_ref.cut_tables(L, buf)
        ref = plan_ref.check_plan(L, tables, b.pos_h, b.batch_h)
        f = plan_ref.facts(L, ref, b.n)
        if f["route"] is not None:
            assert tables["route"] == f["route"], (b.case.name, "second-level route", tables["route"], f["max_l1"])
        if b.n == 0:
            assert not tables["offsets"].any()
        if L is b.main:
            row.update(route=f["route"], scan=f["scan"], scan_items=f["scan_items"], l1="%d/%d" % (f["l1bins"], f["l1seg"]),
                       G=f["G"], max_l1=f["max_l1"], entries=f["entries"])
        else:
            row.update(owned_route=f["route"], owned_max_l1=f["max_l1"], owned_entries=f["entries"], touch=f["touch"],
                       wrapping=f["wrapping"])
    if b.case.borders:
        M = b.main.M
        row["floor_differs"] = int((plan_ref.cells(b.pos_h, M) != plan_ref.floor_cells(b.pos_h, M)).any(axis=1).sum())
    return row


def seal_sequence(b):
    """Changes behind the plan, each reported, each clean again once undone."""
    import torch
    n, d = b.n, b.case.d
    words = b.pos.view(torch.int32).view(-1)
    for i in (0, n - 1, n // 2):
        w = i * d + (i % d)
        old = words[w].clone()
        words[w] = old ^ (1 << (3 + i % 17))  # one mantissa bit
        b.verify_stale("a mantissa bit of point %d" % i)
        words[w] = old
        b.verify()
    i = int(np.flatnonzero(np.diff(b.batch_h))[0])
    pair = b.batch[i: i + 2].clone()
    assert int(pair[0]) != int(pair[1])
    b.batch[i: i + 2] = pair.flip(0)  # two adjacent entries swapped: same values, in range
    b.verify_stale("a swap in the batch vector")
    b.batch[i: i + 2] = pair
    b.verify()
    i, j = 1, n // 3
    rows = b.pos[[i, j]].clone()
    assert not torch.equal(rows[0], rows[1])
    b.pos[[i, j]] = rows.flip(0)  # the same multiset of points under other indices
    b.verify_stale("two points exchanged")
    b.pos[[i, j]] = rows
    b.verify()
    assert torch.equal(b.pos.cpu(), torch.from_numpy(b.pos_h))


def consumer(b):
    """nfft_adjoint and nfft_forward on the case's points against the oracle."""
    import torch
    import torch_nfft_amd as tn
    from oracle import nfft_ref
    c = b.case
    rng = np.random.default_rng(17)
    x = rng.standard_normal((b.n,) if c.C == 1 else (b.n, c.C)).astype(np.float32)
    y = tn.nfft_adjoint(torch.from_numpy(x).cuda(), b.pos, b.batch, bandwidth=c.N, cutoff=c.m)
    ya = nfft_ref.nfft_adjoint(x, b.pos_h, b.batch_h, N=c.N, m=c.m)
    e_adj = rel_l2(y.cpu().numpy(), ya)
    z = tn.nfft_forward(y, b.pos, b.batch, cutoff=c.m, real_output=True)
    za = nfft_ref.nfft_forward(ya, b.pos_h, b.batch_h, m=c.m, real_output=True)
    e_fwd = rel_l2(z.cpu().numpy(), za)
    print("consumer %s: adjoint %.2e forward %.2e" % (c.name, e_adj, e_fwd))
    assert e_adj < 2e-5 and e_fwd < 2e-5, (c.name, e_adj, e_fwd)
    return dict(adjoint=e_adj, forward=e_fwd)


def run_case(name):
    b = Built(plan_cases.CASES[name])
    row = check_tables(b)
    b.verify()
    if b.case.seal:
        seal_sequence(b)
    if b.case.consumer:
        row.update(consumer(b))
    print("PLAN-ROW " + json.dumps(row))
    return row


def run_environment(key):
    """(child process) every case of one environment."""
    for name, c in plan_cases.CASES.items():
        if c.env_key == key:
            run_case(name)
            print("CASE-OK " + name)


@pytest.mark.parametrize("name", DEFAULT)
def test_plan_case(name):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    run_case(name)


@pytest.mark.parametrize("key", SWITCHED)
def test_plan_cases_under_switch(key):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_plan_edges as t; t.run_environment(%r)" % (
        ROOT, os.path.join(ROOT, "tests"), key)
    env = dict(os.environ, **dict(kv.split("=") for kv in key.split()))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    print(out.stdout[-6000:])
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    done = {l.split()[1] for l in out.stdout.splitlines() if l.startswith("CASE-OK ")}
    assert done == {n for n, c in plan_cases.CASES.items() if c.env_key == key}
