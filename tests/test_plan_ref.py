"""Without a GPU: does the plan checker of tests/plan_ref.py bite, and do the cases of tests/plan_cases.py stand where they
claim to stand?

The first half builds a correct plan on the CPU from the reference, for a scatter plan in column-group order, an owned
plan and a 2-D plan, and asserts that check_plan accepts it and rejects every mutant.  The second half asserts, for every
case that tests/test_gpu_plan_edges.py runs, the class it claims -- from the layout entry nfft_dbg_plan_layout (host code
only, like nfft_dbg_route in tests/test_route.py) and the reference counts alone -- and that the long-standing cases of
tests/test_gpu_plan_sort.py reach none of the capacity boundaries.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import plan_cases
import plan_ref
from plan_ref import PlanError, build_tables, cells, check_plan, floor_cells
from torch_nfft_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENVIRONMENTS = sorted({c.env_key for c in plan_cases.CASES.values()})


def layouts(case, n):
    return _lib.plan_layout(_lib.Problem(case.d, n, case.C, case.B, case.N, case.m), 0)


# ---- cells() against split_cell, restated step by step in float32 --------------------------------------------------------
def split_cell_f32(pos32, M):
    """csrc/common.h split_cell with numpy float32 operations: the fast path for power-of-two M, else the general path with
    the fma residual (formed exactly in float64: the product has at most 45 significant bits)."""
    f = np.float32
    pos32 = np.asarray(pos32, dtype=f)
    hi = pos32 * f(M)
    flp = np.floor(hi)
    frp = hi - flp
    fast = (M & (M - 1)) == 0
    lo = (pos32.astype(np.float64) * M - hi.astype(np.float64)).astype(f)
    fl = flp.copy()
    fr = (hi - fl) + lo
    neg = fr < 0
    fr = np.where(neg, fr + f(1), fr).astype(f)
    fl = np.where(neg, fl - 1, fl)
    big = fr >= 1
    fl = np.where(big, fl + 1, fl)
    cell = np.mod(fl.astype(np.int64), M)
    if fast:
        cell = np.where(frp < 1, np.mod(flp.astype(np.int64), M), cell)
    return cell


@pytest.mark.parametrize("M", [16, 64, 128, 144, 192, 768, 2048, 32512])
def test_cells_restates_split_cell(M):
    rng = np.random.default_rng(M)
    v = np.concatenate([plan_cases.border_values(M, [1] if M <= 2048 else [256]), plan_cases.uniform(rng, 20000, 1).ravel(),
                        -(np.float32(2.0) ** -np.arange(20, 60, dtype=np.float32))])
    assert np.array_equal(cells(v, M), split_cell_f32(v, M))
    differ = cells(v, M) != floor_cells(v, M)
    assert differ.any()  # just below a border the float64 floor and split_cell part ways
    assert cells(np.float32([-2.0 ** -40]), M)[0] == 0 and floor_cells(np.float32([-2.0 ** -40]), M)[0] == M - 1
    assert cells(np.float32([-0.0, 0.0, -0.5, 0.5]), M).tolist() == [0, 0, M // 2, M // 2]


# ---- the checker ---------------------------------------------------------------------------------------------------------
def _mutant_inputs(kind):
    """(layout, pos, batch) of a small plan of each kind, with -0.0 and a coordinate just below zero among the points."""
    rng = np.random.default_rng(5)
    if kind == "scatter":
        # the 64^3 grid on the matrix-core tiling; column-group order is a property of the layout record, so the
        # record of a sparse problem with CG = 3 stands for a plan in that order
        n, d = 31000, 3
        L = _lib.plan_layout(_lib.Problem(3, n, 1, 2, 32, 4), 0)[0]._replace(CG=3, grouped=True)
        assert L.wide and not L.owned
    elif kind == "owned":
        n, d = 6000, 3
        L = _lib.plan_layout(_lib.Problem(3, n, 2, 2, 64, 4), 0)[1]
        assert L is not None and L.owned and L.pair
    else:
        n, d = 3000, 2
        L = _lib.plan_layout(_lib.Problem(2, n, 1, 2, 64, 4), 0)[0]
        assert L.one_level
    pos = plan_cases.uniform(rng, n, d)
    pos[7, d - 1] = np.float32(-0.0)
    # cell 0 by split_cell, cell M - 1 by a float64 floor.  (Owned plans: along axis 0 -- in the tiled axes the windows of
    # both cells touch the same two tiles across the seam, and the tables cannot tell them apart.)
    pos[11, 0 if kind == "owned" else d - 1] = np.float32(-2.0 ** -40)
    if kind == "owned":
        pos[13, 1:] = plan_cases.coord([31, 31], L.M, 0.5)  # a window on a corner: four tiles
    batch = plan_cases.sorted_batch(rng, n, 2)
    return L, pos, batch


def _copy(t):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in t.items()}


def _swap(t, a, b):
    t["index"][[a, b]] = t["index"][[b, a]]
    t["coords"][[a, b]] = t["coords"][[b, a]]


def _drop(t, slot, bin_):
    for k in ("index", "coords"):
        t[k] = np.concatenate([t[k][:slot], t[k][slot + 1:], t[k][:1]])
    t["offsets"][bin_ + 1:] -= 1


def _insert(t, slot, bin_, index, coords):
    t["index"] = np.concatenate([t["index"][:slot], [index], t["index"][slot:]]).astype(np.int32)
    t["coords"] = np.concatenate([t["coords"][:slot], coords[None], t["coords"][slot:]])
    t["offsets"][bin_ + 1:] += 1


def _mutants(L, ref, good, pos):
    """[(name, tables)] of wrong plans."""
    out = []
    off = good["offsets"].astype(np.int64)
    full = np.flatnonzero(ref.counts >= 2)
    # two neighbouring occupied bins with different points at the border
    t0 = next(int(t) for t in full[:-1] if ref.counts[t + 1] >= 1 and good["index"][off[t + 1] - 1] != good["index"][off[t + 1]])
    m = _copy(good); _swap(m, off[t0 + 1] - 1, off[t0 + 1]); out.append(("swap across a bin border", m))
    m = _copy(good); m["offsets"][t0 + 1] += 1; out.append(("offset off by one", m))
    m = _copy(good); m["offsets"][-1] -= 1; out.append(("last offset off by one", m))
    s = int(off[t0])
    m = _copy(good); m["index"][s + 1] = m["index"][s]; m["coords"][s + 1] = m["coords"][s]
    out.append(("duplicated index, another missing", m))
    m = _copy(good); m["coords"][s] = pos[good["index"][s + 1]]; out.append(("coordinates of another index", m))
    s = int(np.flatnonzero(good["index"][:off[-1]] == 7)[0])
    assert np.signbit(good["coords"][s, -1]) and good["coords"][s, -1] == 0
    m = _copy(good); m["coords"][s, -1] = np.float32(0.0); out.append(("+0.0 for -0.0", m))
    if L.grouped:
        g = good["groups"].astype(np.int64)
        t1 = next(int(t) for t in range(L.ntiles) if off[t] < g[t, 0] < g[t, 1] < off[t + 1])
        m = _copy(good); _swap(m, g[t1, 0] - 1, g[t1, 0]); out.append(("swap across a group border", m))
        m = _copy(good); _swap(m, g[t1, 1] - 1, g[t1, 1]); out.append(("swap across the second group border", m))
        m = _copy(good); m["groups"][t1, 0] += 1; out.append(("group word off by one", m))
        m = _copy(good); m["groups"][t1, 1] -= 1; out.append(("second group word off by one", m))
    if L.owned:
        assert ref.touched[13] == 4
        slots = np.flatnonzero(good["index"][:off[-1]] == 13)
        assert slots.size == 4
        s = int(slots[2])
        bin_ = int(np.searchsorted(off, s, side="right") - 1)
        m = _copy(good); _drop(m, s, bin_); out.append(("owned entry missing from one of four tiles", m))
        other = next(t for t in range(L.ntiles) if t not in set(np.searchsorted(off, slots, side="right") - 1))
        m = _copy(good); _insert(m, int(off[other]), other, 13, pos[13]); out.append(("owned entry in a fifth tile", m))
    return out


@pytest.mark.parametrize("kind", ["scatter", "owned", "plane"])
def test_checker_rejects_every_mutant(kind):
    L, pos, batch = _mutant_inputs(kind)
    ref = plan_ref.plan_ref(L, pos, batch)
    good = build_tables(L, ref, pos)
    check_plan(L, good, pos, batch)
    # the same plan with the entries of every (bin, group) in another order is as good
    other = _copy(good)
    t = int(np.argmax(ref.counts))
    lo = int(good["groups"][t, 1]) if L.grouped else int(ref.offsets[t])
    hi = int(ref.offsets[t + 1])
    assert hi - lo >= 2
    other["index"][lo:hi] = good["index"][lo:hi][::-1]
    other["coords"][lo:hi] = good["coords"][lo:hi][::-1]
    check_plan(L, other, pos, batch)
    mutants = _mutants(L, ref, good, pos)
    # a border point filed under floor(double) instead of split_cell's cell
    assert (cells(pos, L.M) != floor_cells(pos, L.M)).sum() == 1
    wrong = plan_ref.plan_ref(L, pos, batch, cell_fn=floor_cells)
    mutants.append(("border point filed under floor(double)", build_tables(L, wrong, pos)))
    assert len(mutants) >= 7
    for name, tables in mutants:
        with pytest.raises(PlanError):
            check_plan(L, tables, pos, batch)
            pytest.fail("accepted: " + name)


# ---- the cases -----------------------------------------------------------------------------------------------------------
def case_facts(key):
    """{case: facts} of the cases whose process environment is `key`, JSON-ready."""
    out = {}
    for name, c in plan_cases.CASES.items():
        if c.env_key != key:
            continue
        pos, batch = c.make()
        n = pos.shape[0]
        main, own = layouts(c, n)
        f = plan_ref.facts(main, plan_ref.plan_ref(main, pos, batch), n)
        f["l1_sizes"] = sorted(f["l1_sizes"])
        f["has_owned"] = own is not None
        f["pair"] = bool(own.pair) if own else False
        if own is not None:
            fo = plan_ref.facts(own, plan_ref.plan_ref(own, pos, batch), n)
            f.update(touch=fo["touch"], wrapping=fo["wrapping"], owned_entries=fo["entries"], owned_cap=own.cap,
                     owned_route=fo["route"], owned_max_l1=fo["max_l1"])
        f["floor_differs"] = int((cells(pos, main.M) != floor_cells(pos, main.M)).any(axis=1).sum()) if n else 0
        out[name] = f
    return out


def assert_claims(name, claims, f):
    for k, want in claims.items():
        if k == "l1_has":
            assert want <= set(f["l1_sizes"]), (name, k, want)
        elif k == "touch_min":
            assert all(g >= w for g, w in zip(f["touch"], want)), (name, k, f["touch"])
        elif k == "wrapping_min":
            assert f["wrapping"] >= want, (name, k, f["wrapping"])
        else:
            assert f[k] == want, (name, k, f[k], want)


@pytest.mark.parametrize("key", ENVIRONMENTS, ids=[k or "default" for k in ENVIRONMENTS])
def test_cases_reach_their_edges(key):
    if key:  # the switches are read once per process: one child evaluates all the cases of its environment
        code = ("import json, sys; sys.path[:0] = [%r, %r]; import test_plan_ref as t; "
                "print('FACTS ' + json.dumps(t.case_facts(%r)))") % (ROOT, os.path.join(ROOT, "tests"), key)
        env = dict(os.environ, **dict(kv.split("=") for kv in key.split()))
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-3000:]
        facts = json.loads([l for l in out.stdout.splitlines() if l.startswith("FACTS ")][0][6:])
        for f in facts.values():
            f["touch"] = tuple(f["touch"])
    else:
        facts = case_facts(key)
    assert facts
    for name, f in facts.items():
        c = plan_cases.CASES[name]
        assert_claims(name, c.claims, f)
        if c.borders:
            assert f["floor_differs"] > 0, name
        if c.seal:
            assert c.B >= 2 and f["last_slice"] in (0, 1), name


def test_case_table_covers_every_class():
    """Across the default-environment cases: every G of the in-kernel scan, every scan kind, both block sizes."""
    facts = case_facts("")
    assert {f["G"] for f in facts.values() if f["G"]} == {64, 32, 16, 8, 4, 2, 1}
    assert {f["scan"] for f in facts.values()} == {"none", "small4", "small16", "hipcub"}
    assert {f["block_points"] for f in facts.values()} == {1024, 2048}
    assert {f["l1bins"] for f in facts.values() if f["wide"]} >= {128, 64, 32, 16}
    assert {f["route"] for f in facts.values()} == {None, 0, 1}
    assert {f["two_level"] for f in facts.values()} == {False, True}


def test_committed_cases_stand_on_no_capacity_boundary():
    """The shapes tests/test_gpu_plan_sort.py has had all along: no scan threshold, no LDS limit, no slice of one point or
    one short of full, an average first-level bin far from the one-pass capacity, and only some G of the in-kernel scan."""
    gs = set()
    for d, N, n, B in plan_cases.COMMITTED:
        L = _lib.plan_layout(_lib.Problem(d, n, 1, B, N, 4), 0)[0]
        assert L.two_level
        assert L.scan_items not in (4096, 4097, 16384, 16385, 65536, 65537)
        assert L.npencils not in (8176, 8177)
        assert n % L.block_points not in (0, 1, L.block_points - 1)
        mean = n / L.npencils
        assert not 0.9 * plan_ref.FUSE_CAP < mean < 1.1 * plan_ref.FUSE_CAP
        if L.local_scan:
            gs.add(plan_ref.local_scan_threads(L.npencils))
    assert gs and gs < {64, 32, 16, 8, 4, 2, 1} and len(gs) <= 2
