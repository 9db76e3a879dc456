"""GPU tests of the kernels that carry the VALUES -- spreading and the value gather -- at stage level, at every window width,
tiling and route.

nfft_hip_plan_points, nfft_hip_spread and nfft_hip_interpolate through ctypes: no FFT runs, so nothing on the FFT side can
hide a point-side error.  Every kernel family runs at every width it instantiates:

  leg            kernels                                            shape, real planes           process environment
  narrow-*       spread_kernel<DIM, W>, interp_kernel<DIM, W, false>   1-D, 2-D, narrow 3-D; Cr = 2   default
                 DIM 1..3, m 1..8
  scatter        spread_mfma_kernel<W, ., false, false>                wide, Cr = 1                   default
  scatter-cols   the same kernel behind gather_rows                    wide, Cr = 3                   NFFT_HIP_OWNED=0
  owned-pair     spread_mfma_kernel<W, ., true, true>                  wide, Cr = 2 and Cr = 3 (the   default
                                                                       last column swept alone)
  owned-single   spread_mfma_kernel<W, ., true, false>                 wide, Cr = 1                   NFFT_HIP_OWNED=1
  ring           interp_mfma_kernel<W, .>                              wide, Cr = 2                   default
  cols           interp_cols_kernel<W, .>                              wide, Cr = 5 (a group of 8     default
                                                                       waves, partly idle)
  stream3        interp_stream_kernel<W, ., 3>                         wide, Cr = 2                   NFFT_HIP_STREAM_MIN=1
  stream1        interp_stream_kernel<W, ., 1>                         wide, Cr = 2                   ... NFFT_HIP_COLGROUPS=0
  lanes-wide     interp_kernel<3, W, true>                             wide, Cr = 2                   NFFT_HIP_GATHER=lds
  reg            spread_reg_kernel<W>, m 1..7 (spread_reg_supported:   narrow 3-D, Cr = 2             NFFT_HIP_SPREAD=reg
                 m + 1 <= 8; m = 8: tests/test_route.py)          
  *-listed       the OVERFLOW = true form of the eight range kernels   as above                       the leg's + NFFT_HIP_WORK_LIST=1

(wide: m 1..7).  The shapes are the four of test_gpu_gather_widths.SHAPES, the smallest at which each tiling exists, with
its two unequal point sets and its placed points.  Every leg asserts the route it relies on through nfft_dbg_route
(_lib.route) before it launches, and every range kernel the form that does the work through nfft_dbg_work_list
(info[1]: 1 = the plan walks its list in the persistent launch, OVERFLOW = true).

Balanced and listed plans.  binning.hip calls a plan balanced only if no range of slabs of any pencil holds 1.5 x the
mean over ALL ranges of its point set.  The shape of the derivative file never is: the ragged last pencils of M = 128 hold
a fraction of a full pencil's points, and the second point set lives in six slabs.  Its plans are listed under the default
environment already, so the *-listed legs take those points as they are (NFFT_HIP_WORK_LIST=1 is set as well; info[1] = 1
is asserted either way).  For the per-entry form (OVERFLOW = false) the other range legs append filler points to both sets
until every (pencil, range of slabs) of the plan the kernel walks -- the halo tiling, or the owned tiling with an entry per
touched tile -- holds exactly as many entries: `balanced` below; info[1] = 0 is asserted.  The placed points stay; the
fillers are uniform inside their pencil and range (owned tilings: with the window inside the tile), about 4 000 to 8 000
points in all.  nfft_hip_interpolate passes no ticket buffer, so listed launches deal their list round robin (the ticket
path: tests/test_gpu_graded_items.py).

Extra groups of the owned legs: own2, points whose window [cell - m, cell + m + 1] crosses one border of the owned tiles
(32 x 64, pair form 32 x 32), and own4, both borders; the uniform draw gives at least 24 of each, and 8 are asserted.

Spreading legs, against oracle/nfft_ref_torch.spread in float64 on the device (pinned to oracle/nfft_ref at 1e-12 by
tests/test_ref_torch.py) on the same float32 inputs: the whole grid per plane; every group on its own -- one launch per
group with the coefficients of all other points set to zero (plan, work items and kernel unchanged) against the gridding of
the group's points only, relative L2 per plane against the plane's own norm (a plane the group has no point in must be
exactly 0); groups = the four classes col & 3, every placed category, own2 and own4.  The grid is pre-filled with NaN and
must be finite afterwards, every cell no window touches must be exactly 0, and owned and register-tile spreading give the
same bits twice.

Gather legs: a random float32 grid, not a transform's output, whose planes have the magnitudes 1, 1e-3, 1e3, ... (the
matrix-core gathers scale every plane by its own power of two), against test_pos_grad_ref.interp_f64 on that grid widened
to float64; per column over all compared points and over every group (test_gpu_gather_widths.check; rows are divided by
their plane's magnitude first, so that no point set's plane outweighs the other's); two calls give the same bits.  All
points are compared while n W^d <= 1.5e6 taps, else 400 random ones plus every placed point.

Bounds: tests/test_gpu_parity.py T1N (narrow tiling, register tiles) and T1W (matrix-core kernels and the wide lane
gather), for the whole output and for every group alike; nothing is restated.  Observed figures: profiles/r14_value_widths.md.

Legs with a non-default environment run in child processes (the switches are read once), one child per environment, one
after another, each running all its legs and widths and reporting a line per case as it ends, which the pytest case of
that (leg, m) waits for; a child that fails ends there and is not started again.  The leg table is
tests/value_width_legs.py.
"""
import ctypes
import json
import os
import queue
import subprocess
import sys
import tempfile
import threading

import numpy as np
import pytest
import torch

import test_pos_grad_ref as ref1
from oracle import nfft_ref_torch
from test_gpu_gather_widths import ALL_TAPS, B, SHAPES, SUBSET, cells_of, check, coord, groups_of, make_points, tiling
from test_gpu_parity import T1N, T1W
from value_width_legs import CASES, GEOMETRY, LEGS, POINT_SETS, env_key

pytestmark = pytest.mark.gpu

MAGNITUDES = (1.0, 1e-3, 1e3)  # of grid plane p: MAGNITUDES[p % 3]
TOLERANCE = {"T1N": T1N, "T1W": T1W}
assert POINT_SETS == B and all(SHAPES[g][:3] == dims for g, dims in GEOMETRY.items())  # (the CPU route test reads the shapes from the leg table)


# ---- points ------------------------------------------------------------------------------------------------------------

def owned_tiles(leg):
    """(T1, T2) of the owned tiling a leg spreads on (common.h tile_cfg), or None."""
    return {"owned-pair": (32, 32), "owned-single": (32, 64)}.get(leg.replace("-listed", ""))


def window_tiles(c, m, T, M):
    """Tiles of extent T (M % T == 0) that the windows [c - m, c + m + 1] of the cells c begin and end in."""
    return ((c - m) % M) // T, ((c + m + 1) % M) // T


def balanced(rng, pos, batch, cats, N, m, T1, T2, owned):
    """pos, batch, cats with filler points appended to every point set until each (pencil, range of slabs) of its plan
    holds the same number of plan entries: what binning.hip segment_split_kernel calls a balanced plan.  T1 x T2: the
    pencils' cross-section; owned: a point has an entry in every tile its window touches, and the fillers' windows stay
    inside their tile.  Returns the number of ranges per pencil as well (common.h seg_base_runs on 256 CUs, M = 128)."""
    M = 2 * N
    nt1, nt2 = -(-M // T1), -(-M // T2)
    runs = 1
    while runs < M // 32 and B * nt1 * nt2 * (runs + 1) <= 256:
        runs += 1
    seg = -(-M // runs)
    cells = cells_of(pos, M)
    new_pos, new_batch, first = [], [], {}
    for b in range(B):
        rows = np.flatnonzero(batch == b)
        c = cells[rows]
        count = np.zeros((nt1, nt2, runs), np.int64)
        if owned:
            a0, a1 = window_tiles(c[:, 1], m, T1, M)
            b0, b1 = window_tiles(c[:, 2], m, T2, M)
            for ja, jb in ((a0, b0), (a0, b1), (a1, b0), (a1, b1)):
                fresh = np.ones(len(rows), bool)  # (an entry per DISTINCT tile)
                if ja is a1:
                    fresh &= a1 != a0
                if jb is b1:
                    fresh &= b1 != b0
                np.add.at(count, (ja[fresh], jb[fresh], c[fresh, 0] // seg), 1)
        else:
            np.add.at(count, (c[:, 1] // T1, c[:, 2] // T2, c[:, 0] // seg), 1)
        fill = [pos[rows]]
        for j1, j2, r in np.ndindex(nt1, nt2, runs):
            k = int(count.max() - count[j1, j2, r])
            lo = [r * seg, j1 * T1 + (m if owned else 0), j2 * T2 + (m if owned else 0)]
            hi = [min(r * seg + seg, M), min(j1 * T1 + T1, M) - (m + 1 if owned else 0), min(j2 * T2 + T2, M) - (m + 1 if owned else 0)]
            cell = np.stack([rng.integers(lo[a], hi[a], k) for a in range(3)], axis=1)
            fill.append(coord(cell, rng.uniform(0.05, 0.95, (k, 3)), M).astype(np.float32))
        first[b] = sum(len(p) for p in new_pos)
        new_pos.append(np.concatenate(fill))
        new_batch.append(np.full(len(new_pos[-1]), b, np.int64))
    # (the rows of a point set keep their order in front of its fillers)
    start = {b: int(np.flatnonzero(batch == b)[0]) for b in range(B)}
    cats = {name: np.array([first[int(batch[r])] + r - start[int(batch[r])] for r in rows]) for name, rows in cats.items()}
    return np.concatenate(new_pos), np.concatenate(new_batch), cats, runs


def leg_points(leg, m):
    """The points of a leg at cutoff m: pos, batch, {category: rows}, the class col & 3 of every point, and the ranges per
    pencil of a plan that has to be balanced (else None)."""
    geometry, listed = LEGS[leg][2], LEGS[leg][6]
    d, N, n, wide, n1 = SHAPES[geometry]
    M = 2 * N
    rng = np.random.default_rng(7000 + 1000 * d + 100 * wide + m)
    pos, batch, cats, _ = make_points(rng, d, N, m, n, wide, n1)
    own = owned_tiles(leg)
    if own:
        T1o, T2o = own

        def crossing(both):
            c = cells_of(pos, M)
            a0, a1 = window_tiles(c[:, 1], m, T1o, M)
            b0, b1 = window_tiles(c[:, 2], m, T2o, M)
            return np.flatnonzero((((a0 != a1) & (b0 != b1)) if both else ((a0 != a1) ^ (b0 != b1))) & (batch == 0))

        # (the draw gives 386 ... 1 425 and 24 ... 644 of them at these seeds; run_case asserts at least 8 per group)
        cats["own2"], cats["own4"] = crossing(False), crossing(True)
    runs = None
    if listed == 0:
        _, T1, T2 = tiling(d, N, m, wide)
        T1, T2 = own if own else (T1, T2)
        pos, batch, cats, runs = balanced(rng, pos, batch, cats, N, m, T1, T2, bool(own))
    c2 = cells_of(pos[:, d - 1], M)
    T2 = tiling(d, N, m, wide)[2]
    return pos, batch, cats, (c2 - c2 // T2 * T2) & 3, runs


# ---- the stage calls -----------------------------------------------------------------------------------------------------

def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


class Stage:
    """A problem's plan and the two stage calls on it."""

    def __init__(self, d, N, m, Cr, pos, batch):
        from torch_nfft_amd import _lib
        self._lib, self.lib = _lib, _lib.load()
        self.d, self.N, self.M, self.m, self.Cr, self.n = d, N, 2 * N, m, Cr, len(pos)
        self.prob = _lib.Problem(d, self.n, Cr, B, N, m)
        self.route = _lib.route(self.prob, Cr)
        self.pos, self.batch = dev(pos), dev(batch)
        self.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.plan = torch.empty(self.lib.nfft_hip_plan_bytes(ctypes.byref(self.prob)), dtype=torch.uint8, device="cuda")
        _lib.check(self.lib.nfft_hip_plan_points(ctypes.byref(self.prob), ptr(self.pos), ptr(self.batch), ptr(self.plan),
                                                 self.plan.numel(), self.stream))
        self.scratch = torch.empty(self.lib.nfft_hip_spread_scratch_bytes(ctypes.byref(self.prob), Cr) // 4, device="cuda")

    def work_list(self, which):
        """info[8] of nfft_dbg_work_list: which = 0 the plan of the gather, 1 the plan the spreading kernel walks."""
        info, hdr, entries = np.zeros(8, np.int64), np.zeros((B, 2), np.int32), np.zeros((16, 4), np.int32)
        vp = ctypes.c_void_p
        self._lib.check(self.lib.nfft_dbg_work_list(ctypes.byref(self.prob), ptr(self.plan), which, vp(info.ctypes.data),
                                                    vp(hdr.ctypes.data), vp(entries.ctypes.data), 16, self.stream))
        return info

    def spread(self, x):
        """[B * Cr, M^d] float32 from x [n, Cr] (a device tensor); the grid is pre-filled with NaN."""
        grid = torch.full((B * self.Cr, self.M ** self.d), float("nan"), device="cuda")
        self._lib.check(self.lib.nfft_hip_spread(ctypes.byref(self.prob), ptr(self.plan), ptr(x), self.Cr, ptr(grid),
                                                 ptr(self.scratch), self.stream))
        return grid

    def gather(self, grid):
        yr = torch.full((self.n, self.Cr), float("nan"), device="cuda")
        self._lib.check(self.lib.nfft_hip_interpolate(ctypes.byref(self.prob), ptr(self.plan), ptr(grid), self.Cr, ptr(yr),
                                                      self.stream))
        return yr


def reference_grid(st, x, rows=None):
    """Float64 gridding [B * Cr, M^d] of the rows `rows` (default: all) of x [n, Cr] on the device."""
    pos, batch = (st.pos, st.batch) if rows is None else (st.pos[rows], st.batch[rows])
    x = x if rows is None else x[rows]
    g = nfft_ref_torch.spread(x.to(torch.float64), pos, batch, st.N, st.m).real  # [sets up to the last one, Cr, M..M]
    out = torch.zeros((B, x.shape[1], st.M ** st.d), dtype=torch.float64, device="cuda")
    out[:g.shape[0]] = g.reshape(g.shape[0], g.shape[1], -1)
    return out.reshape(B * x.shape[1], -1)


def plane_figure(got, want):
    """Largest relative L2 error of a plane against its own norm; inf for a plane that should be 0 and is not."""
    err = torch.linalg.vector_norm(got.to(torch.float64) - want, dim=1)
    norm = torch.linalg.vector_norm(want, dim=1)
    fig = torch.where(norm > 0, err / norm.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0))
    return float(fig.max())


def spread_leg(label, st, rng, groups, tol, deterministic):
    """The checks of a spreading leg on the plan st; returns {group: figure}."""
    x = dev(rng.standard_normal((st.n, st.Cr)).astype(np.float32))
    got = st.spread(x)
    assert bool(torch.isfinite(got).all()), "%s: a cell was not written" % label
    figures = {"all": plane_figure(got, reference_grid(st, x))}
    touched = reference_grid(st, torch.ones((st.n, 1), device="cuda")) > 0  # [B, cells]: the window weights are positive
    stray = got.reshape(B, st.Cr, -1)[(~touched)[:, None, :].expand(B, st.Cr, -1)]
    assert bool((stray == 0).all()), "%s: %d cells outside every window are not 0" % (label, int((stray != 0).sum()))
    if deterministic:
        assert torch.equal(got, st.spread(x)), "%s: two calls differ" % label
    for name, rows in groups.items():
        rows = torch.from_numpy(np.asarray(rows)).cuda()
        xg = torch.zeros_like(x)
        xg[rows] = x[rows]
        gg = st.spread(xg)
        assert bool(torch.isfinite(gg).all()), "%s %s: a cell was not written" % (label, name)
        figures[name] = plane_figure(gg, reference_grid(st, x, rows))
    st._lib.check_status()
    print("  %-9s tol %.1e  " % (label, tol) + "  ".join("%s %.2e" % kv for kv in figures.items()))
    bad = {k: f for k, f in figures.items() if not f < tol}
    assert not bad, (label, tol, bad)
    return figures


def gather_leg(label, st, rng, pos, batch, cats, align, tol):
    """The checks of a gather leg on the plan st; returns {column: {group: figure}} as check prints them."""
    W, n = 2 * st.m + 2, st.n
    if n * W ** st.d <= ALL_TAPS:
        sel = np.arange(n)
    else:
        sel = np.union1d(rng.choice(n, SUBSET, replace=False), np.concatenate(list(cats.values())))
    groups = groups_of(sel, cats, align)
    planes = B * st.Cr
    mag = np.array([MAGNITUDES[p % 3] for p in range(planes)])
    grid = (rng.standard_normal((planes, st.M ** st.d)) * mag[:, None]).astype(np.float32)
    gt = dev(grid)
    y = st.gather(gt)
    assert bool(torch.isfinite(y).all()), "%s: an output was not written" % label
    assert torch.equal(y, st.gather(gt)), "%s: two calls differ" % label
    st._lib.check_status()
    y = y.cpu().numpy()[sel]
    g64 = grid.astype(np.float64).reshape((B, st.Cr) + (st.M,) * st.d)
    want = np.zeros((len(sel), st.Cr))
    for b in range(B):
        of_set = batch[sel] == b
        want[of_set] = ref1.interp_f64(g64[b:b + 1], pos[sel][of_set], st.m, True)
    print("  %s: %d of %d points compared" % (label, len(sel), n))
    for c in range(st.Cr):
        scale = mag[batch[sel] * st.Cr + c]
        check("%s c%d" % (label, c), y[:, c] / scale, want[:, c] / scale, groups, tol)


def run_case(leg, m):
    """One (leg, cutoff) in this process, whose environment must be the leg's."""
    from torch_nfft_amd import _lib
    env, kind, geometry, crs, _, expect, listed, tol = LEGS[leg]
    tol = TOLERANCE[tol]
    for name in ("NFFT_HIP_OWNED", "NFFT_HIP_STREAM_MIN", "NFFT_HIP_COLGROUPS", "NFFT_HIP_GATHER", "NFFT_HIP_SPREAD",
                 "NFFT_HIP_WORK_LIST", "NFFT_HIP_SMALL_NARROW", "NFFT_HIP_GRADE"):
        assert os.environ.get(name) == env.get(name), "the leg %s runs in its own environment (%s)" % (leg, name)
    d, N, _, wide, _ = SHAPES[geometry]
    pos, batch, cats, align, runs = leg_points(leg, m)
    print("%s m = %d: %s, tile (TC, T1, T2) = %s, %d points" % (leg, m, geometry, tiling(d, N, m, wide), len(pos)))
    rng = np.random.default_rng(100 * m + len(leg))
    for Cr in crs:
        st = Stage(d, N, m, Cr, pos, batch)
        got = {k: getattr(st.route, k) for k in expect}
        assert got == expect, (leg, m, Cr, st.route)
        if listed is not None:
            info = st.work_list(1 if kind == "spread" else 0)
            # Not a statement about values: `balanced` restates when binning.hip segment_split_kernel calls a plan balanced
            # (no range of slabs with 1.5 x the mean of its point set or 1.5 x seg_target_points; `runs` ranges per pencil
            # by common.h seg_base_runs on 256 CUs; an entry per touched tile in the owned tilings).  If these two fail in
            # every per-entry leg at once, that rule has changed and `balanced` has to follow it.
            assert int(info[1]) == listed, (leg, m, "the plan is %s" % ("listed" if info[1] else "balanced"), info.tolist())
            assert runs is None or int(info[7]) == runs, (runs, info.tolist())
        if kind in ("spread", "both"):
            groups = {"align%d" % a: np.flatnonzero(align == a) for a in range(4)}
            groups.update(cats)
            assert all(len(rows) >= 8 for rows in groups.values()), {k: len(v) for k, v in groups.items()}
            spread_leg("spread Cr%d" % Cr, st, rng, groups, tol, st.route.owned or st.route.spread == "reg")
        if kind in ("gather", "both"):
            gather_leg("gather Cr%d" % Cr, st, rng, pos, batch, cats, align, tol)


# ---- children ----------------------------------------------------------------------------------------------------------------

def child_main(key):
    """Runs every case of the environment `key` (which the parent has set), in the order of CASES, and reports one line
    per case as it ends.  A failed comparison is reported and the child goes on; anything else ends it."""
    import contextlib
    import io
    for leg, m in CASES:
        if env_key(LEGS[leg][0]) != key:
            continue
        out, error = io.StringIO(), None
        with contextlib.redirect_stdout(out):
            try:
                run_case(leg, m)
            except AssertionError as e:
                error = str(e)[:2000]
        print("CASE " + json.dumps({"leg": leg, "m": m, "error": error, "output": out.getvalue()}), flush=True)
    print("DONE", flush=True)


class Child:
    """The child process of one environment.  Its reports are read as they arrive, so a pytest case waits for its own case
    only (the first one of a child for the child's start as well); CASES keeps a child's cases together and in the child's
    order, so a child has ended when the next one starts."""
    CASE_SECONDS = 120

    def __init__(self, key, env):
        tests = os.path.dirname(os.path.abspath(__file__))
        code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_value_widths as t; t.child_main(%r)" % (
            os.path.dirname(tests), tests, key)
        self.key, self.cases, self.failure, self.lines = key, {}, None, queue.Queue()
        self.err = tempfile.TemporaryFile(mode="w+")
        self.proc = subprocess.Popen([sys.executable, "-c", code], env=dict(os.environ, **env), stdout=subprocess.PIPE,
                                     stderr=self.err, text=True)
        threading.Thread(target=self._read, daemon=True).start()

    def _read(self):
        for line in self.proc.stdout:
            self.lines.put(line)
        self.lines.put(None)

    def _fail(self, what, tail=""):
        self.proc.kill()
        self.proc.wait()
        self.err.seek(0)
        self.failure = "child [%s] %s\n%s\n%s" % (self.key, what, tail, self.err.read()[-3000:])

    def report(self, leg, m):
        """The report of a case, or None with self.failure set; a failed child is not started again."""
        done = False
        while (leg, m) not in self.cases and self.failure is None:
            try:
                line = self.lines.get(timeout=self.CASE_SECONDS)
            except queue.Empty:
                self._fail("reported nothing for %d s" % self.CASE_SECONDS)
                break
            if line is None:
                rc = self.proc.wait()
                self._fail("ended with %s %s" % (rc, "after its last case" if done else "before its last case"))
            elif line.startswith("CASE "):
                c = json.loads(line[5:])
                self.cases[(c["leg"], c["m"])] = c
            elif line.startswith("DONE"):
                done = True
        return self.cases.get((leg, m))

    def close(self):
        if self.proc.poll() is None:
            self.proc.kill()
        self.proc.wait()
        self.err.close()


@pytest.fixture(scope="module")
def children():
    started = {}
    yield started
    for child in started.values():
        child.close()


@pytest.mark.parametrize("leg,m", CASES, ids=["%s-m%d" % c for c in CASES])
def test_value_width(children, leg, m):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    env = LEGS[leg][0]
    if not env:
        return run_case(leg, m)
    key = env_key(env)
    if key not in children:
        children[key] = Child(key, env)
    case = children[key].report(leg, m)
    if case is None:
        pytest.fail(children[key].failure)
    print(case["output"])
    assert case["error"] is None, case["error"]
