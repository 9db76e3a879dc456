"""GPU tests of the Buckingham / Born-Mayer-Huggins + Coulomb step with per-type-pair parameters: the pair
walk of csrc/ewald_bmh_table.hip on its own, unmasked and masked, on the points of section 7t's tests and on the counted cells
of tests/test_gpu_pair_frame_lists.py, then nfft_ewald_bmh_table_step as a whole, with a DispersionSplitting and with
dispersion=None, against the float64 restatement (tests/bmh_table_ref.py) on the same float32 positions and the float32-rounded
table.

Points.  Without a list lj_step_ref.lj_points (700, a jittered lattice with the edge cases of the wrap and exact duplicates),
with one lj_excl_ref.bonded_points (600, or 300 + 0 + 300, and the 4 000-point layout over 3 x 3 x 3 cells), types drawn on
top; exp-6 tables (bmh_table_ref.exp6_parameters: r_m between 0.7 and 1.0 d_min, alpha between 12 and 14, a C8 term).  Every
pair that keeps any short-range term is at least d_min apart, each of the three table energies is at least 1e-3 of their sum
of magnitudes and |U_sr| at least 0.1 of it, asserted per point set by the restatement.  For the whole call every position is
moved by (+3, -2, +1) lattice vectors, which rounds it to float32 once more; the restatement takes the moved values.

Tolerances.  Each gate is 4 x the largest relative error of the first device run against the float64 restatement, written
beside it, and none may exceed 1e-4 (the condition of section 7r); rel_l2 for F, rel_fro for W, the relative error for U.
"""
import math

import numpy as np
import pytest
import torch

import bmh_table_ref as bt
import dispersion_virial_ref as dv
import ewald_box_ref as eb
import lj_excl_ref as le
import lj_step_ref as lj
import lj_table_ref as lt
from conftest import rel_l2
from ewald_virial_ref import rel_fro
from test_bmh_table_ref import LARGEST_TABLE_GATE
from test_gpu_pair_frame_lists import _check, _lists, pf, pl

pytestmark = pytest.mark.gpu

CEILING = 1e-4
# (the largest first-run figure in brackets)
NEAR_TOL = {  # the unmasked walk against brute force: forty cases of 700 points
    "F": 2.2e-6,     # (5.289e-7: T at (30, 0.12), one set, T = 1; 2.0e-7 .. 4.9e-7 on the others)
    # (1.345e-5: the unit cube, one set, every T -- the charges are the same for all four, and their +- q_i q_j w cancel to a
    # small remainder: the figure of tests/test_gpu_lj_table.py on the same points, to the digit; 3.3e-8 .. 5.8e-6 on the others)
    "U_C": 5.4e-5,
    "U_sr": 1.5e-6,  # (3.573e-7: T at (12, 0.3), ragged, T = 2; 1.0e-10 .. 2.0e-7 on the others)
    "W": 3.4e-6,     # (8.272e-7: T at (12, 0.3), one set, T = 2; 2.3e-8 .. 6.8e-7 on the others)
}
MASKED_TOL = {  # the masked walk against brute force: six cases of 600 points, the one of 4 000 and the walk with c = 0
    "F": 1.6e-6,     # (3.946e-7: 4 000 points, T = 32; 1.5e-7 .. 2.2e-7 at 600)
    "U_C": 2.6e-6,   # (6.369e-7: 4 000 points; 2.0e-8 .. 5.5e-7 at 600)
    "U_sr": 5.2e-7,  # (1.278e-7: 4 000 points; 6.2e-9 .. 8.2e-8 at 600)
    "W": 1.0e-6,     # (2.470e-7: O, ragged; 8.3e-8 .. 2.1e-7 on the others)
}
WHOLE_TOL = {  # nfft_ewald_bmh_table_step (cutoff = 4) against the restatement: with and without a list, both inputs, dispersion=None
    "F": 2.3e-6,     # (5.533e-7: T, ragged, with a list; 3.6e-7 .. 5.5e-7 on the others)
    "U_C": 4.8e-5,   # (1.198e-5: the unit cube, one set, without a list -- the pair walk's remainder above; 7.9e-7 .. 4.9e-6)
    "U_sr": 2.5e-6,  # (6.168e-7: the unit cube, ragged, with a list; 2.2e-8 .. 5.3e-7 on the others)
    "W": 3.2e-6,     # (7.877e-7: T, ragged, with a list, fractional input; 3.0e-7 .. 7.9e-7 on the others)
}
CELLS_TOL = {  # the walks on the counted cells: every group of points, class of the list and live set on its own
    "F": 4.0e-6,     # (9.758e-7: the ends of `wrap`, boxO in O, unmasked -- the float32 image through a face; 6.7e-7 on row2 of ragged3)
    "U_C": 2.8e-5,   # (6.757e-6: set 2 of ragged3 in T, masked -- the cancelling sum of tests/test_gpu_pair_frame_lists.py, to the digit)
    "U_sr": 1.6e-6,  # (3.782e-7: boxO in O, masked; 3.0e-7 .. 3.8e-7 on the others)
    "W": 1.7e-6,     # (4.003e-7: boxO in O, unmasked; 2.2e-7 .. 3.3e-7 on the others)
}
# The untouched walk of section 7t on the points and types of the five one-set cases at T = 5, with a Lorentz-Berthelot table,
# stood at F 3.0e-7 .. 4.7e-7 in the same run and this walk at 0.96 .. 1.21 times that: the exponential adds nothing to see.
_ALL = (NEAR_TOL, MASKED_TOL, WHOLE_TOL, CELLS_TOL)
assert max(max(t.values()) for t in _ALL) <= CEILING
# the four wrong formulas of tests/test_bmh_table_ref.py are off by 1e3 x this: no gate on F, U_sr or W may be larger
assert max(t[k] for t in _ALL for k in ("F", "U_sr", "W")) <= LARGEST_TABLE_GATE
STEP_U_TOL = 5.5e-5  # WHOLE_TOL["U"] of tests/test_gpu_ewald_step.py: nfft_ewald_step's U against the float64 algorithm

BOXES = {"T": eb.T, "O": eb.O, "S": eb.S, "I": np.eye(3)}
# box, alpha_C, r_c, the cells: NEAR_SPLITS of tests/test_gpu_lj_table.py, restated; alpha_D = alpha_C + 1.5
NEAR_SPLITS = [("O", 14.0, 0.25, (4, 5, 3)), ("T", 12.0, 0.3, (3, 3, 3)), ("T", 30.0, 0.12, (7, 8, 7)),
               ("S", 16.0, 0.22, (3, 4, 4)), ("I", 12.0, 0.3, (3, 3, 3))]
TYPE_COUNTS = {1: (), 2: (), 5: (3,), 32: ()}  # T: the types left unused
SPLITS = {"I": (12.0, 13.0, 0.3, 32), "T": (12.0, 13.0, 0.3, 32), "O": (14.0, 15.0, 0.25, 48)}  # alpha_C, alpha_D, r_c, N
MOVE = np.array([3.0, -2.0, 1.0])
_CACHE = {}


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _six(A):
    return [A[0, 0], A[1, 0], A[1, 1], A[2, 0], A[2, 1], A[2, 2]]


def _relative(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / np.abs(want).max())


def _table(tn, tab, types):
    return tn.BMHPairTable(*(torch.from_numpy(np.ascontiguousarray(v)) for v in tab[:4]), _cuda(types), grid_c=torch.from_numpy(tab[4]))


def _no_grid(tab):
    """the same pair energies with nothing on the grid: the whole C6 / r^6 is truncated at r_c"""
    return tab[:4] + (np.zeros_like(tab[4]),)


def _lists_of(ex):
    return (None,) * 4 if ex is None else (ex.row_start, ex.col, ex.coulomb_weight, ex.dispersion_weight)


def _walk(tn, s, q, table, batch, A, ac, ad, r_c, ex=None, c=None):
    xs = torch.stack([_cuda(q), table.c if c is None else c], 1)
    return tn.ops.nfft_ewald_bmh_table_near(_cuda(s), xs, table.types, table.table, _cuda(batch), *_lists_of(ex), _six(A), ac, ad, r_c)


def _eight_errors(live, f, eight, fref, eref):
    f, eight = f.cpu().numpy().astype(np.float64), eight.cpu().numpy()
    assert np.isfinite(f).all() and np.isfinite(eight).all()
    assert np.linalg.norm(fref) > 0 and all(eref[b, :2].all() and np.linalg.norm(eref[b, 2:]) > 0 for b in live)
    return {"F": rel_l2(f, fref), "U_C": _relative(eight[live, 0], eref[live, 0]), "U_sr": _relative(eight[live, 1], eref[live, 1]),
            "W": rel_fro(eight[live, 2:], eref[live, 2:])}


def _whole_errors(live, got, ref):
    g = [t.cpu().numpy().astype(np.float64) for t in got]
    return {"F": rel_l2(g[0], ref[0]), "U_C": _relative(g[1][live], ref[1][live]), "U_sr": _relative(g[2][live], ref[2][live]),
            "W": rel_fro(g[3][live], ref[3][live])}


def _show(e):
    return " ".join("%s %.3e" % kv for kv in sorted(e.items()))


def _gate(e, tol, label):
    for key, err in e.items():
        assert err <= tol[key], (label, key, err, tol[key])


# ---- the unmasked walk ---------------------------------------------------------------------------------------------------

def _free_points(k, ragged):
    """the 700 points of split k, their charges and set vector; the types and tables are drawn per type count"""
    if ("free", k, ragged) not in _CACHE:
        rng = np.random.default_rng(300 + 10 * k + ragged)
        s = lj.lj_points(rng, 700)
        q = rng.standard_normal(700).astype(np.float32)
        _CACHE[("free", k, ragged)] = (s, q, dv.ragged_batch(700) if ragged else None)
    return _CACHE[("free", k, ragged)]


@pytest.mark.parametrize("T", list(TYPE_COUNTS))
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("k", range(len(NEAR_SPLITS)))
def test_unmasked_walk_against_brute_force(k, ragged, T):
    import torch_nfft_amd as tn
    name, alpha, r_c, cells = NEAR_SPLITS[k]
    A = BOXES[name]
    assert tn.EwaldSplitting(alpha, r_c, 4, box=A).cells == cells
    s, q, batch = _free_points(k, ragged)
    rng = np.random.default_rng(1000 * T + 10 * k + ragged)
    d_min = lj.D_MIN_FRACTIONAL * lt.box_stretch(A)
    types = lt.draw_types(rng, 700, T, TYPE_COUNTS[T])
    assert set(types) == set(range(T)) - set(TYPE_COUNTS[T])
    tab = bt.exp6_parameters(rng, T, d_min)
    bt.check_system(tab, types, s, A, batch, r_c, d_min * (1 - 1e-6))
    table = _table(tn, tab, types)
    args = (tn, s, q, table, batch, A, alpha, alpha + 1.5, r_c)
    f, eight = _walk(*args)
    f2, eight2 = _walk(*args)
    tn.ops.check_status()
    n, B = 700, 3 if ragged else 1
    live = [0, 2] if ragged else [0]
    assert f.shape == (n, 3) and f.dtype == torch.float32 and eight.shape == (B, 8) and eight.dtype == torch.float64
    assert torch.equal(f, f2) and torch.equal(eight, eight2)  # no atomics: the same bits
    fref, eref = bt.near_bmh_step(q, bt.to_float32(tab), types, s, A, batch, alpha, alpha + 1.5, r_c)
    e = _eight_errors(live, f, eight, fref, eref)
    fn = f.cpu().numpy().astype(np.float64)
    newton = np.abs(fn.sum(0)).max() / np.abs(fn).sum()
    print("bmh walk, box %s (%g, %g) ragged=%d T=%d: %s; |sum F| / sum |F| %.2e" % (name, alpha, r_c, ragged, T, _show(e), newton))
    if T == 5 and not ragged:
        # the untouched walk of section 7t on the same points and types with a Lorentz-Berthelot table: what the frame, the
        # image and the Ewald weights alone leave in F (printed, not gated: DESIGN.md section 7u compares the two)
        from test_gpu_lj_table import _rounded as lj_rounded, _table as lj_table, _walk as lj_walk
        ltab = lt.lorentz_berthelot(*lt.type_parameters(rng, T, d_min))
        lf, leight = lj_walk(tn, s, q, lj_table(tn, ltab, types), batch, A, alpha, alpha + 1.5, r_c)
        lref, _ = lt.near_table_step(q, lj_rounded(ltab), types, s, A, batch, alpha, alpha + 1.5, r_c)
        print("lj_table walk on the same points: F %.3e (bmh / lj %.2f)" % (rel_l2(lf.cpu().numpy().astype(np.float64), lref),
                                                                          e["F"] / rel_l2(lf.cpu().numpy().astype(np.float64), lref)))
    _gate(e, NEAR_TOL, "unmasked")
    assert newton <= 3e-5  # (the bound of tests/test_gpu_lj_step.py: a hundred float32 additions per point)
    if ragged:
        assert not bool(eight[1].any())  # the empty point set: exactly zero


# ---- the masked walk -----------------------------------------------------------------------------------------------------

class Bonded:
    """the points of bonded_points in the box `name`, one set of n or three sets of n / 2, 0 and n / 2, with T types on top:
    float32 Cartesian positions x moved by (+3, -2, +1) lattice vectors and the float32 fractional positions s that they
    convert to; the list, with one pair more at scales (1, 1); the float64 references, each computed once"""

    def __init__(self, name, ragged, n=600, G=7, seed=0, T=4):
        self.name, self.A, self.ragged = name, BOXES[name], ragged
        self.split = SPLITS[name]
        rng = np.random.default_rng(ord(name) + 7 * ragged + seed + 40)
        sizes = [n // 2, n // 2] if ragged else [n]
        parts = [le.bonded_points(rng, m, self.A, self.split[2], G=G) for m in sizes]
        offs = np.cumsum([0] + sizes)
        s0 = np.concatenate([p[0] for p in parts])
        self.pairs = np.concatenate([p[1] + o for p, o in zip(parts, offs)])
        self.sc, self.sl = np.concatenate([p[2] for p in parts]), np.concatenate([p[3] for p in parts])
        self.info = parts[0][4]
        self.n, self.B = int(offs[-1]), 3 if ragged else 1
        self.batch = np.concatenate([np.zeros(sizes[0], np.int64), np.full(sizes[1], 2, np.int64)]) if ragged else None
        self.live = [0, 2] if ragged else [0]
        inv = np.linalg.inv(self.A)
        self.x = ((s0.astype(np.float64) + MOVE) @ self.A).astype(np.float32)
        self.s = (self.x.astype(np.float64) @ inv).astype(np.float32)
        self.d_min = self.info["d_min"] * (1 - 1e-4)  # (the move rounds a position by up to 2.4e-7)
        self.q = rng.standard_normal(self.n).astype(np.float32)
        self.types = lt.draw_types(rng, self.n, T)
        self.tab = bt.exp6_parameters(rng, T, self.info["d_min"])
        bt.check_system(self.tab, self.types, self.s, self.A, self.batch, self.split[2], self.d_min, self.pairs, self.sl)
        # a pair at scales (1, 1): the first unlisted pair of neighbours found from the last point down
        r = le.check_separation(self.s[:sizes[0]], self.A, parts[0][1], parts[0][3], self.d_min)
        listed = set(map(tuple, np.sort(parts[0][1], 1)))
        i = sizes[0] - 2
        j = next(int(j) for j in np.argsort(r[i]) if j != i and r[i, j] > 0 and (min(i, j), max(i, j)) not in listed)
        assert r[i, j] < self.split[2]
        self.ones = np.array([[i, j]])
        self._ref = {}

    def lists(self, tn, with_ones=False):
        pairs, sc, sl = self.pairs, self.sc, self.sl
        if with_ones:
            pairs, sc, sl = np.concatenate([pairs, self.ones]), np.append(sc, 1.0), np.append(sl, 1.0)
        return tn.ExclusionList(pairs, self.n, coulomb_scale=sc, dispersion_scale=sl, batch=self.batch)

    def ref(self, what, tab=None):
        if what not in self._ref:
            ac, ad, r_c, N = self.split
            lists = (self.pairs, self.sc, self.sl)
            if what == "near":
                self._ref[what] = bt.near_bmh_step(self.q, bt.to_float32(self.tab), self.types, self.s, self.A, self.batch, ac, ad, r_c, *lists)
            elif what == "whole":
                self._ref[what] = bt.exact_bmh_table_step(self.q, bt.to_float32(self.tab), self.types, self.s, self.A, self.batch, ac,
                                                          ad, r_c, N, *lists)
            else:  # nothing on the grid
                self._ref[what] = bt.exact_bmh_table_step(self.q, bt.to_float32(_no_grid(self.tab)), self.types, self.s, self.A,
                                                          self.batch, ac, ad, r_c, N, *lists)
        return self._ref[what]


def _bonded(name, ragged):
    if ("bonded", name, ragged) not in _CACHE:
        _CACHE[("bonded", name, ragged)] = Bonded(name, ragged)
    return _CACHE[("bonded", name, ragged)]


def _check_masked(tn, w, label):
    ac, ad, r_c, _ = w.split
    table, ex = _table(tn, w.tab, w.types), w.lists(tn)
    args = (tn, w.s, w.q, table, w.batch, w.A, ac, ad, r_c)
    f, eight = _walk(*args, ex)
    f2, eight2 = _walk(*args, ex)
    tn.ops.check_status()
    assert f.shape == (w.n, 3) and f.dtype == torch.float32 and eight.shape == (w.B, 8) and eight.dtype == torch.float64
    assert torch.equal(f, f2) and torch.equal(eight, eight2)  # no atomics: the same bits
    e = _eight_errors(w.live, f, eight, *w.ref("near"))
    print("%s, box %s ragged=%d n=%d T=%d: %s" % (label, w.name, w.ragged, w.n, table.num_types, _show(e)))
    if w.ragged:
        assert not bool(eight[1].any())  # the empty point set: exactly zero
    _gate(e, MASKED_TOL, label)
    # a pair listed at scales (1, 1) is found and changes nothing: the bits of the list without it
    f1, eight1 = _walk(*args, w.lists(tn, with_ones=True))
    assert torch.equal(f1, f) and torch.equal(eight1, eight)
    # an empty list: the bits of the walk without one (which sees the bonded pairs in full, inside the turnover: finite)
    empty = tn.ExclusionList(np.zeros((0, 2), np.int64), w.n, batch=w.batch)
    f0, eight0 = _walk(*args)
    f1, eight1 = _walk(*args, empty)
    f3, eight3 = _walk(*args)
    tn.ops.check_status()
    assert bool(torch.isfinite(f0).all()) and torch.equal(f1, f0) and torch.equal(eight1, eight0)
    assert torch.equal(f3, f0) and torch.equal(eight3, eight0) and not torch.equal(f0, f)


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("name", ["I", "T", "O"])
def test_masked_walk_against_brute_force(name, ragged):
    """the masked walk against the float64 sum of the SCALED pair terms; an empty list gives the unmasked bits"""
    import torch_nfft_amd as tn
    _check_masked(tn, _bonded(name, ragged), "masked bmh walk")


def test_large_cells_and_a_second_tile():
    """about 4 000 points over 3 x 3 x 3 cells, 32 types: a cell holds more than the 128 points of a work item and a walked
    range more than the 256 of an LDS tile, so staged types and indices are read from a second tile"""
    import torch_nfft_amd as tn
    if "large" not in _CACHE:
        _CACHE["large"] = Bonded("I", False, n=4000, G=12, seed=5, T=32)
    w = _CACHE["large"]
    assert tn.EwaldSplitting(w.split[0], w.split[2], 32, box=np.eye(3)).cells == (3, 3, 3)
    s = w.s.astype(np.float64)
    cell = np.floor((s - np.rint(s) + 0.5) * 3).astype(np.int64).clip(0, 2)
    counts = np.bincount(cell[:, 0] + 3 * cell[:, 1] + 9 * cell[:, 2], minlength=27)
    assert counts.max() > 128 and counts.reshape(9, 3).sum(1).min() > 256
    _check_masked(tn, w, "masked bmh walk")


# ---- the counted cells of the frame ----------------------------------------------------------------------------------------

CELL_CASES = [("ragged3", "T", 32, (), False), ("ragged3", "T", 32, (), True), ("boxO", "O", 5, (3,), False),
              ("boxO", "O", 5, (3,), True)]  # layout, box, T, unused types, with the list


class Typed:
    """types and an exp-6 table on top of a Lists case of tests/test_gpu_pair_frame_lists.py: r_m between 0.7 and 1.0 of the
    layout's stated separation"""

    def __init__(self, layout, box, T, unused):
        self.c = c = _lists(layout, box)
        rng = np.random.default_rng(2000 * T + sum(map(ord, layout + box)))
        self.T = T
        self.types = lt.draw_types(rng, c.L.n, T, unused)
        assert set(self.types) == set(range(T)) - set(unused)
        self.d_min = pf.d_min_fractional(c.L.cells) * lt.box_stretch(c.Am)
        self.tab = bt.exp6_parameters(rng, T, self.d_min)
        self._ref = {}

    def ref(self, listed):
        if listed not in self._ref:
            c, L, q, tab = self.c, self.c.L, self.c.x[:, 0], bt.to_float32(self.tab)
            lists = (c.pairs, c.sc, c.sl) if listed else (np.zeros((0, 2), np.int64), np.zeros(0), np.zeros(0))
            self._ref[listed] = pl.per_set(lambda sel, lp, lsc, lsl: bt.near_bmh_step(
                q[sel], tab, self.types[sel], L.points[sel], c.Am, None, *c.split, *((lp, lsc, lsl) if listed else ())), L, *lists)
        return self._ref[listed]


def _typed(layout, box, T, unused):
    key = ("typed", layout, box, T)
    if key not in _CACHE:
        _CACHE[key] = Typed(layout, box, T, unused)
    return _CACHE[key]


@pytest.mark.parametrize("layout,box,T,unused,listed", CELL_CASES, ids=["%s-%s-T%d%s" % (c[0], c[1], c[2], "-listed" if c[4] else "")
                                                                        for c in CELL_CASES])
def test_walk_on_counted_cells(layout, box, T, unused, listed):
    """both instantiations on cells of exactly 0, 1, 63 .. 300 points with the list of pair_frame_lists_ref laid over them,
    against near_bmh_step per point set: every group of points, every class of the list and every live set on its own"""
    import torch_nfft_amd as tn
    w = _typed(layout, box, T, unused)
    c, L = w.c, w.c.L
    sp = tn.EwaldSplitting(c.alpha_c, c.r_c, 4) if c.A is None else tn.EwaldSplitting(c.alpha_c, c.r_c, 4, box=c.A)
    assert sp.cells == L.cells
    if T == 32:  # a half wave of a crowded cell's item mixes many rows of the table in LDS
        _, order, start = pf._sorted(L.points, L.batch, L.cells)
        k = int(np.argmax(start[1:] - start[:-1]))
        assert start[k + 1] - start[k] >= 300
        mixed = [len(set(w.types[order[t:t + 32]])) for t in range(int(start[k]), int(start[k + 1]) - 31, 32)]
        assert min(mixed) >= 16, mixed
    table = _table(tn, w.tab, w.types)
    run = lambda ex: _walk(tn, L.points, c.x[:, 0], table, L.batch, c.Am, *c.split, ex)
    ex = c.exclusions(tn) if listed else None
    f, eight = run(ex)
    f2, eight2 = run(ex)
    tn.ops.check_status()
    assert torch.equal(f, f2) and torch.equal(eight, eight2)
    # (_check prints every figure, then holds them against the gates of section 7t's walk on the same cells; ours follow)
    figures = _check(c, "table_masked" if listed else "table_near", f, eight, *w.ref(listed))
    for (what, where), err in figures.items():
        key = "U_sr" if what == "U_LJ" else what
        assert err <= CELLS_TOL[key], (what, where, err)
    if listed:
        ones = c.classes["s(1,1)"]
        f1, eight1 = run(c.exclusions(tn, c.without(ones)))
        tn.ops.check_status()
        assert torch.equal(f, f1) and torch.equal(eight, eight1)


# ---- the whole call ------------------------------------------------------------------------------------------------------

def _splittings(tn, name, A):
    ac, ad, r_c, N = SPLITS[name]
    box = None if name == "I" else A
    return tn.EwaldSplitting(ac, r_c, N, box=box), tn.DispersionSplitting(ad, r_c, N, box=box)


def _check_whole(tn, name, ragged, n, B, live, q, x, s, batch, table, ex, ref, label, dispersion=True):
    spc, spd = _splittings(tn, name, BOXES[name])
    spd = spd if dispersion else None
    qd, xd, sd, bd = (_cuda(v) for v in (q, x, s, batch))
    cart = tn.nfft_ewald_bmh_table_step(qd, table, xd, bd, coulomb=spc, dispersion=spd, exclusions=ex, cutoff=4)
    runs = [("Cartesian", cart)]
    if name != "I":
        runs.append(("fractional", tn.nfft_ewald_bmh_table_step(qd, table, sd, bd, coulomb=spc, dispersion=spd, exclusions=ex,
                                                                fractional=True)))
    tn.ops.check_status()
    F, UC, USR, W = cart
    assert F.shape == (n, 3) and UC.shape == (B,) and USR.shape == (B,) and W.shape == (B, 3, 3)
    assert F.dtype == UC.dtype == USR.dtype == W.dtype == torch.float32 and torch.equal(W, W.transpose(1, 2))
    for t in cart:
        assert not t.requires_grad and bool(torch.isfinite(t).all())
    for what, got in runs:
        e = _whole_errors(live, got, ref)
        print("nfft_ewald_bmh_table_step %s, box %s ragged=%d, %s input vs float64: %s" % (label, name, ragged, what, _show(e)))
        _gate(e, WHOLE_TOL, label)
        if ragged:
            assert not bool(got[1][1]) and not bool(got[2][1]) and not bool(got[3][1].any())  # the empty set
    Fn = F.cpu().numpy().astype(np.float64)
    assert np.abs(Fn.sum(0)).max() <= WHOLE_TOL["F"] * math.sqrt(n) * np.linalg.norm(Fn)
    return cart


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("name", ["I", "T", "O"])
def test_whole_call_with_a_list(name, ragged):
    """the unit cube (box=None), a triclinic and an orthorhombic box, Cartesian and fractional positions moved by (+3, -2, +1)
    lattice vectors, against the float64 restatement"""
    import torch_nfft_amd as tn
    w = _bonded(name, ragged)
    _check_whole(tn, name, ragged, w.n, w.B, w.live, w.q, w.x, w.s, w.batch, _table(tn, w.tab, w.types), w.lists(tn),
                 w.ref("whole"), "with a list")


class Free:
    """700 points of lj_points in the box `name` with five types (one unused), moved by (+3, -2, +1) lattice vectors"""

    def __init__(self, name, ragged):
        self.name, self.A, self.ragged = name, BOXES[name], ragged
        rng = np.random.default_rng(500 + ord(name) + ragged)
        s0 = lj.lj_points(rng, 700)
        self.n, self.B = 700, 3 if ragged else 1
        self.batch = dv.ragged_batch(700) if ragged else None
        self.live = [0, 2] if ragged else [0]
        self.x = ((s0.astype(np.float64) + MOVE) @ self.A).astype(np.float32)
        self.s = (self.x.astype(np.float64) @ np.linalg.inv(self.A)).astype(np.float32)
        d_min = lj.D_MIN_FRACTIONAL * lt.box_stretch(self.A)
        self.q = rng.standard_normal(700).astype(np.float32)
        self.types = lt.draw_types(rng, 700, 5, (3,))
        self.tab = bt.exp6_parameters(rng, 5, d_min)
        # the move rounds a position by up to 2.4e-7 and a duplicate like its original: the duplicated pairs stay at r = 0,
        # which every sum skips, and everything else d_min apart
        bt.check_system(self.tab, self.types, self.s, self.A, self.batch, SPLITS[name][2], d_min * (1 - 1e-4))
        self._ref = {}

    def ref(self, grid):
        if grid not in self._ref:
            ac, ad, r_c, N = SPLITS[self.name]
            tab = self.tab if grid else _no_grid(self.tab)
            self._ref[grid] = bt.exact_bmh_table_step(self.q, bt.to_float32(tab), self.types, self.s, self.A, self.batch, ac, ad, r_c, N)
        return self._ref[grid]


def _free(name, ragged):
    if ("whole", name, ragged) not in _CACHE:
        _CACHE[("whole", name, ragged)] = Free(name, ragged)
    return _CACHE[("whole", name, ragged)]


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("name", ["I", "T", "O"])
def test_whole_call_without_a_list(name, ragged):
    import torch_nfft_amd as tn
    w = _free(name, ragged)
    _check_whole(tn, name, ragged, w.n, w.B, w.live, w.q, w.x, w.s, w.batch, _table(tn, w.tab, w.types), None, w.ref(True),
                 "without a list")


# ---- dispersion=None -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("listed", [False, True])
@pytest.mark.parametrize("name,ragged", [("T", False), ("O", True)])
def test_nothing_on_the_grid(name, ragged, listed):
    """dispersion=None with grid_c = 0: against the float64 restatement with g = 0 (whose dispersion sums vanish), against the
    same call with a DispersionSplitting within the sum of the two sides' gates, and its U_coulomb against nfft_ewald_step's U
    within the sum of theirs"""
    import torch_nfft_amd as tn
    w = _bonded(name, ragged) if listed else _free(name, ragged)
    table = _table(tn, _no_grid(w.tab), w.types)
    assert table.has_grid is False and not bool(table.c.any())
    ex = w.lists(tn) if listed else None
    ref = w.ref("bare") if listed else w.ref(False)
    label = "dispersion=None%s" % (", with a list" if listed else "")
    got = _check_whole(tn, name, ragged, w.n, w.B, w.live, w.q, w.x, w.s, w.batch, table, ex, ref, label, dispersion=False)
    spc, spd = _splittings(tn, name, w.A)
    qd, xd, bd = _cuda(w.q), _cuda(w.x), _cuda(w.batch)
    want = tn.nfft_ewald_bmh_table_step(qd, table, xd, bd, coulomb=spc, dispersion=spd, exclusions=ex)
    tn.ops.check_status()
    e = _whole_errors(w.live, got, [t.cpu().numpy().astype(np.float64) for t in want])
    print("%s vs the call with a DispersionSplitting, box %s: %s" % (label, name, _show(e)))
    for key, err in e.items():
        assert err <= 2.0 * WHOLE_TOL[key], (key, err)
    _, _, U, _ = tn.nfft_ewald_step(qd, xd, bd, splitting=spc, exclusions=None if ex is None else tn.ExclusionList(
        w.pairs, w.n, coulomb_scale=w.sc, batch=w.batch))
    tn.ops.check_status()
    err = _relative(got[1].cpu().numpy()[w.live], U.cpu().numpy().astype(np.float64)[w.live])
    print("%s: U_coulomb vs nfft_ewald_step's U %.3e" % (label, err))
    assert err <= WHOLE_TOL["U_C"] + STEP_U_TOL


@pytest.mark.parametrize("listed", [False, True])
def test_zero_c_adds_exact_zeros(listed):
    """the walk of dispersion=None: with c = 0 the terms c_i c_j w_D and c_i c_j mg_D are exact zeros whatever alpha_D makes of
    w_D and mg_D, and whether the zeros come as +0 or as an arbitrary finite buffer times a zero grid coefficient"""
    import torch_nfft_amd as tn
    w = _bonded("T", False)
    ac, _, r_c, _ = w.split
    table = _table(tn, _no_grid(w.tab), w.types)
    ex = w.lists(tn) if listed else None
    args = (tn, w.s, w.q, table, None, w.A, ac)
    base = _walk(*args, ac, r_c, ex)
    g = torch.Generator(device="cuda").manual_seed(5)
    arbitrary = 1e3 * torch.randn(w.n, device="cuda", generator=g) * table.grid_c.float()[table.types.long()]
    assert bool(torch.isfinite(arbitrary).all()) and not bool(arbitrary.any()) and bool(torch.signbit(arbitrary).any())
    for ad, c in ((ac + 1.5, None), (0.5 * ac, None), (ac, arbitrary), (ac + 1.5, arbitrary)):
        got = _walk(*args, ad, r_c, ex, c=c)
        tn.ops.check_status()
        assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1])
    if listed:  # (without the list the bonded pairs stand inside the turnover: finite, and no reference to measure against)
        fref, eref = bt.near_bmh_step(w.q, bt.to_float32(_no_grid(w.tab)), w.types, w.s, w.A, None, ac, ac, r_c, w.pairs, w.sc, w.sl)
        e = _eight_errors([0], *base, fref, eref)
        print("the walk with c = 0, with a list: %s" % _show(e))
        _gate(e, MASKED_TOL, "c = 0")


# ---- types in device memory, no points, refusals ---------------------------------------------------------------------------

@pytest.mark.parametrize("listed", [False, True])
def test_a_type_changed_in_device_memory_is_clamped(listed):
    """table.types is checked once, at construction; a value written into it afterwards is clamped into [0, T) by the kernel,
    for the lane's own point and for a streamed one: the result is that of the clamped type, bit for bit, and nothing is read
    outside the table (T = 32 and T = 5: the last row of the second plane in LDS, and far beyond it)"""
    import torch_nfft_amd as tn
    w = _bonded("T", False)
    ac, ad, r_c, _ = w.split
    ex = w.lists(tn) if listed else None
    for T in (5, 32):
        rng = np.random.default_rng(T)
        types = lt.draw_types(rng, w.n, T)
        tab = bt.exp6_parameters(rng, T, w.info["d_min"])
        spoiled, clamped = _table(tn, tab, types), _table(tn, tab, types)
        at = torch.tensor([5, 77, 300, 301], device="cuda")
        spoiled.types[at] = torch.tensor([T, 2 ** 31 - 1, -1, -2 ** 31], dtype=torch.int32, device="cuda")
        clamped.types[at] = torch.tensor([T - 1, T - 1, 0, 0], dtype=torch.int32, device="cuda")
        assert not torch.equal(_cuda(types).int(), clamped.types)
        got = _walk(tn, w.s, w.q, spoiled, None, w.A, ac, ad, r_c, ex)
        want = _walk(tn, w.s, w.q, clamped, None, w.A, ac, ad, r_c, ex)
        tn.ops.check_status()
        assert bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[1]).all())
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        spc, spd = _splittings(tn, "T", w.A)
        whole = tn.nfft_ewald_bmh_table_step(_cuda(w.q), spoiled, _cuda(w.x), coulomb=spc, dispersion=spd, exclusions=ex)
        tn.ops.check_status()
        assert all(bool(torch.isfinite(t).all()) for t in whole)


def test_no_points_and_refused_inputs():
    import torch_nfft_amd as tn
    one = torch.ones(2, 2, dtype=torch.float64)
    none = (None,) * 4
    empty = tn.BMHPairTable(one, one, one, one, torch.zeros(0, dtype=torch.int64, device="cuda"))
    bare = tn.BMHPairTable(one, one, one, one, torch.zeros(0, dtype=torch.int64, device="cuda"), grid_c=torch.zeros(2))
    ex0 = tn.ExclusionList(np.zeros((0, 2), np.int64), 0)
    pos, xs = torch.zeros(0, 3, device="cuda"), torch.zeros(0, 2, device="cuda")
    walk = (_six(eb.T), 12.0, 13.0, 0.3)
    for lists in (none, _lists_of(ex0)):
        f, eight = tn.ops.nfft_ewald_bmh_table_near(pos, xs, empty.types, empty.table, None, *lists, *walk)
        assert f.shape == (0, 3) and eight.shape == (1, 8) and eight.dtype == torch.float64 and not bool(eight.any())
    tn.ops.check_status()
    tab = tn.BMHPairTable(one, one, one, one, torch.tensor([0, 1, 1, 0], device="cuda"))
    four, x4, ex4 = torch.zeros(4, 3, device="cuda"), torch.zeros(4, 2, device="cuda"), tn.ExclusionList([[0, 1]], 4)
    lists = _lists_of(ex4)
    op = tn.ops.nfft_ewald_bmh_table_near
    for bad in (dict(xs=torch.zeros(4, 3, device="cuda")),                    # (q, c) per point, nothing else
                dict(types=tab.types.long()), dict(types=tab.types[:3]),      # int32, one per point
                dict(table=tab.table[:, :, :2]), dict(table=tab.table.double()), dict(table=tab.table[:1]),
                dict(table=torch.zeros(33, 33, 4, device="cuda")),            # more types than the LDS table holds
                dict(table=tab.table.cpu()), dict(types=tab.types.cpu()),
                dict(lists=lists[:1] + (None,) * 3), dict(lists=(None,) + lists[1:]),  # all four list tensors or none
                dict(lists=(ex0.row_start,) + lists[1:]), dict(lists=lists[:3] + (lists[3][:1],)),
                dict(walk=(_six(eb.T), 12.0, 13.0, 0.31)),                    # r_cut above a third of the smallest width
                dict(walk=(_six(eb.T), 12.0, float("nan"), 0.3))):
        a = dict(xs=x4, types=tab.types, table=tab.table, lists=lists, walk=walk)
        a.update(bad)
        with pytest.raises(RuntimeError, match="Input mismatch"):
            op(four, a["xs"], a["types"], a["table"], None, *a["lists"], *a["walk"])
    # a table that starts in the middle of a larger tensor, 8 bytes off a 16-byte boundary: the operator moves it
    wide = torch.zeros(2 * 2 * 4 + 2, device="cuda")
    wide[2:] = tab.table.reshape(-1)
    shifted = wide[2:].view(2, 2, 4)
    assert shifted.data_ptr() % 16 == 8
    x4 = torch.tensor([[0.0, 0.0, 0.0], [0.1, 0.0, 0.0], [0.0, 0.1, 0.0], [0.1, 0.1, 0.1]], device="cuda")
    q4 = torch.tensor([[1.0, 1.0], [-1.0, 1.0], [1.0, 1.0], [-1.0, 1.0]], device="cuda")
    got, want = op(x4, q4, tab.types, shifted, None, *none, *walk), op(x4, q4, tab.types, tab.table, None, *none, *walk)
    tn.ops.check_status()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and bool(want[0].any())
    e = torch.zeros(0, device="cuda")
    spc, spd = tn.EwaldSplitting(12.0, 0.3, 32, box=eb.T), tn.DispersionSplitting(13.0, 0.3, 32, box=eb.T)
    for ex in (None, ex0):
        for t, d in ((empty, spd), (bare, None)):
            F, UC, USR, W = tn.nfft_ewald_bmh_table_step(e, t, pos, coulomb=spc, dispersion=d, exclusions=ex)
            assert F.shape == (0, 3) and UC.shape == (1,) and not bool(UC.any()) and not bool(USR.any()) and not bool(W.any())
    with pytest.raises(ValueError, match="nfft_ewald_bmh_table_step: table lives on cpu"):
        tn.nfft_ewald_bmh_table_step(torch.zeros(4, device="cuda"), tn.BMHPairTable(one, one, one, one, torch.tensor([0, 1, 1, 0])),
                                     four, coulomb=spc, dispersion=spd)
