"""GPU tests of the exclusion and type-table pair walks at the edges of the pair kernels' frame (csrc/pair_frame.h, DESIGN.md
sections 7d, 7s, 7t and 7v): the masked product walk, lj_excl_list_kernel and both table walks of step_near_kernel on the
counted layouts of tests/pair_frame_ref.py -- cells of exactly 0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257 and 300 points,
the same behind an empty point set -- with an exclusion list laid over them by tests/pair_frame_lists_ref.py, whose classes
put a listed pair where the list's own state can go wrong: the partner staged in the second or third LDS tile (its caller
index and type kept as integer bits there), both ends in second-wave lanes, an end in the partly idle last item of a cut
cell, the set behind the empty one (caller indices past the first set's size), through every face, rows of 1 .. 33 entries
with hits on the first, last and middle entry and misses after a full search, scale pairs with exactly one zero, and for
the list kernel a second trip of its strided loop.  tests/test_pair_frame_lists_ref.py asserts on the CPU that the lists reach
all of this, that the older fixtures do not, and that un-listing any class changes the float64 reference visibly.

Every op is compared with the float64 restatement of the same sum on the same float32 fractional positions: F by rel_l2 over
all points, over the four groups of tests/test_gpu_pair_frame_edges.py and over the ends of every class of the list, each
meeting the gate on its own; U_C and U_LJ by their relative error and W by rel_fro, per live point set.

Gates.  Each is 4 x the largest figure of the first device run of these cases, written beside it with where it stood; none
may exceed CEILING = 1e-4 (section 7r).  A figure above that, or a group or class more than a factor 3 from its op's other
groups, would have been a bug to find, not a number to record.  Beside each gate: the older gate of the same op and quantity
and whether every case here keeps it.
"""
import math

import numpy as np
import pytest
import torch

import ewald_box_ref as eb
import lj_excl_ref as le
import lj_table_ref as lt
import pair_frame_lists_ref as pl
import pair_frame_ref as pf
from conftest import rel_l2
from ewald_virial_ref import rel_fro
from test_gpu_lj_excl import WHOLE_TOL as EXCL_WHOLE_TOL
from test_gpu_lj_step import _coefficients
from test_gpu_lj_table import _rounded, _table
from test_gpu_lj_table import _walk as _table_walk
from test_gpu_pair_frame_edges import BOXES, SPLIT, WHOLE, _cuda, _groups, _six

pytestmark = pytest.mark.gpu

CEILING = 1e-4
# (op, quantity): 4 x the largest figure of the first device run over the op's cases, the groups of points, the classes of the
# list and the live point sets.  In brackets: that figure and where it stood, the range of the cases' figures (for F over all
# points), then the older gates of the same op and quantity and whether every case here keeps them.
GATES = {
    # (8.990e-07: the ends of `wrap`, boxO in O; 3.8e-7 .. 4.1e-7 over all points.  NEAR_TOL of test_gpu_lj_excl 1.6e-6 and
    # lj_step_near of test_gpu_pair_frame_edges 1.8e-6: kept by every figure)
    ("excl_near", "F"): 3.6e-6,
    # (6.757e-06: set 2 of ragged3 in T, where U_C = -18.5 is what is left of 41 338 of |q_i q_j w| -- 4.5e-4 of them, against
    # 2.1e-2 in set 0; 8.1e-8 .. 7.1e-7 on the others.  NEAR_TOL 2.1e-6: kept but for that set; lj_step_near 2.7e-5: kept)
    ("excl_near", "U_C"): 2.7e-5,
    ("excl_near", "U_LJ"): 1.9e-6,  # (4.700e-07: grid3 in the cube; 3.5e-7 .. 4.7e-7.  NEAR_TOL 2.3e-6, lj_step_near 2.0e-6: kept)
    ("excl_near", "W"): 1.8e-7,     # (4.404e-08: set 2 of ragged3 in T; 2.8e-8 .. 4.4e-8.  NEAR_TOL 1.1e-6, lj_step_near 4.1e-7: kept)
    # (4.729e-07: the 24 ends of `face`, ragged3 in T; 3.427e-07 on the 9 points of row8, grid3 in T; 4.7e-8 .. 1.0e-7 over all
    # points.  LIST_TOL of test_gpu_lj_excl 3.7e-7: kept over all points and by every group and class but `face`)
    ("excl_list", "F"): 1.9e-6,
    # (7.598e-08: set 0 of ragged3 in T, where U_C is 1.8 % of the sum of its terms' magnitudes; 2.1e-9 .. 4.3e-8 on the
    # others.  LIST_TOL 2.3e-8: kept by grid3, not by boxO and ragged3 -- a list of bonds has no such cancellation)
    ("excl_list", "U_C"): 3.0e-7,
    ("excl_list", "U_LJ"): 3.3e-8,  # (8.316e-09: set 0 of ragged3 in T; 8.6e-10 .. 3.6e-9 on the others.  LIST_TOL 6.3e-9: kept but for that set)
    ("excl_list", "W"): 6.0e-7,     # (1.508e-07: grid3 in T; 4.9e-8 .. 8.6e-8 on the others.  LIST_TOL 3.8e-7: kept)
    ("table_near", "F"): 4.0e-6,    # (9.973e-07: the ends of `wrap`, boxO in O; 3.8e-7 .. 4.0e-7 over all points.  NEAR_TOL of test_gpu_lj_table 2.0e-6: kept)
    ("table_near", "U_C"): 1.9e-5,  # (4.727e-06: set 2 of ragged3 in T, the cancelling sum above; 8.8e-8 .. 2.5e-7 on the others.  NEAR_TOL 5.4e-5: kept)
    ("table_near", "U_LJ"): 1.3e-6,  # (3.166e-07: grid3 in the cube; 1.5e-7 .. 2.2e-7 on the others.  NEAR_TOL 1.3e-6: kept)
    ("table_near", "W"): 2.0e-6,    # (5.076e-07: boxO in O; 1.8e-7 .. 2.7e-7 on the others.  NEAR_TOL 4.4e-6: kept)
    ("table_masked", "F"): 3.8e-6,  # (9.561e-07: the ends of `wrap`, boxO in O; 3.7e-7 .. 4.0e-7 over all points.  MASKED_TOL of test_gpu_lj_table 1.6e-6: kept)
    ("table_masked", "U_C"): 2.7e-5,  # (6.757e-06: set 2 of ragged3 in T -- the charges and scales of excl_near, the same sum; 1.1e-7, 1.8e-7 on the others.  MASKED_TOL 2.6e-6: kept but for that set)
    ("table_masked", "U_LJ"): 9.0e-7,  # (2.259e-07: boxO in O; 2.1e-7 .. 2.2e-7 in ragged3.  MASKED_TOL 6.3e-7: kept)
    ("table_masked", "W"): 1.7e-6,  # (4.155e-07: boxO in O; 1.8e-7 .. 2.9e-7 in ragged3.  MASKED_TOL 6.5e-7: kept)
    # the radial sweep of the list kernel: F per point against the pair's own magnitude, the sums per subset of the pairs
    # (6.333e-07: dispersion alone at r = 0.255, a pair through a face -- T_D falls like r^-8 there, eight times the image's
    # error; 1.7e-7 with both species, 2.3e-7 Coulomb alone; 6.9e-8 at r = 1e-4, 1.8e-7 beyond r_c.  LIST_TOL 3.7e-7 is a
    # rel_l2 over a whole list, not a figure per pair)
    ("sweep", "F"): 2.5e-6,
    ("sweep", "U_C"): 1.4e-9,   # (3.576e-10: the pairs above alpha_D's switch; 7.4e-11 below it.  LIST_TOL 2.3e-8: kept)
    ("sweep", "U_LJ"): 2.8e-8,  # (6.927e-09: the pairs above alpha_D's switch; 2.2e-10 below it.  LIST_TOL 6.3e-9: kept below the switch and over all pairs, 1.6e-9)
    ("sweep", "W"): 2.1e-7,     # (5.222e-08: Coulomb alone, the pairs above the switch; 1.7e-8 .. 5.2e-8.  LIST_TOL 3.8e-7: kept)
    # nfft_ewald_lj_excl_step on ragged3 in T, the same rule; WHOLE_TOL of test_gpu_lj_excl beside each: all four kept
    ("whole", "F"): 2.8e-6,     # (7.063e-07: the 4 points of `duplicate`; 6.236e-07 `moved`; 3.794e-07 over all points, 3.4e-7 .. 4.4e-7 in the groups; 2.6e-6)
    ("whole", "U_C"): 4.5e-6,   # (1.121e-06; 1.9e-5)
    ("whole", "U_LJ"): 1.6e-6,  # (3.965e-07; 3.8e-6)
    ("whole", "W"): 1.0e-6,     # (2.521e-07; 2.6e-6)
}
# Spread.  Over the groups of points and the classes with fifty ends or more, no figure for F stood further than a factor
# 1.5 from the op's figure over all points in the three walks (0.75 .. 1.50), nor than a factor 2.3 in the list kernel
# (0.43 .. 1.97).  The classes that stood highest are those whose image goes through a face: `wrap` and `face`, up to 2.6 x
# in the walks on 25 points and 4.7 x in the list kernel on 24.  That is the float32 image, not the list: t - s of two reduced
# coordinates of opposite sign is rounded at 6e-8 before rint takes the box off, so d carries 4.0e-7 (rms, restated in float32
# on the CPU from these positions) where a pair inside the box carries 3e-8 .. 7e-8, and the list kernel's force is a single
# term T d.  The only other class beyond a factor 3 is row8 of the list kernel in T (4.3 x on 9 points), and three of its
# eight pairs go through a face too; the rows of 7 and 9 beside it stand at 0.7 x and 0.5 x.  In the whole call, where the far
# field's error is added to every point alike, the classes stand between 0.5 x (row2) and 1.9 x (`duplicate`) of all points.
assert max(GATES.values()) <= CEILING

EXCL_CASES = [("grid3", "cube"), ("grid3", "T"), ("boxO", "O"), ("ragged3", "T")]
TABLE_CASES = [("grid3", "cube", 32, (), False), ("boxO", "O", 5, (3,), False), ("ragged3", "T", 32, (), False),
               ("ragged3", "T", 32, (), True), ("boxO", "O", 2, (), True)]  # layout, box, T, unused types, with the list
_CACHE = {}


class Lists:
    """a layout in a box with its split, the coefficients (q, c, a) of tests/test_gpu_lj_step.py on the layout's lattice, the
    list of pair_frame_lists_ref.listed_pairs and the float64 references, each computed once and left unchanged"""

    def __init__(self, layout, box):
        self.layout, self.box, self.L, self.A = layout, box, pf.layout(layout), BOXES[box]
        self.Am = np.eye(3) if self.A is None else self.A
        self.alpha_c, self.r_c = SPLIT["coulomb"][layout]
        self.alpha_d = self.alpha_c + 1.5
        self.split = (self.alpha_c, self.alpha_d, self.r_c)
        rng = np.random.default_rng(sum(map(ord, "lists" + layout + box)))
        L = self.L
        self.x = np.stack(_coefficients(rng, L.n, self.Am, spacing=pf.cartesian_spacing(L.cells, self.A)), 1)
        self.pairs, self.sc, self.sl, self.classes = pl.listed_pairs(L, self.A, self.r_c, rng)
        self.live = sorted(L.counts)
        self.tag = "%s in %s" % (layout, box)
        self._ref = {}

    def without(self, which):
        keep = np.ones(len(self.pairs), bool)
        keep[which] = False
        return self.pairs[keep], self.sc[keep], self.sl[keep]

    def exclusions(self, tn, lists=None, device="cuda"):
        pairs, sc, sl = (self.pairs, self.sc, self.sl) if lists is None else lists
        return tn.ExclusionList(pairs, self.L.n, coulomb_scale=sc, dispersion_scale=sl, batch=self.L.batch, device=device)

    def ref(self, what):
        if what not in self._ref:
            L, q, c, a = self.L, *self.x.T
            if what == "near":
                self._ref[what] = pl.per_set(lambda sel, lp, lsc, lsl: le.near_step_scaled(
                    q[sel], c[sel], a[sel], L.points[sel], self.Am, None, lp, lsc, lsl, *self.split), L, self.pairs, self.sc, self.sl)
            elif what == "list":
                self._ref[what] = le.list_step(q, c, L.points, self.Am, L.batch, self.pairs, self.sc, self.sl, *self.split)
            else:
                raise KeyError(what)
        return self._ref[what]


def _lists(layout, box):
    if (layout, box) not in _CACHE:
        _CACHE[(layout, box)] = Lists(layout, box)
    return _CACHE[(layout, box)]


def _assert_cells(tn, c):
    sp = tn.EwaldSplitting(c.alpha_c, c.r_c, 4) if c.A is None else tn.EwaldSplitting(c.alpha_c, c.r_c, 4, box=c.A)
    assert sp.cells == c.L.cells


def _excl_op(tn, c, op, ex):
    L = c.L
    return op(_cuda(L.points), _cuda(c.x), _cuda(L.batch), ex.row_start, ex.col, ex.coulomb_weight, ex.dispersion_weight,
              _six(c.A), c.alpha_c, c.alpha_d, c.r_c)


def _relative(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / np.abs(want).max())


def _check(c, op, f, eight, fref, eref, extra_groups=None, skip=()):
    """shapes, finiteness, the empty set, and every figure against GATES[(op, .)]: F overall, per group of points and over
    the ends of every class of the list (those in `skip` left out: their reference force is zero); U_C, U_LJ, W per live set.
    Prints every figure; returns them."""
    L = c.L
    assert f.shape == (L.n, 3) and f.dtype == torch.float32 and eight.shape == (L.B, 8) and eight.dtype == torch.float64
    f, eight = f.cpu().numpy().astype(np.float64), eight.cpu().numpy()
    assert np.isfinite(f).all() and np.isfinite(eight).all()
    if L.B == 3:
        assert not eight[1].any()  # the empty point set: exact zeros
    groups = dict(_groups(L))
    groups.update(extra_groups or {})
    figures = {("F", "all"): rel_l2(f, fref)}
    for name, rows in groups.items():
        assert rows.any() and np.linalg.norm(fref[rows]) > 0, name
        figures[("F", name)] = rel_l2(f[rows], fref[rows])
    for name, which in c.classes.items():
        if name in skip or which.size == 0:
            continue
        e = pl.ends(c.pairs, which)
        assert np.linalg.norm(fref[e]) > 0, name
        figures[("F", name)] = rel_l2(f[e], fref[e])
    for b in c.live:
        assert eref[b, :2].all() and np.linalg.norm(eref[b, 2:]) > 0
        figures[("U_C", "set %d" % b)] = _relative(eight[b, :1], eref[b, :1])
        figures[("U_LJ", "set %d" % b)] = _relative(eight[b, 1:2], eref[b, 1:2])
        figures[("W", "set %d" % b)] = rel_fro(eight[b, 2:], eref[b, 2:])
    for what in ("F", "U_C", "U_LJ", "W"):
        mine = {k[1]: v for k, v in figures.items() if k[0] == what}
        worst = max(mine, key=mine.get)
        low = min(v for v in mine.values())
        print("%s, %s: %s worst %.3e (%s), spread %.2f; %s" % (op, c.tag, what, mine[worst], worst, mine[worst] / max(low, 1e-300),
                                                              ", ".join("%s %.3e" % kv for kv in mine.items())))
    for (what, where), err in figures.items():
        assert err <= GATES[(op, what)], (op, c.tag, what, where, err, GATES[(op, what)])
    return figures


def _trips(c):
    """the points by the trip of the list kernel's strided loop that computes them, where a set is larger than one trip;
    the kernel's geometry recomputed from n, B and the constants 256 and 1024 of its header"""
    L = c.L
    blocks = max(1, min(math.ceil(math.ceil(L.n / L.B) / 256), 1024))
    assert blocks == pl.list_blocks(L.n, L.B)
    set_of = L.set_of()
    rank = np.arange(L.n) - np.searchsorted(set_of, set_of)
    sizes = [int((set_of == b).sum()) for b in c.live]
    if max(sizes) <= blocks * 256:
        return blocks, {}
    trips = {}
    for b in c.live:
        trips["set %d, first trip" % b] = (set_of == b) & (rank < blocks * 256)
        trips["set %d, second trip" % b] = (set_of == b) & (rank >= blocks * 256)
    return blocks, trips


# ---- the masked walk and the list kernel ---------------------------------------------------------------------------------

@pytest.mark.parametrize("layout,box", EXCL_CASES, ids=["%s-%s" % c for c in EXCL_CASES])
def test_masked_walk_on_counted_cells(layout, box):
    """nfft_ewald_lj_excl_near against lj_excl_ref.near_step_scaled; the pairs listed at (1, 1) leave the bits of the call
    without them"""
    import torch_nfft_amd as tn
    c = _lists(layout, box)
    _assert_cells(tn, c)
    ex = c.exclusions(tn)
    f, eight = _excl_op(tn, c, tn.ops.nfft_ewald_lj_excl_near, ex)
    f2, eight2 = _excl_op(tn, c, tn.ops.nfft_ewald_lj_excl_near, ex)
    tn.ops.check_status()
    assert torch.equal(f, f2) and torch.equal(eight, eight2)  # no atomics: the same bits
    _check(c, "excl_near", f, eight, *c.ref("near"))
    ones = c.classes["s(1,1)"]
    f1, eight1 = _excl_op(tn, c, tn.ops.nfft_ewald_lj_excl_near, c.exclusions(tn, c.without(ones)))
    tn.ops.check_status()
    e = _cuda(pl.ends(c.pairs, ones))
    assert torch.equal(f[e], f1[e]) and torch.equal(f, f1) and torch.equal(eight, eight1)


@pytest.mark.parametrize("layout,box", EXCL_CASES, ids=["%s-%s" % c for c in EXCL_CASES])
def test_list_kernel_on_counted_cells(layout, box):
    """nfft_ewald_lj_excl_list against lj_excl_ref.list_step.  On ragged3 a point set takes more than one workgroup and more
    than one trip of a workgroup's strided loop, and the per-set sums are made of several workgroups' partials."""
    import torch_nfft_amd as tn
    c = _lists(layout, box)
    _assert_cells(tn, c)
    L = c.L
    blocks, trips = _trips(c)
    if layout == "ragged3":
        n0, n2 = (int((L.set_of() == b).sum()) for b in c.live)
        assert math.ceil(math.ceil(L.n / L.B) / 256) > 1 and blocks > 1 and max(n0, n2) > blocks * 256 and trips
        set_of = L.set_of()
        for b in c.live:  # eight pairs in the second trip of each live set, and pairs across its boundary
            assert (set_of[c.pairs[c.classes["trip2"], 0]] == b).sum() >= 8 and (set_of[c.pairs[c.classes["straddle"], 0]] == b).sum() >= 4
    ex = c.exclusions(tn)
    f, eight = _excl_op(tn, c, tn.ops.nfft_ewald_lj_excl_list, ex)
    f2, eight2 = _excl_op(tn, c, tn.ops.nfft_ewald_lj_excl_list, ex)
    tn.ops.check_status()
    assert torch.equal(f, f2) and torch.equal(eight, eight2)
    _check(c, "excl_list", f, eight, *c.ref("list"), extra_groups=trips, skip=("duplicate", "s(1,1)"))
    rows = pl.row_lengths(c.pairs, L.n)
    assert not bool(f[_cuda(np.flatnonzero(rows == 0))].any())  # a point with an empty row: exactly zero
    twins = pl.ends(c.pairs, c.classes["duplicate"])
    assert (rows[twins] == 1).all() and not bool(f[_cuda(twins)].any())  # their rows hold each other only: no force at r = 0
    ones = c.classes["s(1,1)"]
    f1, eight1 = _excl_op(tn, c, tn.ops.nfft_ewald_lj_excl_list, c.exclusions(tn, c.without(ones)))
    tn.ops.check_status()
    e = _cuda(pl.ends(c.pairs, ones))
    assert torch.equal(f[e], f1[e]) and not bool(f[e].any()) and torch.equal(f, f1) and torch.equal(eight, eight1)


# ---- the table walk ------------------------------------------------------------------------------------------------------

class Typed:
    """types and a Lorentz-Berthelot table on top of a Lists case: sigma between 0.5 and 0.8 of the layout's stated separation"""

    def __init__(self, layout, box, T, unused):
        self.c = c = _lists(layout, box)
        rng = np.random.default_rng(1000 * T + sum(map(ord, layout + box)))
        self.T = T
        self.types = lt.draw_types(rng, c.L.n, T, unused)
        assert set(self.types) == set(range(T)) - set(unused)
        d_min = pf.d_min_fractional(c.L.cells) * lt.box_stretch(c.Am)
        self.tab = lt.lorentz_berthelot(*lt.type_parameters(rng, T, d_min))
        lt.check_types(self.tab, self.types, d_min)
        self._ref = {}

    def ref(self, listed):
        if listed not in self._ref:
            c, L, q, tab = self.c, self.c.L, self.c.x[:, 0], _rounded(self.tab)
            lists = (c.pairs, c.sc, c.sl) if listed else (np.zeros((0, 2), np.int64), np.zeros(0), np.zeros(0))
            self._ref[listed] = pl.per_set(lambda sel, lp, lsc, lsl: lt.near_table_step(
                q[sel], tab, self.types[sel], L.points[sel], c.Am, None, *c.split, *((lp, lsc, lsl) if listed else ())), L, *lists)
        return self._ref[listed]


def _typed(layout, box, T, unused):
    key = ("typed", layout, box, T)
    if key not in _CACHE:
        _CACHE[key] = Typed(layout, box, T, unused)
    return _CACHE[key]


def _run_table(tn, w, ex):
    c = w.c
    return _table_walk(tn, c.L.points, c.x[:, 0], _table(tn, w.tab, w.types), c.L.batch, c.Am, *c.split, ex)


@pytest.mark.parametrize("layout,box,T,unused,listed", TABLE_CASES, ids=["%s-%s-T%d%s" % (c[0], c[1], c[2], "-listed" if c[4] else "")
                                                                         for c in TABLE_CASES])
def test_table_walk_on_counted_cells(layout, box, T, unused, listed):
    """nfft_ewald_lj_table_near, both instantiations, against lj_table_ref.near_table_step on the float32-rounded table"""
    import torch_nfft_amd as tn
    w = _typed(layout, box, T, unused)
    c, L = w.c, w.c.L
    _assert_cells(tn, c)
    if T == 32:  # a half wave of a crowded cell's item mixes many rows of the table in LDS
        _, order, start = pf._sorted(L.points, L.batch, L.cells)
        k = int(np.argmax(start[1:] - start[:-1]))
        assert start[k + 1] - start[k] >= 300
        mixed = [len(set(w.types[order[t:t + 32]])) for t in range(int(start[k]), int(start[k + 1]) - 31, 32)]
        assert min(mixed) >= 16, mixed
    ex = c.exclusions(tn) if listed else None
    f, eight = _run_table(tn, w, ex)
    f2, eight2 = _run_table(tn, w, ex)
    tn.ops.check_status()
    assert torch.equal(f, f2) and torch.equal(eight, eight2)
    _check(c, "table_masked" if listed else "table_near", f, eight, *w.ref(listed))
    if listed:
        ones = c.classes["s(1,1)"]
        f1, eight1 = _run_table(tn, w, c.exclusions(tn, c.without(ones)))
        tn.ops.check_status()
        assert torch.equal(f, f1) and torch.equal(eight, eight1)


# ---- columns that are no points --------------------------------------------------------------------------------------------

def test_columns_outside_the_points_are_skipped():
    """twenty rows of ragged3's list get a column -1 in front and a column n behind, both with weights 1 (fully excluded, were
    they trusted); the rows stay ascending and row_start stays inside the arrays.  Both values are compared with indices and
    never used as one: the three kernels give the bits of the calls on the clean list."""
    import torch_nfft_amd as tn
    c = _lists("ragged3", "T")
    L = c.L
    clean = c.exclusions(tn, device="cpu")
    row_start = clean.row_start.numpy().astype(np.int64)
    col, wc, wl = clean.col.numpy(), clean.coulomb_weight.numpy(), clean.dispersion_weight.numpy()
    rng = np.random.default_rng(20)
    lengths = np.diff(row_start)
    chosen = np.concatenate([rng.permutation(np.flatnonzero(lengths > 0))[:16], rng.permutation(np.flatnonzero(lengths == 0))[:4]])
    assert chosen.size == 20 and (L.set_of()[chosen] == 0).any() and (L.set_of()[chosen] == 2).any()
    new_col, new_wc, new_wl, new_len = [], [], [], lengths.copy()
    spoil = set(chosen.tolist())
    for i in range(L.n):
        a, b = row_start[i], row_start[i + 1]
        extra = i in spoil
        new_col += ([-1] if extra else []) + col[a:b].tolist() + ([L.n] if extra else [])
        new_wc += ([1.0] if extra else []) + wc[a:b].tolist() + ([1.0] if extra else [])
        new_wl += ([1.0] if extra else []) + wl[a:b].tolist() + ([1.0] if extra else [])
        new_len[i] += 2 * extra
    start = np.concatenate([[0], np.cumsum(new_len)])
    assert start[-1] == len(new_col) == col.size + 40
    for i in chosen:
        row = new_col[start[i]:start[i + 1]]
        assert row[0] == -1 and row[-1] == L.n and (np.diff(row) > 0).all()
    spoiled = type("Spoiled", (), {})()
    spoiled.row_start, spoiled.col = _cuda(start.astype(np.int32)), _cuda(np.array(new_col, np.int32))
    spoiled.coulomb_weight, spoiled.dispersion_weight = _cuda(np.array(new_wc, np.float32)), _cuda(np.array(new_wl, np.float32))
    good = c.exclusions(tn)
    for op in (tn.ops.nfft_ewald_lj_excl_near, tn.ops.nfft_ewald_lj_excl_list):
        got, want = _excl_op(tn, c, op, spoiled), _excl_op(tn, c, op, good)
        tn.ops.check_status()
        assert bool(torch.isfinite(got[0]).all()) and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    w = _typed("ragged3", "T", 32, ())
    got, want = _run_table(tn, w, spoiled), _run_table(tn, w, good)
    tn.ops.check_status()
    assert bool(torch.isfinite(got[0]).all()) and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# ---- the list kernel's weights in r ------------------------------------------------------------------------------------------

SWEEP = (12.0, 13.0, 0.3)  # alpha_C, alpha_D, r_c in T
SWITCH = 0.125             # kSeriesSwitch of csrc/ewald_lj_excl.hip: u = alpha^2 r^2 below which its series run


def _sweep_points():
    """isolated listed pairs on the sites of a coarse lattice in T, a row of one entry per point: (s [2 m, 3] float32, pairs,
    the intended r [m], r from the float32 positions [m], the side of the two switches and of r_c that was meant [m, 3]: -1 or
    +1, and `on` [m]: r was put on a switch itself, where either branch may be taken)"""
    ac, ad, r_c = SWEEP
    lo, hi = math.sqrt(SWITCH) / ad, math.sqrt(SWITCH) / ac  # the two switch radii: alpha_D's is the smaller
    rs = [0.0] + list(np.geomspace(1e-4, 0.9 * r_c, 48)) + list(np.geomspace(2e-4, 0.85 * r_c, 28))
    rs += [math.sqrt(SWITCH * factor) / alpha for alpha in (ac, ad) for factor in (1 - 1e-3, 1.0, 1 + 1e-3)]
    rs += [lo + (hi - lo) / 3, lo + 2 * (hi - lo) / 3, r_c * (1 - 1e-3), r_c * (1 + 1e-3), 1.2 * r_c]
    rs = np.array(rs)
    m = rs.size
    on = np.zeros(m, bool)
    on[[1 + 48 + 28 + 1, 1 + 48 + 28 + 4]] = True
    assert np.allclose(rs[on], [hi, lo], rtol=1e-14)
    rng = np.random.default_rng(9)
    sites = np.array([(i, j, k) for i in range(5) for j in range(5) for k in range(4)], dtype=np.float64)
    assert m <= sites.shape[0]
    centres = (sites[rng.permutation(sites.shape[0])[:m]] + 0.5) / np.array([5.0, 5.0, 4.0]) - 0.5
    e = rng.standard_normal((m, 3))
    e /= np.linalg.norm(e, axis=1)[:, None]
    half = 0.5 * rs[:, None] * e @ np.linalg.inv(eb.T)
    s = np.concatenate([centres + half, centres - half]).astype(np.float32)
    s[m] = s[0]  # r = 0: the same bits
    pairs = np.stack([np.arange(m), np.arange(m) + m], 1)
    order = rng.permutation(2 * m)  # (the caller's order is not the pairs' order)
    place = np.empty(2 * m, np.int64)
    place[order] = np.arange(2 * m)
    s, pairs = s[order], place[pairs]
    ds = s[pairs[:, 0]].astype(np.float64) - s[pairs[:, 1]].astype(np.float64)
    r32 = np.linalg.norm((ds - np.rint(ds)) @ eb.T, axis=1)
    meant = np.stack([np.sign(rs - hi), np.sign(rs - lo), np.sign(rs - r_c)], 1)
    assert (meant[on, :2] == 0).sum() == 2 and (meant == 0).sum() == 2
    return s, pairs, rs, r32, meant


def test_list_kernel_radial_sweep():
    """the list kernel's weights from r = 0 to 1.2 r_c, on either side of each series / closed-form switch (u = 0.125 lies at
    another r for alpha_C than for alpha_D), between the two and on either side of r_c, against lj_excl_ref.smooth_parts
    (thirty terms, switch at 1/2: not the kernel's series) through lj_excl_ref.list_step.  F per point against that pair's own
    magnitude, so that a pair at 1e-4 is not hidden by one at r_c; the eight sums for all pairs and for the pairs below and
    above alpha_D's switch apart."""
    import torch_nfft_amd as tn
    ac, ad, r_c = SWEEP
    s, pairs, rs, r32, meant = _sweep_points()
    m, n = pairs.shape[0], s.shape[0]
    assert 85 <= m <= 95 and n == 2 * m
    # each r, as the float32 positions give it, still lies on the side of each switch and of r_c that was meant
    got_side = np.stack([np.sign((alpha * r32) ** 2 - SWITCH) for alpha in (ac, ad)] + [np.sign(r32 - r_c)], 1)
    for k in range(3):
        strict = meant[:, k] != 0
        assert (got_side[strict, k] == meant[strict, k]).all()
    assert np.abs(r32[1:] / rs[1:] - 1).max() < 2e-3 and r32[0] == 0  # (a position is rounded by 3e-8, the shortest pair is 1e-4)
    between = (meant[:, 0] < 0) & (meant[:, 1] > 0)  # the band between the two switch radii
    assert between.sum() >= 3 and (meant[:, 0] > 0).sum() > 10 and (meant[:, 1] < 0).sum() > 10 and (meant[:, 2] > 0).sum() == 2
    rng = np.random.default_rng(10)
    q, c, a = _coefficients(rng, n, eb.T, spacing=0.05)
    sc, sl = np.full(m, 0.5), np.full(m, 0.25)
    zero = np.zeros(n, np.float32)
    # (the Coulomb share of a pair's force is some hundred times its dispersion share: each is also taken alone, so that
    # neither of the two series hides behind the other)
    species = {"q and c": (q, c), "q alone": (q, zero), "c alone": (zero, c)}

    def run(which, qs, cs):
        ex = tn.ExclusionList(pairs[which], n, coulomb_scale=sc[which], dispersion_scale=sl[which])
        out = tn.ops.nfft_ewald_lj_excl_list(_cuda(s), _cuda(np.stack([qs, cs, a], 1)), None, ex.row_start, ex.col, ex.coulomb_weight,
                                             ex.dispersion_weight, _six(eb.T), ac, ad, r_c)
        tn.ops.check_status()
        fref, eref = le.list_step(qs, cs, s, eb.T, None, pairs[which], sc[which], sl[which], ac, ad, r_c)
        return out[0].cpu().numpy().astype(np.float64), out[1].cpu().numpy(), fref, eref

    everything, below = np.ones(m, bool), meant[:, 1] < 0
    twins, rest = pairs[0], pairs[1:]
    for name, (qs, cs) in species.items():
        f, eight, fref, eref = run(everything, qs, cs)
        assert np.isfinite(f).all() and np.isfinite(eight).all()
        assert not f[twins].any() and not fref[twins].any()  # r = 0: no force
        assert (np.linalg.norm(fref[rest.ravel()], axis=1) > 0).all()
        per_point = np.linalg.norm(f - fref, axis=1) / np.maximum(np.linalg.norm(fref, axis=1), 1e-300)
        per_pair = np.maximum(per_point[rest[:, 0]], per_point[rest[:, 1]])
        worst = int(np.argmax(per_pair))
        print("list kernel, radial sweep, %s: F per point worst %.3e at r = %.4e (u_C %.4f, u_D %.4f); at the smallest r %.3e, "
              "beyond r_c %.3e" % (name, per_pair[worst], r32[1 + worst], (ac * r32[1 + worst]) ** 2, (ad * r32[1 + worst]) ** 2,
                                   per_pair[np.argmin(r32[1:])], per_pair[r32[1:] > r_c].max()))
        print("  by r: " + " ".join("%.3g:%.1e" % (r32[1 + k], per_pair[k]) for k in np.argsort(r32[1:])))
        assert per_pair.max() <= GATES[("sweep", "F")], (name, per_pair.max(), r32[1 + worst])
        for label, which in (("all pairs", everything), ("below alpha_D's switch", below), ("above it", ~below)):
            _, eight, _, eref = run(which, qs, cs)
            e = {"W": rel_fro(eight[0, 2:], eref[0, 2:])}
            for key, k in (("U_C", 0), ("U_LJ", 1)):
                if eref[0, k]:
                    e[key] = _relative(eight[0, k:k + 1], eref[0, k:k + 1])
                else:
                    assert not eight[0, k]  # (no charges, or no dispersion coefficients: exactly nothing)
            print("list kernel, radial sweep, %s, %s (%d): %s" % (name, label, which.sum(), " ".join("%s %.3e" % kv for kv in sorted(e.items()))))
            for key, err in e.items():
                assert err <= GATES[("sweep", key)], (name, label, key, err)


# ---- one whole call ----------------------------------------------------------------------------------------------------------

def test_whole_lj_excl_step_on_the_ragged_layout():
    """nfft_ewald_lj_excl_step on ragged3 in T, fractional input (the round trip through float32 Cartesian positions moves the
    point on the face -1/2 into the cell across it, as tests/test_gpu_pair_frame_edges.py notes), cutoff = 4, against
    lj_excl_ref.exact_lj_excl_step"""
    import torch_nfft_amd as tn
    c = _lists("ragged3", "T")
    L, A = c.L, c.A
    alpha_c, alpha_d, r_c, N = WHOLE  # (alpha_D = 13, that of the sibling's whole call; the list was built for this r_c)
    assert (alpha_c, r_c) == (c.alpha_c, c.r_c)
    spc, spd = tn.EwaldSplitting(alpha_c, r_c, N, box=A), tn.DispersionSplitting(alpha_d, r_c, N, box=A)
    assert spc.cells == L.cells
    q, cc, a = c.x.T
    got = tn.nfft_ewald_lj_excl_step(_cuda(q), _cuda(cc), _cuda(a), _cuda(L.points), _cuda(L.batch), coulomb=spc, dispersion=spd,
                                     exclusions=c.exclusions(tn), cutoff=4, fractional=True)
    tn.ops.check_status()
    F, UC, ULJ, W = (t.cpu().numpy().astype(np.float64) for t in got)
    assert F.shape == (L.n, 3) and UC.shape == ULJ.shape == (3,) and W.shape == (3, 3, 3) and np.isfinite(F).all()
    assert not UC[1] and not ULJ[1] and not W[1].any()  # the empty set
    ref = le.exact_lj_excl_step(q, cc, a, L.points, A, L.batch, c.pairs, c.sc, c.sl, alpha_c, alpha_d, r_c, N)
    live = c.live
    e = {"F": rel_l2(F, ref[0]), "U_C": _relative(UC[live], ref[1][live]), "U_LJ": _relative(ULJ[live], ref[2][live]),
         "W": rel_fro(W[live], ref[3][live])}
    per = {k: rel_l2(F[rows], ref[0][rows]) for k, rows in _groups(L).items()}
    for name, which in c.classes.items():
        if which.size:
            ends = pl.ends(c.pairs, which)
            per[name] = rel_l2(F[ends], ref[0][ends])
    worst = max(per, key=per.get)
    print("nfft_ewald_lj_excl_step, ragged3 in T: %s; F worst %.3e (%s), spread %.2f; %s"
          % (" ".join("%s %.3e" % kv for kv in sorted(e.items())), per[worst], worst, per[worst] / min(per.values()),
             ", ".join("%s %.3e" % kv for kv in per.items())))
    for key, err in e.items():
        assert err <= GATES[("whole", key)], (key, err)
    for key, err in per.items():
        assert err <= GATES[("whole", "F")], (key, err)
    for b in live:  # Newton's third law per point set, the bound of tests/test_gpu_lj_excl.py::test_whole_call
        Fb = F[L.set_of() == b]
        assert np.abs(Fb.sum(0)).max() <= EXCL_WHOLE_TOL["F"] * math.sqrt(Fb.shape[0]) * np.linalg.norm(Fb)
