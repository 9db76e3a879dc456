"""GPU tests of the Lennard-Jones + Coulomb step with per-type-pair parameters: the pair walk of
csrc/ewald_lj_table.hip on its own, unmasked and masked, then nfft_ewald_lj_table_step as a whole, against the float64
restatement (tests/lj_table_ref.py) on the same float32 positions.

Points.  Without a list lj_step_ref.lj_points (700, a jittered lattice with the edge cases of the wrap and exact duplicates),
with one lj_excl_ref.bonded_points (600, or 300 + 0 + 300, and the 4 000-point layout over 3 x 3 x 3 cells), types drawn on
top; Lorentz-Berthelot tables with sigma between 0.5 and 0.8 d_min.  Every pair that keeps any repulsion is at least d_min
apart and sigma(t, t') <= 0.8 d_min for the types present, asserted in each box's metric.  For the whole call every position is
moved by (+3, -2, +1) lattice vectors, which rounds it to float32 once more; the restatement takes the moved values.

Tolerances.  Each gate is 4 x the largest relative error of the first device run against the float64 restatement, written
beside it, and none may exceed 1e-4 (the condition of section 7r); rel_l2 for F, rel_fro for W, the relative error for U.

The edges of the pair kernels' frame -- counted cells with 32 types mixed within a half wave, with and without a list -- are
in tests/test_gpu_pair_frame_lists.py.
"""
import math

import numpy as np
import pytest
import torch

import dispersion_virial_ref as dv
import ewald_box_ref as eb
import lj_excl_ref as le
import lj_step_ref as lj
import lj_table_ref as lt
from conftest import rel_l2
from ewald_virial_ref import rel_fro

pytestmark = pytest.mark.gpu

CEILING = 1e-4
# (the largest first-run figure in brackets)
NEAR_TOL = {  # the unmasked walk against brute force: forty cases of 700 points
    "F": 2.0e-6,     # (4.984e-7: S at (16, 0.22), one set, T = 1; 1.4e-7 .. 4.9e-7 on the others)
    # (1.345e-5: the unit cube, one set, every T -- the charges are the same for all four, and their +- q_i q_j w cancel to a
    # small remainder, as in tests/test_gpu_lj_step.py; 5.8e-6 in T at (12, 0.3), 3.3e-8 .. 4.3e-7 on the others)
    "U_C": 5.4e-5,
    "U_LJ": 1.3e-6,  # (3.219e-7: T at (12, 0.3), ragged, T = 2; 5.4e-9 .. 1.9e-7 on the others)
    "W": 4.4e-6,     # (1.085e-6: T at (12, 0.3), one set, T = 2; 9.7e-8 .. 7.8e-7 on the others)
}
MASKED_TOL = {  # the masked walk against brute force: six cases of 600 points and the one of 4 000
    "F": 1.6e-6,     # (3.917e-7: 4 000 points, T = 32; 1.6e-7 .. 2.0e-7 at 600)
    "U_C": 2.6e-6,   # (6.369e-7: 4 000 points; 2.0e-8 .. 5.5e-7 at 600)
    "U_LJ": 6.3e-7,  # (1.573e-7: 4 000 points; 1.3e-8 .. 4.3e-8 at 600)
    "W": 6.5e-7,     # (1.614e-7: O, ragged; 6.6e-8 .. 1.6e-7 on the others)
}
WHOLE_TOL = {  # nfft_ewald_lj_table_step (cutoff = 4) against the restatement, with and without a list, both inputs
    "F": 2.3e-6,     # (5.518e-7: T, ragged, with a list; 3.6e-7 .. 5.1e-7 on the others)
    "U_C": 4.8e-5,   # (1.188e-5: the unit cube, one set, without a list -- the pair walk's remainder above; 7.9e-7 .. 4.9e-6)
    "U_LJ": 2.7e-6,  # (6.655e-7: the unit cube, ragged, with a list)
    "W": 3.4e-6,     # (8.388e-7: T, ragged, with a list, fractional input)
}
assert max(max(t.values()) for t in (NEAR_TOL, MASKED_TOL, WHOLE_TOL)) <= CEILING
# the siblings against the float64 algorithm: WHOLE_TOL of tests/test_gpu_lj_step.py and tests/test_gpu_lj_excl.py, restated
LJ_STEP_TOL = {"F": 5.1e-6, "U_C": 1.2e-5, "U_LJ": 1.5e-6, "W": 1.2e-6}
LJ_EXCL_TOL = {"F": 2.6e-6, "U_C": 1.9e-5, "U_LJ": 3.8e-6, "W": 2.6e-6}

BOXES = {"T": eb.T, "O": eb.O, "S": eb.S, "I": np.eye(3)}
# box, alpha_C, r_c, the cells: NEAR_SPLITS of tests/test_gpu_ewald_step.py; alpha_D = alpha_C + 1.5
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
    return tn.LJPairTable(torch.from_numpy(tab[0]), torch.from_numpy(tab[1]), _cuda(types), grid_c=torch.from_numpy(tab[2]))


def _rounded(tab):
    """the table as the device holds it: (C12, dC6) and the grid coefficient rounded to float32, then float64 again -- the
    restatement takes the kernel's parameters, as it takes its float32 positions"""
    C6, C12, g = tab
    g32 = g.astype(np.float32).astype(np.float64)
    D6 = (C6 - np.outer(g, g)).astype(np.float32).astype(np.float64)
    return D6 + np.outer(g32, g32), C12.astype(np.float32).astype(np.float64), g32


def _walk(tn, s, q, table, batch, A, ac, ad, r_c, ex=None):
    xs = torch.stack([_cuda(q), table.c], 1)
    lists = (None,) * 4 if ex is None else (ex.row_start, ex.col, ex.coulomb_weight, ex.dispersion_weight)
    return tn.ops.nfft_ewald_lj_table_near(_cuda(s), xs, table.types, table.table, _cuda(batch), *lists, _six(A), ac, ad, r_c)


def _eight_errors(live, f, eight, fref, eref):
    f, eight = f.cpu().numpy().astype(np.float64), eight.cpu().numpy()
    assert np.isfinite(f).all() and np.isfinite(eight).all()
    assert np.linalg.norm(fref) > 0 and all(eref[b, :2].all() and np.linalg.norm(eref[b, 2:]) > 0 for b in live)
    return {"F": rel_l2(f, fref), "U_C": _relative(eight[live, 0], eref[live, 0]), "U_LJ": _relative(eight[live, 1], eref[live, 1]),
            "W": rel_fro(eight[live, 2:], eref[live, 2:])}


def _whole_errors(live, got, ref):
    g = [t.cpu().numpy().astype(np.float64) for t in got]
    return {"F": rel_l2(g[0], ref[0]), "U_C": _relative(g[1][live], ref[1][live]), "U_LJ": _relative(g[2][live], ref[2][live]),
            "W": rel_fro(g[3][live], ref[3][live])}


def _show(e):
    return " ".join("%s %.3e" % kv for kv in sorted(e.items()))


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
    assert lj.dr.min_separation(s, A) >= d_min * (1 - 1e-6)
    types = lt.draw_types(rng, 700, T, TYPE_COUNTS[T])
    assert set(types) == set(range(T)) - set(TYPE_COUNTS[T])
    tab = lt.lorentz_berthelot(*lt.type_parameters(rng, T, d_min))
    lt.check_types(tab, types, d_min)
    table = _table(tn, tab, types)
    args = (tn, s, q, table, batch, A, alpha, alpha + 1.5, r_c)
    f, eight = _walk(*args)
    f2, eight2 = _walk(*args)
    tn.ops.check_status()
    n, B = 700, 3 if ragged else 1
    live = [0, 2] if ragged else [0]
    assert f.shape == (n, 3) and f.dtype == torch.float32 and eight.shape == (B, 8) and eight.dtype == torch.float64
    assert torch.equal(f, f2) and torch.equal(eight, eight2)  # no atomics: the same bits
    fref, eref = lt.near_table_step(q, _rounded(tab), types, s, A, batch, alpha, alpha + 1.5, r_c)
    e = _eight_errors(live, f, eight, fref, eref)
    fn = f.cpu().numpy().astype(np.float64)
    newton = np.abs(fn.sum(0)).max() / np.abs(fn).sum()
    print("table walk, box %s (%g, %g) ragged=%d T=%d: %s; |sum F| / sum |F| %.2e" % (name, alpha, r_c, ragged, T, _show(e), newton))
    for key, err in e.items():
        assert err <= NEAR_TOL[key], (key, err)
    assert newton <= 3e-5  # (the bound of tests/test_gpu_lj_step.py: a hundred float32 additions per point)
    if ragged:
        assert not bool(eight[1].any())  # the empty point set: exactly zero


# ---- the masked walk -----------------------------------------------------------------------------------------------------

class Bonded:
    """the points of bonded_points in the box `name`, one set of n or three sets of n / 2, 0 and n / 2, with T types on top:
    float32 Cartesian positions x moved by (+3, -2, +1) lattice vectors and the float32 fractional positions s that they
    convert to; the list; the float64 references, each computed once"""

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
        # the move rounds a position by up to 2.4e-7: the builder's separations hold within 1e-4 of d_min
        for p, o, m in zip(parts, offs, sizes):  # (set by set: points of two sets do not see each other)
            r = le.check_separation(self.s[o:o + m], self.A, p[1], p[3], self.info["d_min"] * (1 - 1e-4))
            rl = r[p[1][:, 0], p[1][:, 1]]
            assert np.abs(rl - self.split[2]).min() > 1e-5 and (rl == 0).sum() == 1 and (rl >= self.split[2]).sum() == 1
        self.q = rng.standard_normal(self.n).astype(np.float32)
        self.types = lt.draw_types(rng, self.n, T)
        self.params = lt.type_parameters(rng, T, self.info["d_min"])
        self.tab = lt.lorentz_berthelot(*self.params)
        lt.check_types(self.tab, self.types, self.info["d_min"])
        self._ref = {}

    def lists(self, tn):
        return tn.ExclusionList(self.pairs, self.n, coulomb_scale=self.sc, dispersion_scale=self.sl, batch=self.batch)

    def ref(self, what):
        if what not in self._ref:
            ac, ad, r_c, N = self.split
            lists = (self.pairs, self.sc, self.sl)
            if what == "near":
                self._ref[what] = lt.near_table_step(self.q, _rounded(self.tab), self.types, self.s, self.A, self.batch, ac, ad, r_c, *lists)
            else:
                self._ref[what] = lt.exact_lj_table_step(self.q, _rounded(self.tab), self.types, self.s, self.A, self.batch, ac, ad, r_c,
                                                         N, *lists)
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
    for key, err in e.items():
        assert err <= MASKED_TOL[key], (key, err)
    # an empty list: the bits of the walk without one (which sees the bonded pairs in full: sums of 1e7, finite)
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
    _check_masked(tn, _bonded(name, ragged), "masked table walk")


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
    _check_masked(tn, w, "masked table walk")


# ---- the whole call ------------------------------------------------------------------------------------------------------

def _splittings(tn, name, A):
    ac, ad, r_c, N = SPLITS[name]
    box = None if name == "I" else A
    return tn.EwaldSplitting(ac, r_c, N, box=box), tn.DispersionSplitting(ad, r_c, N, box=box)


def _check_whole(tn, name, ragged, n, B, live, q, x, s, batch, table, ex, ref, label):
    spc, spd = _splittings(tn, name, BOXES[name])
    qd, xd, sd, bd = (_cuda(v) for v in (q, x, s, batch))
    cart = tn.nfft_ewald_lj_table_step(qd, table, xd, bd, coulomb=spc, dispersion=spd, exclusions=ex, cutoff=4)
    runs = [("Cartesian", cart)]
    if name != "I":
        runs.append(("fractional", tn.nfft_ewald_lj_table_step(qd, table, sd, bd, coulomb=spc, dispersion=spd, exclusions=ex,
                                                               fractional=True)))
    tn.ops.check_status()
    F, UC, ULJ, W = cart
    assert F.shape == (n, 3) and UC.shape == (B,) and ULJ.shape == (B,) and W.shape == (B, 3, 3)
    assert F.dtype == UC.dtype == ULJ.dtype == W.dtype == torch.float32 and torch.equal(W, W.transpose(1, 2))
    for t in cart:
        assert not t.requires_grad and bool(torch.isfinite(t).all())
    for what, got in runs:
        e = _whole_errors(live, got, ref)
        print("nfft_ewald_lj_table_step %s, box %s ragged=%d, %s input vs float64: %s" % (label, name, ragged, what, _show(e)))
        for key, err in e.items():
            assert err <= WHOLE_TOL[key], (key, err)
        if ragged:
            assert not bool(got[1][1]) and not bool(got[2][1]) and not bool(got[3][1].any())  # the empty set
    Fn = F.cpu().numpy().astype(np.float64)
    assert np.abs(Fn.sum(0)).max() <= WHOLE_TOL["F"] * math.sqrt(n) * np.linalg.norm(Fn)


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
        # the move rounds a position by up to 2.4e-7 and a duplicate like its original: the twenty duplicated pairs stay at
        # r = 0, which every sum skips, and everything else d_min apart
        ds = self.s[:, None, :].astype(np.float64) - self.s[None, :, :].astype(np.float64)
        r = np.linalg.norm((ds - np.rint(ds)) @ self.A, axis=-1)
        close = (r < d_min * (1 - 1e-4)) & ~np.eye(700, dtype=bool)
        assert close.sum() == 40 and not r[close].any()
        self.q = rng.standard_normal(700).astype(np.float32)
        self.types = lt.draw_types(rng, 700, 5, (3,))
        self.params = lt.type_parameters(rng, 5, d_min)
        self.tab = lt.lorentz_berthelot(*self.params)
        lt.check_types(self.tab, self.types, d_min)


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("name", ["I", "T", "O"])
def test_whole_call_without_a_list(name, ragged):
    import torch_nfft_amd as tn
    w = Free(name, ragged)
    ac, ad, r_c, N = SPLITS[name]
    ref = lt.exact_lj_table_step(w.q, _rounded(w.tab), w.types, w.s, w.A, w.batch, ac, ad, r_c, N)
    _check_whole(tn, name, ragged, w.n, w.B, w.live, w.q, w.x, w.s, w.batch, _table(tn, w.tab, w.types), None, ref, "without a list")


@pytest.mark.parametrize("listed", [False, True])
def test_a_geometric_table_is_the_step_of_the_siblings(listed):
    """LJPairTable.geometric against nfft_ewald_lj_step / nfft_ewald_lj_excl_step on lj_coefficients' (c, a) of the same sigma and
    epsilon: each side is within its gates of the float64 algorithm (the transforms spread with float atomics, and a_i a_j is
    rounded twice where C12 is rounded once), so the two differ by at most the gates' sum"""
    import torch_nfft_amd as tn
    w = _bonded("T", False) if listed else Free("T", False)  # (their points, types, sigma and epsilon; sqrt(sigma_i sigma_j) <= max)
    spc, spd = _splittings(tn, "T", w.A)
    sigma, eps = (torch.from_numpy(v) for v in w.params)
    types = _cuda(w.types)
    table = tn.LJPairTable.geometric(sigma, eps, types)
    assert float(table.table[..., 1].abs().max()) <= 1e-6 * float(table.c.max()) ** 2
    c, a = (v.cuda()[types].float() for v in tn.lj_coefficients(sigma, eps))
    qd, xd = _cuda(w.q), _cuda(w.x)
    if listed:
        ex = w.lists(tn)
        got = tn.nfft_ewald_lj_table_step(qd, table, xd, coulomb=spc, dispersion=spd, exclusions=ex)
        want = tn.nfft_ewald_lj_excl_step(qd, c, a, xd, coulomb=spc, dispersion=spd, exclusions=ex)
    else:
        got = tn.nfft_ewald_lj_table_step(qd, table, xd, coulomb=spc, dispersion=spd)
        want = tn.nfft_ewald_lj_step(qd, c, a, xd, coulomb=spc, dispersion=spd)
    tn.ops.check_status()
    e = _whole_errors([0], got, [t.cpu().numpy().astype(np.float64) for t in want])
    print("geometric table vs %s: %s" % ("nfft_ewald_lj_excl_step" if listed else "nfft_ewald_lj_step", _show(e)))
    other = LJ_EXCL_TOL if listed else LJ_STEP_TOL
    for key, err in e.items():
        assert err <= WHOLE_TOL[key] + other[key], (key, err)


# ---- types in device memory, no points, refusals ---------------------------------------------------------------------------

@pytest.mark.parametrize("listed", [False, True])
def test_a_type_changed_in_device_memory_is_clamped(listed):
    """table.types is checked once, at construction; a value written into it afterwards is clamped into [0, T) by the kernel,
    for the lane's own point and for a streamed one: the result is that of the clamped type, bit for bit, and nothing is read
    outside the table (T = 32 and T = 5: the last row of the table in LDS, and far beyond it)"""
    import torch_nfft_amd as tn
    w = _bonded("T", False)
    ac, ad, r_c, _ = w.split
    ex = w.lists(tn) if listed else None
    for T in (5, 32):
        rng = np.random.default_rng(T)
        types = lt.draw_types(rng, w.n, T)
        tab = lt.lorentz_berthelot(*lt.type_parameters(rng, T, w.info["d_min"]))
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
        whole = tn.nfft_ewald_lj_table_step(_cuda(w.q), spoiled, _cuda(w.x), coulomb=spc, dispersion=spd, exclusions=ex)
        tn.ops.check_status()
        assert all(bool(torch.isfinite(t).all()) for t in whole)


def test_no_points_and_refused_inputs():
    import torch_nfft_amd as tn
    one = torch.ones(2, 2, dtype=torch.float64)
    none = (None,) * 4
    empty = tn.LJPairTable(one, one, torch.zeros(0, dtype=torch.int64, device="cuda"))
    ex0 = tn.ExclusionList(np.zeros((0, 2), np.int64), 0)
    pos, xs = torch.zeros(0, 3, device="cuda"), torch.zeros(0, 2, device="cuda")
    walk = (_six(eb.T), 12.0, 13.0, 0.3)
    for lists in (none, (ex0.row_start, ex0.col, ex0.coulomb_weight, ex0.dispersion_weight)):
        f, eight = tn.ops.nfft_ewald_lj_table_near(pos, xs, empty.types, empty.table, None, *lists, *walk)
        assert f.shape == (0, 3) and eight.shape == (1, 8) and eight.dtype == torch.float64 and not bool(eight.any())
    tn.ops.check_status()
    tab = tn.LJPairTable(one, one, torch.tensor([0, 1, 1, 0], device="cuda"))
    four, x4, ex4 = torch.zeros(4, 3, device="cuda"), torch.zeros(4, 2, device="cuda"), tn.ExclusionList([[0, 1]], 4)
    lists = (ex4.row_start, ex4.col, ex4.coulomb_weight, ex4.dispersion_weight)
    op = tn.ops.nfft_ewald_lj_table_near
    for bad in (dict(xs=torch.zeros(4, 3, device="cuda")),                    # (q, c) per point, nothing else
                dict(types=tab.types.long()), dict(types=tab.types[:3]),      # int32, one per point
                dict(table=tab.table[:, :, :1]), dict(table=tab.table.double()), dict(table=tab.table[:1]),
                dict(table=torch.zeros(33, 33, 2, device="cuda")),            # more types than the LDS table holds
                dict(table=tab.table.cpu()), dict(types=tab.types.cpu()),
                dict(lists=lists[:1] + (None,) * 3), dict(lists=(None,) + lists[1:]),  # all four list tensors or none
                dict(lists=(ex0.row_start,) + lists[1:]), dict(lists=lists[:3] + (lists[3][:1],)),
                dict(walk=(_six(eb.T), 12.0, 13.0, 0.31)),                    # r_cut above a third of the smallest width
                dict(walk=(_six(eb.T), 12.0, float("nan"), 0.3))):
        a = dict(xs=x4, types=tab.types, table=tab.table, lists=lists, walk=walk)
        a.update(bad)
        with pytest.raises(RuntimeError, match="Input mismatch"):
            op(four, a["xs"], a["types"], a["table"], None, *a["lists"], *a["walk"])
    e = torch.zeros(0, device="cuda")
    spc, spd = tn.EwaldSplitting(12.0, 0.3, 32, box=eb.T), tn.DispersionSplitting(13.0, 0.3, 32, box=eb.T)
    for ex in (None, ex0):
        F, UC, ULJ, W = tn.nfft_ewald_lj_table_step(e, empty, pos, coulomb=spc, dispersion=spd, exclusions=ex)
        assert F.shape == (0, 3) and UC.shape == (1,) and not bool(UC.any()) and not bool(ULJ.any()) and not bool(W.any())
    with pytest.raises(ValueError, match="nfft_ewald_lj_table_step: table lives on cpu"):
        tn.nfft_ewald_lj_table_step(torch.zeros(4, device="cuda"), tn.LJPairTable(one, one, torch.tensor([0, 1, 1, 0])), four,
                                    coulomb=spc, dispersion=spd)
