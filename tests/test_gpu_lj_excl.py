"""GPU tests of the Lennard-Jones + Coulomb step with bonded-pair exclusions: the masked pair walk
(csrc/ewald_lj_step.hip) and the list kernel of csrc/ewald_lj_excl.hip on their own, then nfft_ewald_lj_excl_step as a whole, against the float64
restatement (tests/lj_excl_ref.py) on the same float32 positions.

Points.  lj_excl_ref.bonded_points: water-like molecules with bonds of sigma / 3, four-atom chains with scaled 1-4 pairs, a
hub with rows of 20, listed pairs through every face, a coincident pair, a listed pair beyond the cut, a row that spans
nearly all indices, atoms given outside the box -- 600 points in one set, or 300 + 0 + 300 in three.  Every pair that keeps
any repulsion is at least d_min apart with sigma <= 0.8 d_min, asserted by the builder in each box's metric.  Every position is
then moved by (+3, -2, +1) lattice vectors, Cartesian and fractional, which rounds it to float32 once more; the restatement
takes the moved float32 values, and the separations are asserted again on them.

Tolerances.  Each gate is 4 x the largest relative error of the first device run against the float64 restatement, written
beside it, and none may exceed 1e-4 (the condition of section 7r); rel_l2 for F, rel_fro for W, the relative error for U.

The edges of the pair kernels' frame -- counted cells, listed partners in a second and third LDS tile, every row shape of the
search, the list kernel's second loop trip and its weights in r -- are in tests/test_gpu_pair_frame_lists.py.
"""
import math

import numpy as np
import pytest
import torch

import ewald_box_ref as eb
import lj_excl_ref as le
from conftest import rel_l2
from ewald_virial_ref import rel_fro

pytestmark = pytest.mark.gpu

CEILING = 1e-4
# (the largest first-run figure in brackets; six cases of 600 points each, and for the two kernels the one of 4 000)
NEAR_TOL = {  # the masked walk against brute force
    "F": 1.6e-6,     # (3.808e-7: 4 000 points in the unit cube; 1.2e-7 .. 2.0e-7 at 600)
    "U_C": 2.1e-6,   # (5.046e-7: T, ragged; 4.2e-8 .. 5.0e-7 on the others)
    "U_LJ": 2.3e-6,  # (5.626e-7: 4 000 points; 8.9e-10 .. 9.8e-8 at 600)
    "W": 1.1e-6,     # (2.609e-7: the unit cube; 7.3e-8 .. 2.2e-7 on the others)
}
LIST_TOL = {  # the list kernel against float64: its weights and its eight sums are float64, its force sums float32
    "F": 3.7e-7,     # (9.029e-8: O, ragged; 4.6e-8 .. 9.0e-8 on the others)
    "U_C": 2.3e-8,   # (5.560e-9: O)
    "U_LJ": 6.3e-9,  # (1.568e-9: O)
    "W": 3.8e-7,     # (9.454e-8: O, ragged -- the float32 image d enters twice)
}
WHOLE_TOL = {  # nfft_ewald_lj_excl_step (cutoff = 4) against the restatement: I, T, O, one set and ragged, both inputs
    "F": 2.6e-6,     # (6.480e-7: T, ragged, fractional input; 4.2e-7 .. 6.5e-7)
    "U_C": 1.9e-5,   # (4.575e-6: O; the 2.9e-6 of nfft_ewald_lj_step's U_C, made by the same arithmetic, on other points)
    "U_LJ": 3.8e-6,  # (9.419e-7: the unit cube, ragged)
    "W": 2.6e-6,     # (6.330e-7: O, ragged, fractional input)
}
assert max(max(t.values()) for t in (NEAR_TOL, LIST_TOL, WHOLE_TOL)) <= CEILING
# nfft_ewald_lj_step against the float64 algorithm: WHOLE_TOL of tests/test_gpu_lj_step.py, restated
LJ_STEP_TOL = {"F": 5.1e-6, "U_C": 1.2e-5, "U_LJ": 1.5e-6, "W": 1.2e-6}

BOXES = {"T": eb.T, "O": eb.O, "I": np.eye(3)}
SPLITS = {"I": (12.0, 13.0, 0.3, 32), "T": (12.0, 13.0, 0.3, 32), "O": (14.0, 15.0, 0.25, 48)}  # alpha_C, alpha_D, r_c, N
MOVE = np.array([3.0, -2.0, 1.0])
_CASES = {}


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _six(A):
    return [A[0, 0], A[1, 0], A[1, 1], A[2, 0], A[2, 1], A[2, 2]]


def _relative(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / np.abs(want).max())


class Case:
    """the points of bonded_points in the box `name`, one set of 600 or three sets of 300, 0 and 300: float32 Cartesian
    positions x moved by (+3, -2, +1) lattice vectors, and the float32 fractional positions s that they convert to (moved
    likewise); the list; the float64 references, each computed once"""

    def __init__(self, name, ragged, n=600, G=7, seed=0):
        self.name, self.A, self.ragged = name, BOXES[name], ragged
        self.split = SPLITS[name]
        rng = np.random.default_rng(ord(name) + 7 * ragged + seed)
        sizes = [n // 2, n // 2] if ragged else [n]
        parts = [le.bonded_points(rng, m, self.A, self.split[2], G=G) for m in sizes]
        offs = np.cumsum([0] + sizes)
        s0 = np.concatenate([p[0] for p in parts])
        self.pairs = np.concatenate([p[1] + o for p, o in zip(parts, offs)])
        self.sc, self.sl = np.concatenate([p[2] for p in parts]), np.concatenate([p[3] for p in parts])
        self.info = parts[0][4]
        self.tight = np.concatenate([p[4]["tight"] + o for p, o in zip(parts, offs)])
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
        self.q, self.c, self.a = le.coefficients(rng, self.n, self.info)
        self._ref = {}

    def lists(self, tn):
        return tn.ExclusionList(self.pairs, self.n, coulomb_scale=self.sc, dispersion_scale=self.sl, batch=self.batch)

    def ref(self, what):
        if what not in self._ref:
            ac, ad, r_c, N = self.split
            args = (self.s, self.A, self.batch, self.pairs, self.sc, self.sl)
            if what == "near":
                self._ref[what] = le.near_step_scaled(self.q, self.c, self.a, *args, ac, ad, r_c)
            elif what == "list":
                self._ref[what] = le.list_step(self.q, self.c, *args, ac, ad, r_c)
            else:
                self._ref[what] = le.exact_lj_excl_step(self.q, self.c, self.a, *args, ac, ad, r_c, N)
        return self._ref[what]


def _case(name, ragged):
    if (name, ragged) not in _CASES:
        _CASES[(name, ragged)] = Case(name, ragged)
    return _CASES[(name, ragged)]


def _native(tn, w, op, ex=None):
    ex = w.lists(tn) if ex is None else ex
    ac, ad, r_c, _ = w.split
    xs = _cuda(np.stack([w.q, w.c, w.a], 1))
    return op(_cuda(w.s), xs, _cuda(w.batch), ex.row_start, ex.col, ex.coulomb_weight, ex.dispersion_weight, _six(w.A), ac, ad, r_c)


def _eight_errors(w, f, eight, fref, eref):
    f, eight = f.cpu().numpy().astype(np.float64), eight.cpu().numpy()
    assert np.isfinite(f).all() and np.isfinite(eight).all()
    assert np.linalg.norm(fref) > 0 and all(eref[b, :2].all() and np.linalg.norm(eref[b, 2:]) > 0 for b in w.live)
    return {"F": rel_l2(f, fref), "U_C": _relative(eight[w.live, 0], eref[w.live, 0]), "U_LJ": _relative(eight[w.live, 1], eref[w.live, 1]),
            "W": rel_fro(eight[w.live, 2:], eref[w.live, 2:])}


def _check_native(tn, w, op, what, tol, label):
    f, eight = _native(tn, w, op)
    f2, eight2 = _native(tn, w, op)
    tn.ops.check_status()
    assert f.shape == (w.n, 3) and f.dtype == torch.float32 and eight.shape == (w.B, 8) and eight.dtype == torch.float64
    assert torch.equal(f, f2) and torch.equal(eight, eight2)  # no atomics: the same bits
    e = _eight_errors(w, f, eight, *w.ref(what))
    print("%s, box %s ragged=%d n=%d: %s" % (label, w.name, w.ragged, w.n, " ".join("%s %.3e" % kv for kv in sorted(e.items()))))
    if w.ragged:
        assert not bool(eight[1].any())  # the empty point set: exactly zero
    for key, err in e.items():
        assert err <= tol[key], (key, err)
    return f, eight


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("name", ["I", "T", "O"])
def test_masked_walk_against_brute_force(name, ragged):
    """the masked pair walk alone against the float64 sum of the SCALED pair terms"""
    import torch_nfft_amd as tn
    w = _case(name, ragged)
    _check_native(tn, w, tn.ops.nfft_ewald_lj_excl_near, "near", NEAR_TOL, "masked walk")


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("name", ["I", "T", "O"])
def test_list_kernel_against_float64(name, ragged):
    """the list kernel alone against float64 on the same reduced positions: the smooth share within r_c (r = 0 included),
    the whole Coulomb and dispersion terms of the pair beyond"""
    import torch_nfft_amd as tn
    w = _case(name, ragged)
    f, _ = _check_native(tn, w, tn.ops.nfft_ewald_lj_excl_list, "list", LIST_TOL, "list kernel")
    rows = np.bincount(w.pairs.ravel(), minlength=w.n)
    assert not bool(f[_cuda(np.flatnonzero(rows == 0))].any())  # a point with an empty row: exactly zero
    i, j = w.info["coincident"]
    assert not bool(f[i].any()) and not bool(f[j].any())  # (their rows hold each other only: no force at r = 0)


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("name", ["I", "T", "O"])
def test_whole_call(name, ragged):
    """the unit cube (box=None), a triclinic and an orthorhombic box, Cartesian and fractional positions moved by (+3, -2, +1)
    lattice vectors, against the float64 restatement"""
    import torch_nfft_amd as tn
    w = _case(name, ragged)
    ac, ad, r_c, N = w.split
    box = None if name == "I" else w.A
    spc, spd = tn.EwaldSplitting(ac, r_c, N, box=box), tn.DispersionSplitting(ad, r_c, N, box=box)
    ex = w.lists(tn)
    qd, cd, ad_, xd, sd, bd = (_cuda(v) for v in (w.q, w.c, w.a, w.x, w.s, w.batch))
    ref = w.ref("whole")
    cart = tn.nfft_ewald_lj_excl_step(qd, cd, ad_, xd, bd, coulomb=spc, dispersion=spd, exclusions=ex, cutoff=4)
    runs = [("Cartesian", cart)]
    if name != "I":
        runs.append(("fractional", tn.nfft_ewald_lj_excl_step(qd, cd, ad_, sd, bd, coulomb=spc, dispersion=spd, exclusions=ex,
                                                              fractional=True)))
    tn.ops.check_status()
    F, UC, ULJ, W = cart
    assert F.shape == (w.n, 3) and UC.shape == (w.B,) and ULJ.shape == (w.B,) and W.shape == (w.B, 3, 3)
    assert F.dtype == UC.dtype == ULJ.dtype == W.dtype == torch.float32 and torch.equal(W, W.transpose(1, 2))
    for t in cart:
        assert not t.requires_grad and bool(torch.isfinite(t).all())
    for what, got in runs:
        g = [t.cpu().numpy().astype(np.float64) for t in got]
        e = {"F": rel_l2(g[0], ref[0]), "U_C": _relative(g[1][w.live], ref[1][w.live]), "U_LJ": _relative(g[2][w.live], ref[2][w.live]),
             "W": rel_fro(g[3][w.live], ref[3][w.live])}
        print("nfft_ewald_lj_excl_step, box %s ragged=%d, %s input vs float64: %s"
              % (name, ragged, what, " ".join("%s %.3e" % kv for kv in sorted(e.items()))))
        for key, err in e.items():
            assert err <= WHOLE_TOL[key], (key, err)
        if ragged:
            assert not bool(got[1][1]) and not bool(got[2][1]) and not bool(got[3][1].any())  # the empty set
    Fn = F.cpu().numpy().astype(np.float64)
    assert np.abs(Fn.sum(0)).max() <= WHOLE_TOL["F"] * math.sqrt(w.n) * np.linalg.norm(Fn)


@pytest.mark.parametrize("name", ["I", "T"])
def test_what_subtracting_afterwards_would_leave(name):
    """The test that shows the point.  A correction applied after the walk would first hold a_i a_j 12 d / r^14 of a bonded pair
    in the float32 force sum of each end, and leave its rounding, 2^-24 a_i a_j 12 / r^13, behind.  Over the ends of the
    tightest fully excluded bonds (r = sigma / 3) that is at least 100 x what the gate on F allows these points; the masked
    call keeps them within the gate."""
    import torch_nfft_amd as tn
    w = _case(name, False)
    ac, ad, r_c, N = w.split
    box = None if name == "I" else w.A
    spc, spd = tn.EwaldSplitting(ac, r_c, N, box=box), tn.DispersionSplitting(ad, r_c, N, box=box)
    F = tn.nfft_ewald_lj_excl_step(*(_cuda(v) for v in (w.q, w.c, w.a, w.x)), coulomb=spc, dispersion=spd, exclusions=w.lists(tn))[0]
    tn.ops.check_status()
    ref = w.ref("whole")[0]
    i, j = w.tight[:, 0], w.tight[:, 1]
    ds = w.s[i].astype(np.float64) - w.s[j].astype(np.float64)
    r = np.linalg.norm((ds - np.rint(ds)) @ w.A, axis=1)
    assert np.abs(r / (w.info["sigma"] / 3.0) - 1).max() < 1e-3
    left = 2.0 ** -24 * w.a[i].astype(np.float64) * w.a[j].astype(np.float64) * 12.0 / r ** 13  # at each end of the bond
    ends = np.concatenate([i, j])
    gate = WHOLE_TOL["F"] * np.linalg.norm(ref[ends])
    would = np.linalg.norm(np.concatenate([left, left]))
    err = np.linalg.norm(F.cpu().numpy().astype(np.float64)[ends] - ref[ends])
    print("box %s: %d ends of tight bonds, |F| there %.3e; subtracting afterwards would leave %.3e = %.0f x the gate %.3e; "
          "the error is %.3e" % (name, ends.size, np.linalg.norm(ref[ends]), would, would / gate, gate, err))
    assert would >= 100 * gate
    assert err <= gate


@pytest.mark.parametrize("ragged", [False, True])
def test_an_empty_list_gives_the_bits_of_the_unmasked_walk(ragged):
    import torch_nfft_amd as tn
    w = _case("T", ragged)
    ac, ad, r_c, _ = w.split
    empty = tn.ExclusionList(np.zeros((0, 2), np.int64), w.n, batch=w.batch)
    f, eight = _native(tn, w, tn.ops.nfft_ewald_lj_excl_near, empty)
    f0, eight0 = tn.ops.nfft_ewald_lj_step_near(_cuda(w.s), _cuda(np.stack([w.q, w.c, w.a], 1)), _cuda(w.batch), _six(w.A), ac, ad, r_c)
    lf, leight = _native(tn, w, tn.ops.nfft_ewald_lj_excl_list, empty)
    tn.ops.check_status()
    # (the unmasked walk sees the bonded pairs in full: sums of 1e7, finite)
    assert bool(torch.isfinite(f0).all()) and torch.equal(f, f0) and torch.equal(eight, eight0)
    assert not bool(lf.any()) and not bool(leight.any())


@pytest.mark.parametrize("ragged", [False, True])
def test_without_a_list_it_is_nfft_ewald_lj_step(ragged):
    """exclusions=None takes the code path of nfft_ewald_lj_step.  Its transforms spread with float atomics, so two calls
    differ in the last bits: each is within the gates of tests/test_gpu_lj_step.py of the float64 algorithm, the two within
    their sum.  On one atom of every bonded cluster: nfft_ewald_lj_step has no way to leave a bond's r^-12 out."""
    import torch_nfft_amd as tn
    w = _case("T", ragged)
    ac, ad, r_c, N = w.split
    spc, spd = tn.EwaldSplitting(ac, r_c, N, box=w.A), tn.DispersionSplitting(ad, r_c, N, box=w.A)
    # one atom per listed cluster: no pair closer than d_min is left
    keep = np.ones(w.n, dtype=bool)
    keep[w.pairs[w.sl == 0.0].max(1)] = False
    batch = None if w.batch is None else _cuda(w.batch[keep])
    args = [_cuda(v[keep]) for v in (w.q, w.c, w.a, w.x)] + [batch]
    got = tn.nfft_ewald_lj_excl_step(*args, coulomb=spc, dispersion=spd, exclusions=None)
    want = tn.nfft_ewald_lj_step(*args, coulomb=spc, dispersion=spd)
    tn.ops.check_status()
    g, r = [t.cpu().numpy().astype(np.float64) for t in got], [t.cpu().numpy().astype(np.float64) for t in want]
    e = {"F": rel_l2(g[0], r[0]), "U_C": _relative(g[1][w.live], r[1][w.live]), "U_LJ": _relative(g[2][w.live], r[2][w.live]),
         "W": rel_fro(g[3][w.live], r[3][w.live])}
    print("exclusions=None vs nfft_ewald_lj_step, ragged=%d, %d points: %s" % (ragged, int(keep.sum()), " ".join("%s %.3e" % kv for kv in sorted(e.items()))))
    for key, err in e.items():
        assert err <= 2 * LJ_STEP_TOL[key], (key, err)


def test_large_cells_and_a_second_tile():
    """about 4 000 points over 3 x 3 x 3 cells: a cell holds more than the 128 points of a work item and a walked range more
    than the 256 of an LDS tile, so staged indices are read from a second tile"""
    import torch_nfft_amd as tn
    if "large" not in _CASES:
        _CASES["large"] = Case("I", False, n=4000, G=12, seed=5)
    w = _CASES["large"]
    assert tn.EwaldSplitting(w.split[0], w.split[2], 32, box=np.eye(3)).cells == (3, 3, 3)
    s = w.s.astype(np.float64)
    cell = np.floor((s - np.rint(s) + 0.5) * 3).astype(np.int64).clip(0, 2)
    counts = np.bincount(cell[:, 0] + 3 * cell[:, 1] + 9 * cell[:, 2], minlength=27)
    assert counts.max() > 128 and counts.reshape(9, 3).sum(1).min() > 256
    _check_native(tn, w, tn.ops.nfft_ewald_lj_excl_near, "near", NEAR_TOL, "masked walk")
    _check_native(tn, w, tn.ops.nfft_ewald_lj_excl_list, "list", LIST_TOL, "list kernel")


def test_no_points_and_refused_inputs():
    import torch_nfft_amd as tn
    pos, xs = torch.zeros(0, 3, device="cuda"), torch.zeros(0, 3, device="cuda")
    ex = tn.ExclusionList(np.zeros((0, 2), np.int64), 0)
    for op in (tn.ops.nfft_ewald_lj_excl_near, tn.ops.nfft_ewald_lj_excl_list):
        f, eight = op(pos, xs, None, ex.row_start, ex.col, ex.coulomb_weight, ex.dispersion_weight, _six(eb.T), 12.0, 13.0, 0.3)
        assert f.shape == (0, 3) and eight.shape == (1, 8) and eight.dtype == torch.float64 and not bool(eight.any())
    tn.ops.check_status()
    four, ex4 = torch.zeros(4, 3, device="cuda"), tn.ExclusionList([[0, 1]], 4)
    lists = (ex4.row_start, ex4.col, ex4.coulomb_weight, ex4.dispersion_weight)
    for op in (tn.ops.nfft_ewald_lj_excl_near, tn.ops.nfft_ewald_lj_excl_list):
        with pytest.raises(RuntimeError, match="Input mismatch"):  # (q, c, a) per point, nothing else
            op(four, torch.zeros(4, 2, device="cuda"), None, *lists, _six(eb.T), 12.0, 13.0, 0.3)
        with pytest.raises(RuntimeError, match="Input mismatch"):  # r_cut above a third of the smallest width
            op(four, torch.zeros(4, 3, device="cuda"), None, *lists, _six(eb.T), 12.0, 13.0, 0.31)
        with pytest.raises(RuntimeError, match="Input mismatch"):  # a list over another number of points
            op(four, torch.zeros(4, 3, device="cuda"), None, ex.row_start, ex.col, ex.coulomb_weight, ex.dispersion_weight,
               _six(eb.T), 12.0, 13.0, 0.3)
        with pytest.raises(RuntimeError, match="Input mismatch"):  # one weight per entry
            op(four, torch.zeros(4, 3, device="cuda"), None, ex4.row_start, ex4.col, ex4.coulomb_weight, ex4.dispersion_weight[:1],
               _six(eb.T), 12.0, 13.0, 0.3)
    e = torch.zeros(0, device="cuda")
    spc, spd = tn.EwaldSplitting(12.0, 0.3, 32, box=eb.T), tn.DispersionSplitting(13.0, 0.3, 32, box=eb.T)
    F, UC, ULJ, W = tn.nfft_ewald_lj_excl_step(e, e, e, pos, coulomb=spc, dispersion=spd, exclusions=ex)
    assert F.shape == (0, 3) and UC.shape == (1,) and not bool(UC.any()) and not bool(ULJ.any()) and not bool(W.any())
