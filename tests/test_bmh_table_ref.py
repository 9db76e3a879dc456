"""CPU tests of the Buckingham / Born-Mayer-Huggins + Coulomb step with per-type-pair parameters: the
float64 restatement tests/bmh_table_ref.py against the restatement of section 7t (A = 0, C8 = 0), against an independent
composition of converged sums, against central differences of that energy and against four wrong formulas; BMHPairTable's
constructors and refusals; the refusals of nfft_ewald_bmh_table_step before any device work, the operator schema, the C ABI's
validation and the resource figures of csrc/ewald_bmh_table.hip."""
import ctypes
import re

import numpy as np
import pytest
import torch

import bmh_table_ref as bt
import ewald_box_ref as eb
import lj_step_ref as lj
import lj_table_ref as lt
from conftest import rel_l2
from ewald_virial_ref import rel_fro

# The split and its truncation factors are those of tests/test_lj_table_ref.py: the table's own terms are summed directly
# within r_c on both sides and carry no truncation, so the restatement stands within the largest factor, 3.9e-6, of the
# converged composition; 1e-5 leaves a factor 2.5.
SPLIT = (13.0, 14.0, 0.3, 40)  # alpha_C, alpha_D, r_c, N
TRUNCATION = 1e-5
# the largest gate of tests/test_gpu_bmh_table.py on F, U_sr and W (that file asserts it at import); each wrong formula must
# move what it bears on by 1e3 times as much
LARGEST_TABLE_GATE = 4.0e-6
D_MIN = 0.14
N_FREE, N_BONDED, TYPES = 30, 44, 3


@pytest.fixture(scope="module")
def system():
    """30 points in the triclinic box T, no two closer than D_MIN, three types with r_m = 1.0, 0.7 .. 1.0 and 0.7 D_MIN; partial
    charges of 0.4, so that the table's terms are no small share of the force"""
    rng = np.random.default_rng(31)
    s = lj.separated_points(rng, N_FREE, eb.T, D_MIN).astype(np.float32).astype(np.float64)
    q = 0.4 * rng.standard_normal(N_FREE)
    q -= q.mean()
    types = lt.draw_types(rng, N_FREE, TYPES)
    tab = bt.exp6_parameters(rng, TYPES, D_MIN)
    bt.check_system(tab, types, s, eb.T, None, SPLIT[2], D_MIN * (1 - 1e-6))
    return s, q, types, tab


@pytest.fixture(scope="module")
def bonded():
    """44 points of lj_excl_ref.bonded_points in T with three types on top"""
    rng = np.random.default_rng(33)
    s, pairs, sc, sl, info = lt.le.bonded_points(rng, N_BONDED, eb.T, SPLIT[2])
    types = lt.draw_types(rng, N_BONDED, TYPES)
    tab = bt.exp6_parameters(rng, TYPES, info["d_min"])
    bt.check_system(tab, types, s, eb.T, None, SPLIT[2], info["d_min"] * (1 - 1e-5), pairs, sl)
    q = rng.standard_normal(N_BONDED)
    q -= q.mean()
    return s.astype(np.float64), q, types, tab, pairs, sc, sl, info


def _errors(got, want, scale_sr=None):
    F, UC, USR, W = got
    rF, rUC, rUSR, rW = want
    scale_sr = abs(rUSR[0]) if scale_sr is None else scale_sr
    return {"F": rel_l2(F, rF), "U_C": abs(UC[0] / rUC[0] - 1), "U_sr": abs(USR[0] - rUSR[0]) / scale_sr, "W": rel_fro(W, rW)}


def _show(e):
    return " ".join("%s %.3e" % kv for kv in sorted(e.items()))


def test_without_exponential_and_c8_it_is_the_table_step_of_7t(system, bonded):
    """A = 0 and C8 = 0 leave -C6 / r^6 alone: lj_table_ref with C12 = 0, with and without a list"""
    s, q, types, tab, = system
    zero = np.zeros_like(tab[0])
    mine, theirs = (zero, tab[1], tab[2], zero, tab[4]), (tab[2], zero, tab[4])
    e = _errors(bt.exact_bmh_table_step(q, mine, types, s, eb.T, None, *SPLIT, shares=False), lt.exact_lj_table_step(q, theirs, types, s, eb.T, None, *SPLIT))
    print("A = C8 = 0 vs lj_table_ref: %s" % _show(e))
    assert max(e.values()) <= 1e-12
    s, q, types, tab, pairs, sc, sl, _ = bonded
    mine, theirs = (zero, tab[1], tab[2], zero, tab[4]), (tab[2], zero, tab[4])
    for b in (None, np.zeros(N_BONDED, np.int64)):
        e = _errors(bt.exact_bmh_table_step(q, mine, types, s, eb.T, b, *SPLIT, pairs, sc, sl, shares=False),
                    lt.exact_lj_table_step(q, theirs, types, s, eb.T, b, *SPLIT, pairs, sc, sl))
        print("A = C8 = 0 vs lj_table_ref, with a list: %s" % _show(e))
        assert max(e.values()) <= 1e-12
    fa, ea = bt.near_bmh_step(q, mine, types, s, eb.T, None, *SPLIT[:3], pairs, sc, sl, shares=False)
    fb, eb8 = lt.near_table_step(q, theirs, types, s, eb.T, None, *SPLIT[:3], pairs, sc, sl)
    assert rel_l2(fa, fb) <= 1e-12 and np.abs(ea - eb8).max() <= 1e-12 * np.abs(eb8).max()


def _trace(cUC, parts):
    """(U_C - 6 U_D - 6 U_delta - 8 U_8 + 1/2 sum A B r e^(-B r), the sum of the terms' sizes)"""
    _, UD, UA, UX, U8, HB = parts
    want = cUC[0] - 6.0 * UD[0] - 6.0 * UX[0] - 8.0 * U8[0] + HB[0]
    return want, abs(cUC[0]) + 6.0 * abs(UD[0]) + 6.0 * abs(UX[0]) + 8.0 * abs(U8[0]) + abs(HB[0])


def test_against_the_converged_composition(system):
    """against the converged Coulomb sum, the brute-force c_i c_j / r^6 lattice sum over every image within R = 14 and the
    table's three terms summed directly within r_c; Newton's third law; the trace identity"""
    s, q, types, tab = system
    got = bt.exact_bmh_table_step(q, tab, types, s, eb.T, None, *SPLIT)
    cF, cUC, cUSR, cW, parts = bt.converged_bmh_table_step(q, tab, types, s, eb.T, SPLIT[2], R=14.0)
    _, UD, UA, UX, U8, HB = parts
    e = _errors(got, (cF, cUC, cUSR, cW), abs(UD[0]) + abs(UA[0]) + abs(UX[0]) + abs(U8[0]))
    print("restatement vs converged composition: %s" % _show(e))
    assert max(e.values()) <= TRUNCATION
    F, _, _, W = got
    assert np.abs(F.sum(0)).max() <= 1e-9 * np.abs(F).sum() and np.abs(cF.sum(0)).max() <= 1e-9 * np.abs(cF).sum()
    assert np.abs(W - W.transpose(0, 2, 1)).max() <= 1e-12 * np.abs(W).max()
    # the exponential is not homogeneous in the lengths: -r u' = B r u for it, where a power -k gives k u
    want, size = _trace(cUC, parts)
    print("tr W %.9g, U_C - 6 U_D - 6 U_delta - 8 U_8 + half_ABr %.9g (U_A %.6g U_delta %.6g U_8 %.6g half_ABr %.6g)"
          % (np.trace(cW[0]), want, UA[0], UX[0], U8[0], HB[0]))
    assert abs(np.trace(cW[0]) - want) <= 1e-7 * size
    assert abs(np.trace(W[0]) - want) <= 3.0 * TRUNCATION * size
    assert min(abs(HB[0]), 8.0 * abs(U8[0]), 6.0 * abs(UX[0])) >= 1e3 * 1e-7 * size  # (the identity would notice each term)
    assert abs(bt.half_ABr(tab, types, s, eb.T, None, SPLIT[2], nimg=1)[0] - HB[0]) <= 1e-14 * abs(HB[0])


def test_with_exclusions_against_the_converged_composition(bonded):
    s, q, types, tab, pairs, sc, sl, info = bonded
    got = bt.exact_bmh_table_step(q, tab, types, s, eb.T, None, *SPLIT, pairs, sc, sl)
    # (each side takes the r = 0 constants of its own alphas; converged_lj_excl_step's defaults are those of its sums)
    cF, cUC, cUSR, cW, parts = bt.converged_bmh_table_step(q, tab, types, s, eb.T, SPLIT[2], pairs, sc, sl)
    _, UD, UA, UX, U8, HB = parts
    e = _errors(got, (cF, cUC, cUSR, cW), abs(UD[0]) + abs(UA[0]) + abs(UX[0]) + abs(U8[0]))
    print("with exclusions, restatement vs converged composition: %s" % _show(e))
    assert max(e.values()) <= TRUNCATION
    want, size = _trace(cUC, parts)
    assert abs(np.trace(cW[0]) - want) <= 1e-6 * size
    assert np.abs(got[0].sum(0)).max() <= 1e-9 * np.abs(got[0]).sum()


def test_force_and_virial_are_derivatives_of_the_energy(system):
    """F = -dU/dx and W = -dU/d eps by central differences (h = 1e-5) of the converged energy, thresholds as in
    tests/test_lj_table_ref.py: the exponential's third derivative is B^2 = (14 / 0.7 d_min)^2 = 2e4 times the first, the
    truncation h^2 |U'''| / 6 is 4e-7 relative; 1e-5 leaves a factor 25.  No pair may cross r_c on the way: all three table
    terms jump there."""
    s, q, types, tab = system
    A, r_c, h = eb.T, SPLIT[2], 1e-5
    ds = s[:, None, :] - s[None, :, :]
    r = np.linalg.norm((ds - np.rint(ds)) @ A, axis=-1)
    assert np.abs(r - r_c).min() > 10 * h  # (a point moves by h, a strained separation by h r)
    F, _, _, W, _ = bt.converged_bmh_table_step(q, tab, types, s, A, r_c)
    inv = np.linalg.inv(A)
    energy = lambda s_, A_: bt.converged_energy(q, tab, types, s_, A_, r_c)
    fd = np.zeros((N_FREE, 3))
    for i in range(N_FREE):
        for k in range(3):
            dx = np.zeros(3)
            dx[k] = h
            sp, sm = s.copy(), s.copy()
            sp[i] += dx @ inv
            sm[i] -= dx @ inv
            fd[i, k] = -(energy(sp, A) - energy(sm, A)) / (2 * h)
    e = np.abs(F - fd).max() / np.abs(F).max()
    print("F against central differences: %.3e of |F|_max %.3g" % (e, np.abs(F).max()))
    assert e <= 1e-5
    fw = np.zeros((3, 3))
    for k in range(3):
        for l in range(3):
            eps = np.zeros((3, 3))
            eps[k, l] = h
            fw[k, l] = -(energy(s, A @ (np.eye(3) + eps)) - energy(s, A @ (np.eye(3) - eps))) / (2 * h)
    e = np.abs(W[0] - fw).max() / np.abs(W).max()
    print("W against central differences: %.3e of |W|_max %.3g" % (e, np.abs(W).max()))
    assert e <= 1e-5


@pytest.mark.parametrize("mutant", ["slope_without_b", "c8_sign", "six_for_eight", "a_unscaled"])
def test_mutants_are_far_off(system, bonded, mutant):
    """each wrong formula moves what it bears on -- F and W; the energy too unless only a slope is wrong -- by at least 1e3 x the
    largest gate that the device comparison has for those quantities"""
    floor = 1e3 * LARGEST_TABLE_GATE
    if mutant == "a_unscaled":  # (needs a list: the 1-4 pairs keep half their short-range term)
        s, q, types, tab, pairs, sc, sl, _ = bonded
        args = (q, tab, types, s, eb.T, None, *SPLIT, pairs, sc, sl)
    else:
        s, q, types, tab = system
        args = (q, tab, types, s, eb.T, None, *SPLIT)
    F, UC, USR, W = bt.exact_bmh_table_step(*args)
    Fm, UCm, USRm, Wm = bt.exact_bmh_table_step(*args, mutant=mutant)
    e = rel_l2(Fm, F), abs(USRm[0] - USR[0]) / abs(USR[0]), rel_fro(Wm, W)
    print("mutant %-16s relative error of F %.3e, U_sr %.3e, W %.3e" % ((mutant,) + e))
    assert UCm[0] == UC[0]
    if mutant in ("slope_without_b", "six_for_eight"):
        assert e[0] >= floor and e[2] >= floor and e[1] == 0.0
    else:
        assert min(e) >= floor


def _t(a, dtype=torch.float64):
    return torch.as_tensor(np.asarray(a), dtype=dtype)


def test_pair_table_constructors_and_refusals():
    import torch_nfft
    import torch_nfft_amd as tn
    assert "BMHPairTable" in tn.__all__ and torch_nfft.BMHPairTable is tn.BMHPairTable is tn.bmh.BMHPairTable
    assert torch_nfft.bmh is tn.bmh
    rng = np.random.default_rng(3)
    T, n = 5, 40
    types = torch.from_numpy(lt.draw_types(rng, n, T, unused=(3,)))
    PA, PB, C6, C8, g = bt.exp6_parameters(rng, T, 0.1)
    tab = tn.BMHPairTable(_t(PA), _t(PB), _t(C6), _t(C8), types)
    assert tab.num_types == T and tab.num_points == n and tab.has_grid is True
    assert tab.types.dtype == torch.int32 and torch.equal(tab.types.long(), types)
    assert tab.c.dtype == torch.float32 and tab.c.shape == (n,) and tab.table.dtype == torch.float32 and tab.table.shape == (T, T, 4)
    assert tab.table.is_contiguous() and torch.equal(tab.table, tab.table.transpose(0, 1))
    assert np.abs(tab.grid_c.numpy() / g - 1).max() <= 1e-15  # sqrt(diag(c6)) by default
    assert torch.equal(tab.c, torch.from_numpy(tab.grid_c.numpy()[types.numpy()]).float())
    D6 = C6 - np.outer(g, g)
    for k, want in enumerate((PA, PB, D6, C8)):  # derived in float64: the cast is the only rounding
        assert np.abs(tab.table[..., k].double().numpy() - want).max() <= 2.0 ** -23 * np.abs(want).max() + 1e-13 * C6.max()
    assert np.abs(np.diagonal(tab.table[..., 2].numpy())).max() <= 1e-15 * C6.max() and np.abs(D6).max() >= 1e-3 * C6.max()
    twice = tn.BMHPairTable(_t(PA), _t(PB), _t(C6), _t(C8), types.to(torch.int32), grid_c=_t(2 * g))
    assert abs(float(twice.table[1, 1, 2]) / (C6[1, 1] - 4 * g[1] ** 2) - 1) <= 1e-6 and twice.has_grid is True
    none = tn.BMHPairTable(_t(PA), _t(PB), _t(C6), _t(C8), types, grid_c=torch.zeros(T))
    assert none.has_grid is False and not bool(none.c.any()) and torch.equal(none.table[..., 2], _t(C6).float())
    assert tn.BMHPairTable(*(_t(v[:1, :1]) for v in (PA, PB, C6, C8)), torch.zeros(3, dtype=torch.int64)).num_types == 1
    big = np.ones((32, 32))
    assert tn.BMHPairTable(_t(big), _t(big), _t(big), _t(big), torch.arange(32)).table.shape == (32, 32, 4)
    # the class methods: LAMMPS' buck and born parameters
    rho = 1.0 / PB
    buck = tn.BMHPairTable.buckingham(_t(PA), _t(rho), _t(C6), types, grid_c=torch.zeros(T))
    direct = tn.BMHPairTable(_t(PA), _t(1.0 / rho), _t(C6), torch.zeros(T, T), types, grid_c=torch.zeros(T))
    assert torch.equal(buck.table, direct.table) and not bool(buck.table[..., 3].any()) and buck.has_grid is False
    sigma = 0.05 + 0.05 * rng.random((T, T))
    sigma = 0.5 * (sigma + sigma.T)
    D = -C8  # (an attraction: LAMMPS' D is negative)
    born = tn.BMHPairTable.born(_t(PA * 1e-6), _t(rho), _t(sigma), _t(C6), _t(D), types)
    direct = tn.BMHPairTable(_t(PA * 1e-6 * np.exp(sigma / rho)), _t(1.0 / rho), _t(C6), _t(-D), types)
    assert torch.equal(born.table, direct.table) and torch.equal(born.c, direct.c) and float(born.table[..., 3].min()) > 0
    with pytest.raises(ValueError, match=r"A e\^\(sigma / rho\) at \[\d, \d\] leaves float32"):
        tn.BMHPairTable.born(_t(PA), _t(rho), _t(sigma * 40), _t(C6), _t(D), types)
    with pytest.raises(ValueError, match="rho must be positive"):
        tn.BMHPairTable.buckingham(_t(PA), _t(rho * 0), _t(C6), types)
    assert "Tosi-Fumi" in tn.BMHPairTable.born.__doc__ and "NEGATED" in tn.BMHPairTable.born.__doc__
    # refusals
    make = lambda a=PA, b=PB, c6=C6, c8=C8, t=types, **kw: tn.BMHPairTable(_t(a), _t(b), _t(c6), _t(c8), t, **kw)
    for k in range(4):
        bad = [PA.copy(), PB.copy(), C6.copy(), C8.copy()]
        bad[k][0, 1] *= 1.0 + 1e-12
        with pytest.raises(ValueError, match="symmetric"):
            make(*bad)
        bad = [PA.copy(), PB.copy(), C6.copy(), C8.copy()]
        bad[k][1, 1] = float("nan")
        with pytest.raises(ValueError, match="finite"):
            make(*bad)
        bad = [PA, PB, C6, C8]
        bad[k] = bad[k][:4, :4]
        with pytest.raises(ValueError, match=r"\[T, T\]"):
            make(*bad)
    big = np.ones((33, 33))
    with pytest.raises(ValueError, match="33 types, the limit is 32"):
        make(big, big, big, big)
    with pytest.raises(ValueError, match="0 types, the limit is 32"):
        tn.BMHPairTable(*(torch.zeros(0, 0),) * 4, types)
    with pytest.raises(ValueError, match=r"\[T, T\]"):
        make(PA[:4], PB[:4], C6[:4], C8[:4])
    with pytest.raises(ValueError, match="must be real"):
        tn.BMHPairTable(_t(PA).to(torch.complex128), _t(PB), _t(C6), _t(C8), types)
    neg = PA.copy()
    neg[1, 2] = neg[2, 1] = -0.5
    with pytest.raises(ValueError, match=r"A\[1, 2\] = -0.5 is negative"):
        make(a=neg)
    neg = PB.copy()
    neg[4, 4] = -2.0
    with pytest.raises(ValueError, match=r"B\[4, 4\] = -2 is negative"):
        make(b=neg)
    assert make(c8=-C8).num_types == T and make(a=0 * PA, b=0 * PB).num_types == T  # (a repulsive C8, no exponential: allowed)
    off = types.clone()
    off[7], off[9] = 5, -1
    with pytest.raises(ValueError, match=r"types\[7\] = 5 lies outside \[0, 5\)"):
        make(t=off)
    off[7] = 0
    with pytest.raises(ValueError, match=r"types\[9\] = -1 lies outside \[0, 5\)"):
        make(t=off)
    with pytest.raises(ValueError, match="integer"):
        make(t=types.double())
    with pytest.raises(ValueError, match="integer"):
        make(t=types.reshape(2, -1))
    neg = C6.copy()
    neg[2, 2] = -1e-9
    with pytest.raises(ValueError, match="negative diagonal"):
        make(c6=neg)
    assert make(c6=neg, grid_c=_t(g)).num_types == T  # (a grid coefficient of the caller's)
    with pytest.raises(ValueError, match=r"grid_c must be real \[T\]"):
        make(grid_c=_t(g[:4]))
    with pytest.raises(ValueError, match="grid_c must be finite"):
        make(grid_c=_t(g * float("inf")))


def test_refusals_without_gpu():
    import torch_nfft
    import torch_nfft_amd as tn
    assert "nfft_ewald_bmh_table_step" in tn.__all__ and torch_nfft.nfft_ewald_bmh_table_step is tn.nfft_ewald_bmh_table_step
    assert tn.nfft_ewald_bmh_table_step is tn.bmh.nfft_ewald_bmh_table_step
    spc = tn.EwaldSplitting(12.0, 0.25, 16, box=eb.T, device="cpu")
    spd = tn.DispersionSplitting(11.0, 0.25, 16, box=eb.T, device="cpu")
    q, pos = torch.zeros(5), torch.zeros(5, 3)
    one = torch.ones(2, 2, dtype=torch.float64)
    t5 = torch.tensor([0, 1, 1, 0, 1])
    tab = tn.BMHPairTable(one, one, one, one, t5)
    bare = tn.BMHPairTable(one, one, one, one, t5, grid_c=torch.zeros(2))
    call = tn.nfft_ewald_bmh_table_step
    ex = tn.ExclusionList([[0, 1], [3, 1]], 5, coulomb_scale=[0.0, 0.5], dispersion_scale=0.5, device="cpu")
    with pytest.raises(TypeError, match="nfft_ewald_bmh_table_step: table must be a BMHPairTable"):
        call(q, q, pos, coulomb=spc, dispersion=spd)
    with pytest.raises(TypeError, match="nfft_ewald_bmh_table_step: table must be a BMHPairTable"):
        call(q, tn.LJPairTable(one, one, t5), pos, coulomb=spc, dispersion=spd)
    with pytest.raises(ValueError, match="nfft_ewald_bmh_table_step: table holds the types of 4 points, pos has 5"):
        call(q, tn.BMHPairTable(one, one, one, one, torch.tensor([0, 1, 1, 0])), pos, coulomb=spc, dispersion=spd)
    with pytest.raises(TypeError, match="nfft_ewald_bmh_table_step: exclusions must be an ExclusionList or None"):
        call(q, tab, pos, coulomb=spc, dispersion=spd, exclusions=[[0, 1]])
    with pytest.raises(ValueError, match="nfft_ewald_bmh_table_step: exclusions lists pairs of 4 points, pos has 5"):
        call(q, tab, pos, coulomb=spc, dispersion=spd, exclusions=tn.ExclusionList([[0, 1]], 4, device="cpu"))
    with pytest.raises(TypeError, match="nfft_ewald_bmh_table_step: coulomb must be an EwaldSplitting"):
        call(q, tab, pos, coulomb=spd, dispersion=spd, exclusions=ex)
    with pytest.raises(TypeError, match="nfft_ewald_bmh_table_step: coulomb must be an EwaldSplitting"):
        call(q, bare, pos, coulomb=spd, dispersion=None)
    with pytest.raises(TypeError, match="nfft_ewald_bmh_table_step: dispersion must be a DispersionSplitting"):
        call(q, tab, pos, coulomb=spc, dispersion=spc)
    # dispersion=None puts nothing on the grid: a table that carries r^-6 there is refused, and the default grid_c does
    with pytest.raises(ValueError, match="nfft_ewald_bmh_table_step: dispersion=None needs a table with grid_c = 0"):
        call(q, tab, pos, coulomb=spc, dispersion=None)
    with pytest.raises(ValueError, match="grid_c"):
        call(q, tab, pos, coulomb=spc)  # (None is the default)
    with pytest.raises(ValueError, match="same r_cut"):
        call(q, tab, pos, coulomb=spc, dispersion=tn.DispersionSplitting(11.0, 0.2, 16, box=eb.T, device="cpu"))
    with pytest.raises(ValueError, match="same bandwidth"):
        call(q, tab, pos, coulomb=spc, dispersion=tn.DispersionSplitting(11.0, 0.25, 18, box=eb.T, device="cpu"))
    with pytest.raises(ValueError, match="same box"):
        call(q, tab, pos, coulomb=spc, dispersion=tn.DispersionSplitting(11.0, 0.25, 16, box=eb.O, device="cpu"))
    for t, d in ((tab, spd), (bare, None)):
        with pytest.raises(ValueError, match="nfft_ewald_bmh_table_step: q must be \\[n\\]: columns are not supported"):
            call(torch.zeros(5, 2), t, pos, coulomb=spc, dispersion=d)
        with pytest.raises(ValueError, match="nfft_ewald_bmh_table_step: q must be real"):
            call(q.to(torch.complex64), t, pos, coulomb=spc, dispersion=d)
        with pytest.raises(ValueError, match="one value per point"):
            call(torch.zeros(4), t, pos, coulomb=spc, dispersion=d)
        with pytest.raises(ValueError, match="must be float32"):
            call(q.double(), t, pos, coulomb=spc, dispersion=d)
        with pytest.raises(ValueError, match="nfft_ewald_bmh_table_step: .*three-dimensional"):
            call(q, t, torch.zeros(5, 2), coulomb=spc, dispersion=d)
        with pytest.raises(AssertionError, match="nfft_ewald_bmh_table_step: batch holds point-set indices and must not require grad"):
            call(q, t, pos, torch.zeros(5, requires_grad=True), coulomb=spc, dispersion=d)
        for e in (None, ex):
            with pytest.raises(RuntimeError, match="is currently only implemented for GPU tensors"):
                call(q, t, pos, coulomb=spc, dispersion=d, exclusions=e)
    with pytest.raises(ValueError, match="nfft_ewald_bmh_table_step: fractional=True needs"):
        call(q, tab, pos, coulomb=tn.EwaldSplitting(12.0, 0.25, 16, device="cpu"),
             dispersion=tn.DispersionSplitting(11.0, 0.25, 16, device="cpu"), fractional=True)
    assert "jumps by" in call.__doc__ and "turnover" in call.__doc__
    # the operator: _nfft_ewald_lj_table_near's schema under its own name
    s = str(torch.ops.torch_nfft._nfft_ewald_bmh_table_near.default._schema)
    assert s == ("torch_nfft::_nfft_ewald_bmh_table_near(Tensor pos, Tensor xs, Tensor types, Tensor table, Tensor? batch, "
                 "Tensor? row_start, Tensor? col, Tensor? weight_coulomb, Tensor? weight_lj, float[] box, float alpha_coulomb, "
                 "float alpha_dispersion, float r_cut) -> (Tensor, Tensor)")
    assert s.replace("bmh_table", "lj_table") == str(torch.ops.torch_nfft._nfft_ewald_lj_table_near.default._schema)
    lists = (ex.row_start, ex.col, ex.coulomb_weight, ex.dispersion_weight)
    for ls in (lists, (None,) * 4):
        with pytest.raises(RuntimeError, match="_nfft_ewald_bmh_table_near is currently only implemented for GPU tensors"):
            tn.ops.nfft_ewald_bmh_table_near(pos, torch.zeros(5, 2), tab.types, tab.table, None, *ls, spc.box6, 12.0, 11.0, 0.25)


def _six(A):
    A = np.asarray(A, dtype=np.float64)
    return (ctypes.c_double * 6)(A[0, 0], A[1, 0], A[1, 1], A[2, 0], A[2, 1], A[2, 2])


def test_c_abi_validation_without_gpu():
    """the refusals of nfft_hip_ewald_lj_table_near under the new entry's name, with an entry of 16 bytes: num_types outside
    [1, 32], a null table, tables at addresses 264 (refused) and 272 (accepted up to the workspace check), list pointers without
    row_start"""
    from torch_nfft_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 7 and lib.nfft_hip_abi_version() == 7  # (additions only)
    for name in ("nfft_hip_ewald_bmh_table_near_workspace_bytes", "nfft_hip_ewald_bmh_table_near"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)

    def problem(A=eb.O, **kw):
        f = dict(cells=(4, 5, 3), with_field=1, num_points=1000, num_columns=1, batch_size=1, alpha=14.0, r_cut=0.25, box=_six(A))
        f.update(kw)
        f["cells"] = (ctypes.c_int32 * 3)(*f["cells"])
        return _lib.EwaldBoxProblem(**f)

    ok = problem()
    size = lib.nfft_hip_ewald_bmh_table_near_workspace_bytes
    need = size(ctypes.byref(ok), 12.0)
    assert need == lib.nfft_hip_ewald_lj_step_near_workspace_bytes(ctypes.byref(ok), 12.0)
    for bad in (problem(cells=(5, 5, 3)), problem(cells=(2, 5, 3)), problem(with_field=2), problem(num_points=-1),
                problem(num_columns=2), problem(batch_size=0), problem(alpha=float("nan")), problem(r_cut=0.5)):
        assert size(ctypes.byref(bad), 12.0) == -1 and _lib.last_error().startswith("Input mismatch")
    for bad_alpha in (0.0, -1.0, float("inf"), float("nan")):
        assert size(ctypes.byref(ok), bad_alpha) == -1
        assert _lib.last_error() == "Input mismatch: alpha_dispersion must be positive and finite"
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(256)  # (never dereferenced: the checks come first)

    def near(q, alpha_d=12.0, T=5, entries=10, ws=null, nbytes=0, points=one, xs=one, types=one, table=one, start=one, index=one,
             row_start=one, col=one, wc=one, wl=one, f=one, out=one):
        return lib.nfft_hip_ewald_bmh_table_near(ctypes.byref(q), alpha_d, T, entries, points, xs, types, table, start, index,
                                                 row_start, col, wc, wl, f, out, ws, nbytes, null)

    unmasked = dict(entries=0, row_start=null, col=null, wc=null, wl=null)
    for kw in ({}, unmasked, dict(T=1), dict(T=32), dict(entries=0, col=null, wc=null, wl=null)):
        assert near(ok, **kw) == _lib.EWORKSPACE and _lib.last_error() == "workspace too small", kw
        assert near(ok, ws=one, nbytes=need - 1, **kw) == _lib.EWORKSPACE
    for T in (0, -1, 33, 1 << 40):
        assert near(ok, T=T) == _lib.EINVAL and _lib.last_error() == "Input mismatch: num_types must lie in [1, 32]"
    assert near(ok, table=null) == _lib.EINVAL and _lib.last_error() == "Input mismatch: table is null"
    assert near(problem(num_points=0), table=null) == _lib.EINVAL
    for address in (260, 264):
        assert near(ok, table=ctypes.c_void_p(address)) == _lib.EINVAL
        assert _lib.last_error() == "Input mismatch: table must be 16-byte aligned"
    assert near(ok, table=ctypes.c_void_p(272)) == _lib.EWORKSPACE
    for kw in (dict(col=null), dict(wc=null), dict(wl=null), dict(entries=-1), dict(entries=1 << 31), dict(row_start=null),
               dict(unmasked, entries=3), dict(unmasked, col=one), dict(unmasked, wc=one), dict(unmasked, wl=one)):
        assert near(ok, **kw) == _lib.EINVAL and _lib.last_error().startswith("Input mismatch"), kw
    assert near(ok, **dict(unmasked, col=one)) == _lib.EINVAL and _lib.last_error() == "Input mismatch: a list without row_start"
    for base in ({}, unmasked):
        for kw in (dict(out=null), dict(points=null), dict(xs=null), dict(types=null), dict(start=null), dict(index=null),
                   dict(f=null), dict(alpha_d=float("nan"))):
            assert near(ok, **base, **kw) == _lib.EINVAL and _lib.last_error().startswith("Input mismatch"), kw
    assert near(problem(cells=(2, 5, 3))) == _lib.EINVAL and near(problem(r_cut=0.5)) == _lib.EINVAL


def test_kernel_resource_usage():
    """both instantiations of step_near_kernel with BmhTableLaw: no scratch and no spills, the 8320 bytes of static LDS of the walks of 7r,
    7s and 7t (the table's 16 T (T | 1) bytes are dynamic), and no name that the resource gates of those sections would take
    for their kernels (the VGPR and SGPR figures are recorded in DESIGN.md section 7u, not gated)"""
    from resource_usage import resource_usage
    usage = resource_usage("ewald_bmh_table.hip")
    seen = set()
    for name, u in sorted(usage.items()):
        assert not re.search(r"LjProductLaw|LjTableLaw|lj_excl_list_kernel", name)
        m = re.search(r"step_near_kernelI\w*?BmhTableLawELb(\d)E", name)
        if not m:
            continue
        seen.add(int(m.group(1)))
        print("step_near_kernel<BmhTableLaw, %s>" % m.group(1), "VGPRs %d SGPRs %d occupancy %d LDS %d" % (u["VGPRs"], u["TotalSGPRs"], u["Occupancy"], u["LDS Size"]))
        assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
        assert u["LDS Size"] == 8320
    assert seen == {0, 1}
