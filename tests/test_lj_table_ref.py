"""CPU tests of the Lennard-Jones + Coulomb step with per-type-pair parameters: the float64 restatement
tests/lj_table_ref.py against the restatements of sections 7r and 7s (a geometric table), against an independent composition
of converged sums (a Lorentz-Berthelot table), against central differences of that energy and against four wrong formulas;
LJPairTable's refusals and constructors; the refusals of nfft_ewald_lj_table_step before any device work, the operator schema,
the C ABI's validation and the resource figures of csrc/ewald_lj_table.hip."""
import ctypes
import re

import numpy as np
import pytest
import torch

import ewald_box_ref as eb
import lj_excl_ref as le
import lj_step_ref as lj
import lj_table_ref as lt
from conftest import rel_l2
from ewald_virial_ref import rel_fro

# The split and its truncation factors are those of tests/test_lj_step_ref.py: erfc(alpha_C r_c) = 3.5e-8 and 2e-8 at the
# grid's edge for the Coulomb sum, 3.9e-6 at a = alpha_D r_c = 4.2 and 2.4e-8 for the dispersion sum of c.  The table's own
# terms are summed directly within r_c on both sides and carry no truncation: the restatement stands within the largest
# factor, 3.9e-6, of the converged composition; 1e-5 leaves a factor 2.5.
SPLIT = (13.0, 14.0, 0.3, 40)  # alpha_C, alpha_D, r_c, N
TRUNCATION = 1e-5
LARGEST_GPU_TOLERANCE = 1e-4
D_MIN = 0.14
N_FREE, N_BONDED, TYPES = 30, 44, 3


@pytest.fixture(scope="module")
def system():
    """30 points in the triclinic box T, no two closer than D_MIN, three types with sigma = 0.8, 0.5 .. 0.8 and 0.5 D_MIN;
    partial charges of 0.4, so that the Lennard-Jones terms are no small share of the force"""
    rng = np.random.default_rng(31)
    s = lj.separated_points(rng, N_FREE, eb.T, D_MIN).astype(np.float32).astype(np.float64)
    assert lj.dr.min_separation(s, eb.T) >= D_MIN * (1 - 1e-6)
    q = 0.4 * rng.standard_normal(N_FREE)
    q -= q.mean()
    types = lt.draw_types(rng, N_FREE, TYPES)
    sigma, eps = lt.type_parameters(rng, TYPES, D_MIN)
    tab = lt.lorentz_berthelot(sigma, eps)
    lt.check_types(tab, types, D_MIN)
    return s, q, types, tab, (sigma, eps)


@pytest.fixture(scope="module")
def bonded():
    """44 points of lj_excl_ref.bonded_points in T with three types on top"""
    rng = np.random.default_rng(33)
    s, types, tab, pairs, sc, sl, info = lt.typed_bonded(rng, N_BONDED, TYPES, eb.T, SPLIT[2])
    q = rng.standard_normal(N_BONDED)
    q -= q.mean()
    return s.astype(np.float64), q, types, tab, pairs, sc, sl, info


def _errors(got, want, scale_lj=None):
    F, UC, ULJ, W = got
    rF, rUC, rULJ, rW = want
    scale_lj = abs(rULJ[0]) if scale_lj is None else scale_lj
    return {"F": rel_l2(F, rF), "U_C": abs(UC[0] / rUC[0] - 1), "U_LJ": abs(ULJ[0] - rULJ[0]) / scale_lj, "W": rel_fro(W, rW)}


def test_geometric_table_is_the_step_of_7r_and_7s(system, bonded):
    """with sigma_ij = sqrt(sigma_i sigma_j) the grid's product is the pair's C6 and C12 = a_i a_j: lj_step_ref and lj_excl_ref"""
    s, q, types, _, (sigma, eps) = system
    tab = lt.geometric(sigma, eps)
    assert not (tab[0] - np.outer(tab[2], tab[2])).any()
    c, a = (v[types] for v in lj.lj_coefficients(sigma, eps))
    want = lj.exact_lj_step(q, c, a, s, eb.T, None, *SPLIT)
    e = _errors(lt.exact_lj_table_step(q, tab, types, s, eb.T, None, *SPLIT), want)
    print("geometric table vs lj_step_ref: %s" % " ".join("%s %.3e" % kv for kv in sorted(e.items())))
    assert max(e.values()) <= 1e-12
    s, q, types, _, pairs, sc, sl, info = bonded
    sigma, eps = lt.type_parameters(np.random.default_rng(2), TYPES, info["d_min"])
    tab = lt.geometric(sigma, eps)
    c, a = (v[types] for v in lj.lj_coefficients(sigma, eps))
    batch = np.concatenate([np.zeros(N_BONDED, np.int64)])
    for b in (None, batch):
        want = le.exact_lj_excl_step(q, c, a, s, eb.T, b, pairs, sc, sl, *SPLIT)
        e = _errors(lt.exact_lj_table_step(q, tab, types, s, eb.T, b, *SPLIT, pairs, sc, sl), want)
        print("geometric table vs lj_excl_ref: %s" % " ".join("%s %.3e" % kv for kv in sorted(e.items())))
        assert max(e.values()) <= 1e-12


def test_lorentz_berthelot_against_the_converged_composition(system):
    """against the converged Coulomb sum, the brute-force c_i c_j / r^6 lattice sum over every image within R = 14 and the exact
    dC6 and C12 terms summed directly within r_c; Newton's third law; the trace identity"""
    s, q, types, tab, _ = system
    got = lt.exact_lj_table_step(q, tab, types, s, eb.T, None, *SPLIT)
    cF, cUC, cULJ, cW, (_, UD, UR, UX) = lt.converged_lj_table_step(q, tab, types, s, eb.T, SPLIT[2], R=14.0)
    assert abs(UX[0]) > 1e-3 * abs(UD[0])  # (the table's correction is no rounding error of the sum)
    e = _errors(got, (cF, cUC, cULJ, cW), abs(UD[0]) + abs(UR[0]) + abs(UX[0]))
    print("restatement vs converged composition: %s" % " ".join("%s %.3e" % kv for kv in sorted(e.items())))
    assert max(e.values()) <= TRUNCATION
    F, _, _, W = got
    assert np.abs(F.sum(0)).max() <= 1e-9 * np.abs(F).sum() and np.abs(cF.sum(0)).max() <= 1e-9 * np.abs(cF).sum()
    assert np.abs(W - W.transpose(0, 2, 1)).max() <= 1e-12 * np.abs(W).max()
    # tr W = U_C - 6 U_D + 12 U_R - 6 U_delta with U_delta = 1/2 sum dC6 / r^6, which the energy holds with a minus sign as it
    # holds U_D: every term of degree -k in the lengths adds k times its signed energy
    want = cUC[0] - 6.0 * UD[0] + 12.0 * UR[0] - 6.0 * UX[0]
    size = abs(cUC[0]) + 6.0 * abs(UD[0]) + 12.0 * abs(UR[0]) + 6.0 * abs(UX[0])
    print("tr W %.9g, U_C - 6 U_D + 12 U_R - 6 U_delta %.9g (U_delta %.6g)" % (np.trace(cW[0]), want, UX[0]))
    assert abs(np.trace(cW[0]) - want) <= 1e-7 * size
    assert abs(np.trace(W[0]) - want) <= 3.0 * TRUNCATION * size
    assert abs(6.0 * UX[0]) >= 1e3 * 1e-7 * size  # (the identity would notice the term's sign)


def test_with_exclusions_against_the_converged_composition(bonded):
    s, q, types, tab, pairs, sc, sl, info = bonded
    got = lt.exact_lj_table_step(q, tab, types, s, eb.T, None, *SPLIT, pairs, sc, sl)
    # (each side takes the r = 0 constants of its own alphas; converged_lj_excl_step's defaults are those of its sums)
    cF, cUC, cULJ, cW, (_, UD, UR, UX) = lt.converged_lj_table_step(q, tab, types, s, eb.T, SPLIT[2], pairs, sc, sl)
    e = _errors(got, (cF, cUC, cULJ, cW), abs(UD[0]) + abs(UR[0]) + abs(UX[0]))
    print("with exclusions, restatement vs converged composition: %s" % " ".join("%s %.3e" % kv for kv in sorted(e.items())))
    assert max(e.values()) <= TRUNCATION
    want = cUC[0] - 6.0 * UD[0] + 12.0 * UR[0] - 6.0 * UX[0]
    size = abs(cUC[0]) + 6.0 * abs(UD[0]) + 12.0 * abs(UR[0]) + 6.0 * abs(UX[0])
    assert abs(np.trace(cW[0]) - want) <= 1e-6 * size
    assert np.abs(got[0].sum(0)).max() <= 1e-9 * np.abs(got[0]).sum()


def test_force_and_virial_are_derivatives_of_the_energy(system):
    """F = -dU/dx and W = -dU/d eps by central differences (h = 1e-5) of the converged energy, bounds as in
    tests/test_lj_step_ref.py: truncation h^2 |U'''| / 6 with |U''' / U'| <= 14 * 15 / d_min^2 = 1.1e4, 2e-7 relative; 1e-5 leaves a
    factor 50.  No pair may cross r_c on the way: both table terms jump there."""
    s, q, types, tab, _ = system
    A, r_c, h = eb.T, SPLIT[2], 1e-5
    ds = s[:, None, :] - s[None, :, :]
    r = np.linalg.norm((ds - np.rint(ds)) @ A, axis=-1)
    assert np.abs(r - r_c).min() > 10 * h  # (a point moves by h, a strained separation by h r)
    F, _, _, W, _ = lt.converged_lj_table_step(q, tab, types, s, A, r_c)
    inv = np.linalg.inv(A)
    energy = lambda s_, A_: lt.converged_energy(q, tab, types, s_, A_, r_c)
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


@pytest.mark.parametrize("mutant", ["c6_for_delta", "delta_sign", "types_permuted", "delta_unscaled"])
def test_mutants_are_far_off(system, bonded, mutant):
    """each wrong formula is off by at least 100 x the largest tolerance that a GPU test may have"""
    gate = 100 * LARGEST_GPU_TOLERANCE
    if mutant == "delta_unscaled":  # (needs a list: the 1-4 pairs keep half their Lennard-Jones term)
        s, q, types, tab, pairs, sc, sl, _ = bonded
        args = (q, tab, types, s, eb.T, None, *SPLIT, pairs, sc, sl)
    else:
        s, q, types, tab, _ = system
        args = (q, tab, types, s, eb.T, None, *SPLIT)
    F, UC, ULJ, W = lt.exact_lj_table_step(*args)
    Fm, UCm, ULJm, Wm = lt.exact_lj_table_step(*args, mutant=mutant)
    e = rel_l2(Fm, F), abs(ULJm[0] - ULJ[0]) / abs(ULJ[0]), rel_fro(Wm, W)
    print("mutant %-16s relative error of F %.3e, U_LJ %.3e, W %.3e" % ((mutant,) + e))
    assert UCm[0] == UC[0]
    if mutant == "types_permuted":
        # (the same entries dealt out to other pairs: the energy, one total over all pairs, moves less than a point's force)
        assert e[0] >= gate and e[2] >= gate and e[1] >= 10 * LARGEST_GPU_TOLERANCE
    else:
        assert min(e) >= gate


def _t(a, dtype=torch.float64):
    return torch.as_tensor(np.asarray(a), dtype=dtype)


def test_pair_table_constructors_and_refusals():
    import torch_nfft
    import torch_nfft_amd as tn
    assert "LJPairTable" in tn.__all__ and torch_nfft.LJPairTable is tn.LJPairTable is tn.lj.LJPairTable
    rng = np.random.default_rng(3)
    T, n = 5, 40
    sigma, eps = 0.1 + 0.1 * rng.random(T), 0.5 + rng.random(T)
    types = torch.from_numpy(lt.draw_types(rng, n, T, unused=(3,)))
    for make, ref in ((tn.LJPairTable.lorentz_berthelot, lt.lorentz_berthelot), (tn.LJPairTable.geometric, lt.geometric)):
        C6, C12, g = ref(sigma, eps)
        tab = make(_t(sigma), _t(eps), types)
        assert tab.num_types == T and tab.num_points == n
        assert tab.types.dtype == torch.int32 and torch.equal(tab.types.long(), types)
        assert tab.c.dtype == torch.float32 and tab.c.shape == (n,) and tab.table.dtype == torch.float32 and tab.table.shape == (T, T, 2)
        assert torch.equal(tab.table, tab.table.transpose(0, 1))
        # against the closed forms: the cast is the only rounding beyond 1e-13
        assert np.abs(tab.grid_c.numpy() / g - 1).max() <= 1e-13
        assert torch.equal(tab.c, torch.from_numpy(tab.grid_c.numpy()[types.numpy()]).float())
        assert np.abs(tab.table[..., 0].double().numpy() / C12 - 1).max() <= 2.0 ** -23
        D6 = C6 - np.outer(g, g)
        assert np.abs(tab.table[..., 1].double().numpy() - D6).max() <= 2.0 ** -23 * np.abs(D6).max() + 1e-13 * C6.max()
        if ref is lt.geometric:
            assert np.abs(tab.table[..., 1].numpy()).max() <= 1e-13 * C6.max()  # dC6 = 0 up to the rounding of float64
        else:
            assert np.abs(D6).max() >= 1e-3 * C6.max()
    # the plain constructor: grid_c defaults to sqrt(diag(c6)); NBFIX is an edited entry
    C6, C12, g = lt.lorentz_berthelot(sigma, eps)
    C6[0, 2] = C6[2, 0] = 1.25 * C6[0, 2]
    tab = tn.LJPairTable(_t(C6), _t(C12), types)
    assert np.abs(tab.grid_c.numpy() / np.sqrt(np.diag(C6)) - 1).max() <= 1e-15
    assert abs(float(tab.table[0, 2, 1]) / (C6[0, 2] - g[0] * g[2]) - 1) <= 1e-6
    assert np.abs(np.diagonal(tab.table[..., 1].numpy())).max() <= 1e-15 * C6.max()
    tab = tn.LJPairTable(_t(C6), _t(C12), types.to(torch.int32), grid_c=_t(2 * g))
    assert abs(float(tab.table[1, 1, 1]) / (C6[1, 1] - 4 * g[1] ** 2) - 1) <= 1e-6
    assert tn.LJPairTable(_t(C6[:1, :1]), _t(C12[:1, :1]), torch.zeros(3, dtype=torch.int64)).num_types == 1
    big = np.ones((32, 32))
    assert tn.LJPairTable(_t(big), _t(big), torch.arange(32)).table.shape == (32, 32, 2)
    # refusals
    bad = C6.copy()
    bad[0, 1] *= 1.0 + 1e-12
    with pytest.raises(ValueError, match="symmetric"):
        tn.LJPairTable(_t(bad), _t(C12), types)
    with pytest.raises(ValueError, match="symmetric"):
        tn.LJPairTable(_t(C6), _t(bad), types)
    big = np.ones((33, 33))
    with pytest.raises(ValueError, match="33 types, the limit is 32"):
        tn.LJPairTable(_t(big), _t(big), types)
    with pytest.raises(ValueError, match="0 types, the limit is 32"):
        tn.LJPairTable(torch.zeros(0, 0), torch.zeros(0, 0), types)
    with pytest.raises(ValueError, match=r"\[T, T\]"):
        tn.LJPairTable(_t(C6[:4]), _t(C12[:4]), types)
    with pytest.raises(ValueError, match=r"\[T, T\]"):
        tn.LJPairTable(_t(C6), _t(C12[:4, :4]), types)
    with pytest.raises(ValueError, match="must be real"):
        tn.LJPairTable(_t(C6).to(torch.complex128), _t(C12), types)
    nan = C12.copy()
    nan[1, 1] = float("nan")
    with pytest.raises(ValueError, match="finite"):
        tn.LJPairTable(_t(C6), _t(nan), types)
    off = types.clone()
    off[7], off[9] = 5, -1
    with pytest.raises(ValueError, match=r"types\[7\] = 5 lies outside \[0, 5\)"):
        tn.LJPairTable(_t(C6), _t(C12), off)
    off[7] = 0
    with pytest.raises(ValueError, match=r"types\[9\] = -1 lies outside \[0, 5\)"):
        tn.LJPairTable(_t(C6), _t(C12), off)
    with pytest.raises(ValueError, match="integer"):
        tn.LJPairTable(_t(C6), _t(C12), types.double())
    with pytest.raises(ValueError, match="integer"):
        tn.LJPairTable(_t(C6), _t(C12), types.reshape(2, -1))
    neg = C6.copy()
    neg[2, 2] = -1e-9
    with pytest.raises(ValueError, match="negative diagonal"):
        tn.LJPairTable(_t(neg), _t(C12), types)
    assert tn.LJPairTable(_t(neg), _t(C12), types, grid_c=_t(g)).num_types == T  # (a grid coefficient of the caller's)
    with pytest.raises(ValueError, match=r"grid_c must be real \[T\]"):
        tn.LJPairTable(_t(C6), _t(C12), types, grid_c=_t(g[:4]))
    with pytest.raises(ValueError, match="sigma and epsilon"):
        tn.LJPairTable.lorentz_berthelot(_t(sigma), _t(eps[:4]), types)
    with pytest.raises(ValueError, match="epsilon must not be negative"):
        tn.LJPairTable.geometric(_t(sigma), _t(-eps), types)
    assert "NBFIX" in tn.LJPairTable.__doc__


def test_refusals_without_gpu():
    import torch_nfft
    import torch_nfft_amd as tn
    assert "nfft_ewald_lj_table_step" in tn.__all__ and torch_nfft.nfft_ewald_lj_table_step is tn.nfft_ewald_lj_table_step
    assert tn.nfft_ewald_lj_table_step is tn.lj.nfft_ewald_lj_table_step
    spc = tn.EwaldSplitting(12.0, 0.25, 16, box=eb.T, device="cpu")
    spd = tn.DispersionSplitting(11.0, 0.25, 16, box=eb.T, device="cpu")
    q, pos = torch.zeros(5), torch.zeros(5, 3)
    one = torch.ones(2, 2, dtype=torch.float64)
    tab = tn.LJPairTable(one, one, torch.tensor([0, 1, 1, 0, 1]))
    call = tn.nfft_ewald_lj_table_step
    ex = tn.ExclusionList([[0, 1], [3, 1]], 5, coulomb_scale=[0.0, 0.5], dispersion_scale=0.5, device="cpu")
    with pytest.raises(TypeError, match="nfft_ewald_lj_table_step: table must be an LJPairTable"):
        call(q, q, pos, coulomb=spc, dispersion=spd)
    with pytest.raises(ValueError, match="nfft_ewald_lj_table_step: table holds the types of 4 points, pos has 5"):
        call(q, tn.LJPairTable(one, one, torch.tensor([0, 1, 1, 0])), pos, coulomb=spc, dispersion=spd)
    with pytest.raises(TypeError, match="nfft_ewald_lj_table_step: exclusions must be an ExclusionList or None"):
        call(q, tab, pos, coulomb=spc, dispersion=spd, exclusions=[[0, 1]])
    with pytest.raises(ValueError, match="nfft_ewald_lj_table_step: exclusions lists pairs of 4 points, pos has 5"):
        call(q, tab, pos, coulomb=spc, dispersion=spd, exclusions=tn.ExclusionList([[0, 1]], 4, device="cpu"))
    with pytest.raises(TypeError, match="nfft_ewald_lj_table_step: coulomb must be an EwaldSplitting"):
        call(q, tab, pos, coulomb=spd, dispersion=spd, exclusions=ex)
    with pytest.raises(TypeError, match="nfft_ewald_lj_table_step: dispersion must be a DispersionSplitting"):
        call(q, tab, pos, coulomb=spc, dispersion=spc)
    with pytest.raises(ValueError, match="same r_cut"):
        call(q, tab, pos, coulomb=spc, dispersion=tn.DispersionSplitting(11.0, 0.2, 16, box=eb.T, device="cpu"))
    with pytest.raises(ValueError, match="same bandwidth"):
        call(q, tab, pos, coulomb=spc, dispersion=tn.DispersionSplitting(11.0, 0.25, 18, box=eb.T, device="cpu"))
    with pytest.raises(ValueError, match="same box"):
        call(q, tab, pos, coulomb=spc, dispersion=tn.DispersionSplitting(11.0, 0.25, 16, box=eb.O, device="cpu"))
    with pytest.raises(ValueError, match="nfft_ewald_lj_table_step: q must be \\[n\\]: columns are not supported"):
        call(torch.zeros(5, 2), tab, pos, coulomb=spc, dispersion=spd)
    with pytest.raises(ValueError, match="nfft_ewald_lj_table_step: q must be real"):
        call(q.to(torch.complex64), tab, pos, coulomb=spc, dispersion=spd)
    with pytest.raises(ValueError, match="one value per point"):
        call(torch.zeros(4), tab, pos, coulomb=spc, dispersion=spd)
    with pytest.raises(ValueError, match="must be float32"):
        call(q.double(), tab, pos, coulomb=spc, dispersion=spd)
    with pytest.raises(ValueError, match="nfft_ewald_lj_table_step: .*three-dimensional"):
        call(q, tab, torch.zeros(5, 2), coulomb=spc, dispersion=spd)
    with pytest.raises(ValueError, match="nfft_ewald_lj_table_step: fractional=True needs"):
        call(q, tab, pos, coulomb=tn.EwaldSplitting(12.0, 0.25, 16, device="cpu"),
             dispersion=tn.DispersionSplitting(11.0, 0.25, 16, device="cpu"), fractional=True)
    with pytest.raises(AssertionError, match="nfft_ewald_lj_table_step: batch holds point-set indices and must not require grad"):
        call(q, tab, pos, torch.zeros(5, requires_grad=True), coulomb=spc, dispersion=spd)
    for e in (None, ex):
        with pytest.raises(RuntimeError, match="is currently only implemented for GPU tensors"):
            call(q, tab, pos, coulomb=spc, dispersion=spd, exclusions=e)
    # the siblings keep their signatures
    with pytest.raises(TypeError):
        tn.nfft_ewald_lj_step(q, q, q, pos, coulomb=spc, dispersion=spd, exclusions=None)
    with pytest.raises(TypeError):
        tn.nfft_ewald_lj_excl_step(q, tab, pos, coulomb=spc, dispersion=spd)
    assert "jumps by" in call.__doc__
    s = str(torch.ops.torch_nfft._nfft_ewald_lj_table_near.default._schema)
    assert s == ("torch_nfft::_nfft_ewald_lj_table_near(Tensor pos, Tensor xs, Tensor types, Tensor table, Tensor? batch, "
                 "Tensor? row_start, Tensor? col, Tensor? weight_coulomb, Tensor? weight_lj, float[] box, float alpha_coulomb, "
                 "float alpha_dispersion, float r_cut) -> (Tensor, Tensor)")
    lists = (ex.row_start, ex.col, ex.coulomb_weight, ex.dispersion_weight)
    for ls in (lists, (None,) * 4):
        with pytest.raises(RuntimeError, match="_nfft_ewald_lj_table_near is currently only implemented for GPU tensors"):
            tn.ops.nfft_ewald_lj_table_near(pos, torch.zeros(5, 2), tab.types, tab.table, None, *ls, spc.box6, 12.0, 11.0, 0.25)


def _six(A):
    A = np.asarray(A, dtype=np.float64)
    return (ctypes.c_double * 6)(A[0, 0], A[1, 0], A[1, 1], A[2, 0], A[2, 1], A[2, 2])


def test_c_abi_validation_without_gpu():
    """the refusals of nfft_hip_ewald_lj_excl_near, and the table's own: num_types outside [1, 32], a null or misaligned table, list
    pointers without row_start"""
    from torch_nfft_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 7 and lib.nfft_hip_abi_version() == 7  # (additions only)
    for name in ("nfft_hip_ewald_lj_table_near_workspace_bytes", "nfft_hip_ewald_lj_table_near"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)

    def problem(A=eb.O, **kw):
        f = dict(cells=(4, 5, 3), with_field=1, num_points=1000, num_columns=1, batch_size=1, alpha=14.0, r_cut=0.25, box=_six(A))
        f.update(kw)
        f["cells"] = (ctypes.c_int32 * 3)(*f["cells"])
        return _lib.EwaldBoxProblem(**f)

    ok = problem()
    size = lib.nfft_hip_ewald_lj_table_near_workspace_bytes
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
        return lib.nfft_hip_ewald_lj_table_near(ctypes.byref(q), alpha_d, T, entries, points, xs, types, table, start, index,
                                                row_start, col, wc, wl, f, out, ws, nbytes, null)

    unmasked = dict(entries=0, row_start=null, col=null, wc=null, wl=null)
    for kw in ({}, unmasked, dict(T=1), dict(T=32), dict(entries=0, col=null, wc=null, wl=null)):
        assert near(ok, **kw) == _lib.EWORKSPACE and _lib.last_error() == "workspace too small", kw
        assert near(ok, ws=one, nbytes=need - 1, **kw) == _lib.EWORKSPACE
    for T in (0, -1, 33, 1 << 40):
        assert near(ok, T=T) == _lib.EINVAL and _lib.last_error() == "Input mismatch: num_types must lie in [1, 32]"
    assert near(ok, table=null) == _lib.EINVAL and _lib.last_error() == "Input mismatch: table is null"
    assert near(problem(num_points=0), table=null) == _lib.EINVAL
    assert near(ok, table=ctypes.c_void_p(260)) == _lib.EINVAL and _lib.last_error() == "Input mismatch: table must be 8-byte aligned"
    assert near(ok, table=ctypes.c_void_p(264)) == _lib.EWORKSPACE
    for kw in (dict(col=null), dict(wc=null), dict(wl=null), dict(entries=-1), dict(entries=1 << 31), dict(row_start=null),
               dict(unmasked, entries=3), dict(unmasked, col=one), dict(unmasked, wc=one), dict(unmasked, wl=one)):
        assert near(ok, **kw) == _lib.EINVAL and _lib.last_error().startswith("Input mismatch"), kw
    for base in ({}, unmasked):
        for kw in (dict(out=null), dict(points=null), dict(xs=null), dict(types=null), dict(start=null), dict(index=null),
                   dict(f=null), dict(alpha_d=float("nan"))):
            assert near(ok, **base, **kw) == _lib.EINVAL and _lib.last_error().startswith("Input mismatch"), kw
    assert near(problem(cells=(2, 5, 3))) == _lib.EINVAL and near(problem(r_cut=0.5)) == _lib.EINVAL


def test_kernel_resource_usage():
    """both instantiations of step_near_kernel with LjTableLaw: no scratch and no spills, the 8320 bytes of static LDS of the walks of 7r
    and 7s (the table's 8 T (T | 1) bytes are dynamic), and no name that the resource gates of those sections would take for
    their kernels (the VGPR and SGPR figures are recorded in DESIGN.md section 7t, not gated)"""
    from resource_usage import resource_usage
    usage = resource_usage("ewald_lj_table.hip")
    seen = set()
    for name, u in sorted(usage.items()):
        assert not re.search(r"LjProductLaw|BmhTableLaw|lj_excl_list_kernel", name)
        m = re.search(r"step_near_kernelI\w*?LjTableLawELb(\d)E", name)
        if not m:
            continue
        seen.add(int(m.group(1)))
        print("step_near_kernel<LjTableLaw, %s>" % m.group(1), "VGPRs %d SGPRs %d occupancy %d LDS %d" % (u["VGPRs"], u["TotalSGPRs"], u["Occupancy"], u["LDS Size"]))
        assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
        assert u["LDS Size"] == 8320
    assert seen == {0, 1}
