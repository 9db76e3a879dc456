"""CPU tests of the Lennard-Jones + Coulomb step: the resource figures of csrc/ewald_lj_step.hip, the
refusals of nfft_ewald_lj_step before any device work, the C ABI's validation, lj_coefficients, and the float64 restatement
tests/lj_step_ref.py -- a composition of the committed restatements plus the r^-12 pair terms -- against brute-force lattice
sums, against central differences of the energy, against itself and against three wrong formulas."""
import ctypes
import re

import numpy as np
import pytest
import torch

import ewald_box_ref as eb
import lj_step_ref as lj
from conftest import rel_l2
from ewald_virial_ref import rel_fro


def test_kernel_resource_usage():
    """the spectral kernel and both instantiations of step_near_kernel with the product law, the unmasked walk and the masked
    one of section 7s: no scratch and no spills (the library's own flags; the VGPR, SGPR and LDS figures are recorded in
    DESIGN.md sections 7r and 7v, not gated)"""
    from resource_usage import resource_usage
    usage = resource_usage("ewald_lj_step.hip")
    seen = set()
    for name, u in sorted(usage.items()):
        m = re.search(r"step_near_kernelI\w*?(LjProductLaw)ELb(\d)E|(lj_step_spectral_kernel)", name)
        if not m:
            continue
        key = (m.group(1), int(m.group(2))) if m.group(1) else (m.group(3),)
        seen.add(key)
        print(key, "VGPRs %d SGPRs %d occupancy %d LDS %d" % (u["VGPRs"], u["TotalSGPRs"], u["Occupancy"], u["LDS Size"]))
        assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (key, u)
    assert seen == {("LjProductLaw", 0), ("LjProductLaw", 1), ("lj_step_spectral_kernel",)}


def test_lj_coefficients():
    import torch_nfft_amd as tn
    rng = np.random.default_rng(5)
    sigma, eps = rng.random(40) + 0.5, rng.random(40) + 0.1
    c, a = tn.lj_coefficients(torch.from_numpy(sigma), torch.from_numpy(eps))
    assert c.dtype == torch.float64 and c.shape == (40,) and a.shape == (40,)
    c, a = c.numpy(), a.numpy()
    rc, ra = lj.lj_coefficients(sigma, eps)
    assert np.abs(c / rc - 1).max() <= 1e-14 and np.abs(a / ra - 1).max() <= 1e-14
    # the products are the pair coefficients of the geometric (OPLS) rule, the diagonal those of each species
    eij, sij = np.sqrt(eps[:, None] * eps[None, :]), np.sqrt(sigma[:, None] * sigma[None, :])
    assert np.abs(np.outer(c, c) / (4 * eij * sij ** 6) - 1).max() <= 1e-13
    assert np.abs(np.outer(a, a) / (4 * eij * sij ** 12) - 1).max() <= 1e-13
    assert np.abs(c * c / (4 * eps * sigma ** 6) - 1).max() <= 1e-13 and np.abs(a * a / (4 * eps * sigma ** 12) - 1).max() <= 1e-13
    c32, a32 = tn.lj_coefficients(torch.tensor([0.3], dtype=torch.float32), torch.tensor([2.0], dtype=torch.float32))
    assert c32.dtype == torch.float32 and a32.dtype == torch.float32


def test_refusals_without_gpu():
    import torch_nfft
    import torch_nfft_amd as tn
    for name in ("nfft_ewald_lj_step", "lj_coefficients"):
        assert name in tn.__all__ and getattr(torch_nfft, name) is getattr(tn, name)
    assert torch_nfft.lj is tn.lj
    spc = tn.EwaldSplitting(12.0, 0.25, 16, box=eb.T, device="cpu")
    spd = tn.DispersionSplitting(11.0, 0.25, 16, box=eb.T, device="cpu")
    q, pos = torch.zeros(5), torch.zeros(5, 3)
    call = tn.nfft_ewald_lj_step
    with pytest.raises(TypeError, match="nfft_ewald_lj_step: coulomb must be an EwaldSplitting"):
        call(q, q, q, pos, coulomb=spd, dispersion=spd)
    with pytest.raises(TypeError, match="nfft_ewald_lj_step: coulomb must be an EwaldSplitting"):
        call(q, q, q, pos, dispersion=spd)
    with pytest.raises(TypeError, match="nfft_ewald_lj_step: dispersion must be a DispersionSplitting"):
        call(q, q, q, pos, coulomb=spc, dispersion=spc)
    with pytest.raises(TypeError):  # (no exclusions= keyword)
        call(q, q, q, pos, coulomb=spc, dispersion=spd, exclusions=None)
    with pytest.raises(ValueError, match="same r_cut"):
        call(q, q, q, pos, coulomb=spc, dispersion=tn.DispersionSplitting(11.0, 0.2, 16, box=eb.T, device="cpu"))
    with pytest.raises(ValueError, match="same bandwidth"):
        call(q, q, q, pos, coulomb=spc, dispersion=tn.DispersionSplitting(11.0, 0.25, 18, box=eb.T, device="cpu"))
    with pytest.raises(ValueError, match="same box"):
        call(q, q, q, pos, coulomb=spc, dispersion=tn.DispersionSplitting(11.0, 0.25, 16, box=eb.O, device="cpu"))
    with pytest.raises(ValueError, match="same box"):
        call(q, q, q, pos, coulomb=spc, dispersion=tn.DispersionSplitting(11.0, 0.25, 16, device="cpu"))
    for k in range(3):
        v = [q, q, q]
        v[k] = torch.zeros(5, 2)
        with pytest.raises(ValueError, match="nfft_ewald_lj_step: %s must be \\[n\\]: columns are not supported" % "qca"[k]):
            call(*v, pos, coulomb=spc, dispersion=spd)
        v[k] = q.to(torch.complex64)
        with pytest.raises(ValueError, match="nfft_ewald_lj_step: %s must be real" % "qca"[k]):
            call(*v, pos, coulomb=spc, dispersion=spd)
        v[k] = torch.zeros(4)
        with pytest.raises(ValueError, match="one value per point"):
            call(*v, pos, coulomb=spc, dispersion=spd)
        v[k] = q.double()
        with pytest.raises(ValueError, match="must be float32"):
            call(*v, pos, coulomb=spc, dispersion=spd)
    with pytest.raises(ValueError, match="nfft_ewald_lj_step: .*three-dimensional"):
        call(q, q, q, torch.zeros(5, 2), coulomb=spc, dispersion=spd)
    with pytest.raises(ValueError, match="nfft_ewald_lj_step: fractional=True needs"):
        call(q, q, q, pos, coulomb=tn.EwaldSplitting(12.0, 0.25, 16, device="cpu"),
             dispersion=tn.DispersionSplitting(11.0, 0.25, 16, device="cpu"), fractional=True)
    with pytest.raises(AssertionError, match="nfft_ewald_lj_step: batch holds point-set indices and must not require grad"):
        call(q, q, q, pos, torch.zeros(5, requires_grad=True), coulomb=spc, dispersion=spd)
    with pytest.raises(RuntimeError, match="is currently only implemented for GPU tensors"):
        call(q, None, None, pos, coulomb=spc, dispersion=spd)
    s = str(torch.ops.torch_nfft._nfft_ewald_lj_step_near.default._schema)
    assert s == ("torch_nfft::_nfft_ewald_lj_step_near(Tensor pos, Tensor xs, Tensor? batch, float[] box, float alpha_coulomb, "
                 "float alpha_dispersion, float r_cut) -> (Tensor, Tensor)")
    s = str(torch.ops.torch_nfft._nfft_ewald_lj_step_spectral.default._schema)
    assert s == ("torch_nfft::_nfft_ewald_lj_step_spectral(Tensor band, Tensor coeffs_coulomb, Tensor coeffs_dispersion, "
                 "Tensor strain_dispersion, float[] box, float alpha_coulomb) -> (Tensor, Tensor)")
    with pytest.raises(RuntimeError, match="_nfft_ewald_lj_step_near is currently only implemented for GPU tensors"):
        tn.ops.nfft_ewald_lj_step_near(pos, torch.zeros(5, 3), None, spc.box6, 12.0, 11.0, 0.25)
    with pytest.raises(RuntimeError, match="_nfft_ewald_lj_step_spectral is currently only implemented for GPU tensors"):
        tn.ops.nfft_ewald_lj_step_spectral(torch.zeros(1, 16, 16, 16, 2, dtype=torch.complex64), spc.coeffs, spd.coeffs,
                                           spd.strain_coeffs(), spc.box6, 12.0)


def _six(A):
    A = np.asarray(A, dtype=np.float64)
    return (ctypes.c_double * 6)(A[0, 0], A[1, 0], A[1, 1], A[2, 0], A[2, 1], A[2, 2])


def test_c_abi_validation_without_gpu():
    """the refusals of the siblings: null pointers, cells too small for r_cut, alpha not finite, workspace too small"""
    from torch_nfft_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 7 and lib.nfft_hip_abi_version() == 7
    for name in ("nfft_hip_ewald_lj_step_near_workspace_bytes", "nfft_hip_ewald_lj_step_near",
                 "nfft_hip_ewald_lj_step_spectral_workspace_bytes", "nfft_hip_ewald_lj_step_spectral"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)

    def problem(A=eb.O, **kw):
        f = dict(cells=(4, 5, 3), with_field=1, num_points=1000, num_columns=1, batch_size=1, alpha=14.0, r_cut=0.25,
                 box=_six(A))
        f.update(kw)
        f["cells"] = (ctypes.c_int32 * 3)(*f["cells"])
        return _lib.EwaldBoxProblem(**f)

    ok = problem()
    need = lib.nfft_hip_ewald_lj_step_near_workspace_bytes(ctypes.byref(ok), 12.0)
    assert need > 0
    for bad in (problem(cells=(5, 5, 3)), problem(cells=(2, 5, 3)), problem(with_field=2), problem(num_points=-1),
                problem(num_columns=2), problem(num_columns=0), problem(batch_size=0), problem(alpha=0.0),
                problem(alpha=float("inf")), problem(alpha=float("nan")), problem(r_cut=0.0), problem(r_cut=0.5)):
        assert lib.nfft_hip_ewald_lj_step_near_workspace_bytes(ctypes.byref(bad), 12.0) == -1
        assert _lib.last_error().startswith("Input mismatch")
    for bad_alpha in (0.0, -1.0, float("inf"), float("nan")):
        assert lib.nfft_hip_ewald_lj_step_near_workspace_bytes(ctypes.byref(ok), bad_alpha) == -1
        assert _lib.last_error() == "Input mismatch: alpha_dispersion must be positive and finite"
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(256)  # (never dereferenced: the checks come first)

    def near(q, alpha_d=12.0, ws=null, nbytes=0, points=one, xs=one, start=one, index=one, f=one, out=one):
        return lib.nfft_hip_ewald_lj_step_near(ctypes.byref(q), alpha_d, points, xs, start, index, f, out, ws, nbytes, null)

    assert near(ok) == _lib.EWORKSPACE and _lib.last_error() == "workspace too small"
    assert near(ok, ws=one, nbytes=need - 1) == _lib.EWORKSPACE
    for kw in (dict(out=null), dict(points=null), dict(xs=null), dict(start=null), dict(index=null), dict(f=null),
               dict(alpha_d=float("nan"))):
        assert near(ok, **kw) == _lib.EINVAL and _lib.last_error().startswith("Input mismatch")
    assert near(problem(cells=(2, 5, 3))) == _lib.EINVAL and near(problem(r_cut=0.5)) == _lib.EINVAL

    inv = _six(np.linalg.inv(eb.T))
    for N, B in ((6, 2), (32, 2), (256, 1)):
        assert lib.nfft_hip_ewald_lj_step_spectral_workspace_bytes(N, B) > 0
    for N, B in ((7, 1), (0, 1), (4096, 1), (8, 0), (8, 1 << 14)):
        assert lib.nfft_hip_ewald_lj_step_spectral_workspace_bytes(N, B) == -1
        assert _lib.last_error().startswith("Input mismatch")

    def spectral(N=8, B=1, band=one, bc=one, bd=one, td=one, inv=inv, p2a2=0.1, spectra=one, out=one, ws=null, nbytes=0):
        return lib.nfft_hip_ewald_lj_step_spectral(N, B, band, bc, bd, td, inv, p2a2, spectra, out, ws, nbytes, null)

    assert spectral() == _lib.EWORKSPACE and _lib.last_error() == "workspace too small"
    assert spectral(ws=one, nbytes=lib.nfft_hip_ewald_lj_step_spectral_workspace_bytes(8, 1) - 1) == _lib.EWORKSPACE
    nan = np.linalg.inv(eb.T)
    nan[1, 0] = float("nan")
    for kw in (dict(N=7), dict(band=null), dict(bc=null), dict(bd=null), dict(td=null), dict(spectra=null), dict(out=null),
               dict(p2a2=0.0), dict(p2a2=float("inf")), dict(inv=_six(nan)), dict(inv=_six(-np.eye(3))), dict(inv=None)):
        assert spectral(**kw) == _lib.EINVAL and _lib.last_error().startswith("Input mismatch")


# ---- the restatement -------------------------------------------------------------------------------------------------
# 30 points in the triclinic box T, no two closer than D_MIN, sigma about 0.8 x the typical nearest-neighbour distance, so that
# the three parts of the force are of comparable size.  The split: alpha_C = 13, alpha_D = 14, r_c = 0.3, N = 40.
D_MIN = 0.14
SPLIT = (13.0, 14.0, 0.3, 40)  # alpha_C, alpha_D, r_c, N
# The truncation factors of this split: erfc(alpha_C r_c) = 3.5e-8 and e^(-pi^2 kappa^2 / alpha_C^2) = 2e-8 at the grid's edge
# |kappa| >= (N/2) / 1.15 for the Coulomb sum; for the dispersion sum e^(-a^2)(1 + a^2 + a^4/2) = 3.9e-6 at a = alpha_D r_c = 4.2 and
# f(b) = 2.4e-8 at b = pi |kappa| / alpha_D = 3.9.  Each is the factor by which a term at the cut is smaller than the same term
# of the untruncated sum, and no point has more than a few neighbours at the cut: the restatement stands within the largest
# of them, 3.9e-6, of the converged sums; 1e-5 leaves a factor 2.5.
TRUNCATION = 1e-5
LARGEST_GPU_TOLERANCE = 1e-4  # (the condition of tests/test_gpu_lj_step.py on every gate)


@pytest.fixture(scope="module")
def system():
    rng = np.random.default_rng(11)
    s = lj.separated_points(rng, 30, eb.T, D_MIN).astype(np.float32).astype(np.float64)
    q = rng.standard_normal(30)
    q -= q.mean()
    sigma, eps = 0.15 * (1.0 + 0.1 * rng.random(30)), 0.5 + rng.random(30)
    c, a = lj.lj_coefficients(sigma, eps)
    return s, q, c, a


@pytest.fixture(scope="module")
def assembled(system):
    s, q, c, a = system
    return lj.exact_lj_step(q, c, a, s, eb.T, None, *SPLIT)


def test_parts_are_of_comparable_size(system):
    s, q, c, a = system
    r_c = SPLIT[2]
    z = np.zeros(30)
    parts = [np.linalg.norm(lj.converged_lj_step(*v, s, eb.T, r_c)[0]) for v in ((q, z, z), (z, c, z), (z, z, a))]
    print("|F| of the Coulomb, dispersion and repulsion parts: %.3g %.3g %.3g" % tuple(parts))
    assert max(parts) / min(parts) < 30.0
    d = lj.dr.min_separation(s, eb.T)
    assert d >= D_MIN * (1 - 1e-6)


def test_restatement_against_brute_force(system, assembled):
    """against the converged Coulomb sum (ewald_box_ref, ewald_virial_ref), the brute-force 1/r^6 lattice sum over every
    image within R = 14 with its continuum tail (dispersion_ref.lattice_sum) and r^-12 summed directly within r_c"""
    s, q, c, a = system
    F, UC, ULJ, W = assembled
    assert F.shape == (30, 3) and UC.shape == (1,) and ULJ.shape == (1,) and W.shape == (1, 3, 3)
    cF, cUC, cULJ, cW, (_, cUD, cUR) = lj.converged_lj_step(q, c, a, s, eb.T, SPLIT[2], R=14.0)
    e = rel_l2(F, cF), abs(UC[0] / cUC[0] - 1), abs(ULJ[0] - cULJ[0]) / (abs(cUD[0]) + abs(cUR[0])), rel_fro(W, cW)
    print("restatement vs brute force: F %.3e U_C %.3e U_LJ %.3e W %.3e" % e)
    assert max(e) <= TRUNCATION
    assert np.abs(W - W.transpose(0, 2, 1)).max() <= 1e-12 * np.abs(W).max()
    # tr W = U_C - 6 U_D + 12 U_R for the converged sums; the restatement's own parts within its truncation
    tr = np.trace(cW[0])
    want = cUC[0] - 6.0 * cUD[0] + 12.0 * cUR[0]
    scale = abs(cUC[0]) + 6.0 * abs(cUD[0]) + 12.0 * abs(cUR[0])
    print("tr W %.9g, U_C - 6 U_D + 12 U_R %.9g" % (tr, want))
    assert abs(tr - want) <= 1e-7 * scale  # (W from the analytic split, U_D from the lattice sum: the tail's own error)
    assert abs(np.trace(W[0]) - want) <= 3.0 * TRUNCATION * scale
    # Newton's third law
    assert np.abs(F.sum(0)).max() <= 1e-9 * np.abs(F).sum()
    assert np.abs(cF.sum(0)).max() <= 1e-9 * np.abs(cF).sum()


def test_force_and_virial_are_derivatives_of_the_energy(system):
    """F = -dU/dx and W = -dU/d eps by central differences (h = 1e-5) of the converged energy.  The truncation of the
    quotient is h^2 |U'''| / 6, with |U''' / U'| <= 14 * 15 / d_min^2 = 1.1e4 for r^-12: 2e-7 relative; its rounding 1e-16 |U| / h
    is smaller.  1e-5 leaves a factor 50.  No pair may cross r_c on the way: the repulsion jumps there."""
    s, q, c, a = system
    A, r_c, h = eb.T, SPLIT[2], 1e-5
    ds = s[:, None, :] - s[None, :, :]
    r = np.linalg.norm((ds - np.rint(ds)) @ A, axis=-1)
    assert np.abs(r - r_c).min() > 10 * h  # (a point moves by h, a strained separation by h r)
    F, _, _, W, _ = lj.converged_lj_step(q, c, a, s, A, r_c)
    inv = np.linalg.inv(A)
    fd = np.zeros((30, 3))
    for i in range(30):
        for k in range(3):
            dx = np.zeros(3)
            dx[k] = h
            sp, sm = s.copy(), s.copy()
            sp[i] += dx @ inv
            sm[i] -= dx @ inv
            fd[i, k] = -(lj.converged_energy(q, c, a, sp, A, r_c) - lj.converged_energy(q, c, a, sm, A, r_c)) / (2 * h)
    e = np.abs(F - fd).max() / np.abs(F).max()
    print("F against central differences: %.3e of |F|_max %.3g" % (e, np.abs(F).max()))
    assert e <= 1e-5
    fw = np.zeros((3, 3))
    for k in range(3):
        for l in range(3):
            eps = np.zeros((3, 3))
            eps[k, l] = h
            fw[k, l] = -(lj.converged_energy(q, c, a, s, A @ (np.eye(3) + eps), r_c)
                         - lj.converged_energy(q, c, a, s, A @ (np.eye(3) - eps), r_c)) / (2 * h)
    e = np.abs(W[0] - fw).max() / np.abs(W).max()
    print("W against central differences: %.3e of |W|_max %.3g" % (e, np.abs(W).max()))
    assert e <= 1e-5


def test_ragged_sets_and_single_species(system, assembled):
    """the composition set by set: two point sets with an empty one between give each set's own sums, and each species alone
    gives its own part"""
    s, q, c, a = system
    batch = np.concatenate([np.zeros(12, np.int64), np.full(18, 2, np.int64)])
    F, UC, ULJ, W = lj.exact_lj_step(q, c, a, s, eb.T, batch, *SPLIT)
    assert UC.shape == (3,) and UC[1] == 0 and ULJ[1] == 0 and not W[1].any()
    for b, sel in ((0, slice(0, 12)), (2, slice(12, 30))):
        f1, u1, l1, w1 = lj.exact_lj_step(q[sel], c[sel], a[sel], s[sel], eb.T, None, *SPLIT)
        assert rel_l2(F[sel], f1) <= 1e-12 and abs(UC[b] - u1[0]) <= 1e-12 * abs(u1[0])
        # (U_LJ is what is left of terms of the size of the dispersion sum's self term: rounded at that size)
        cancelling = abs(l1[0]) + SPLIT[1] ** 6 / 12.0 * (c[sel] * c[sel]).sum()
        assert abs(ULJ[b] - l1[0]) <= 1e-12 * cancelling and rel_fro(W[b], w1[0]) <= 1e-12
    z = np.zeros(30)
    total = [np.zeros_like(x) for x in assembled]
    for v in ((q, z, z), (z, c, z), (z, z, a)):
        for t, x in zip(total, lj.exact_lj_step(*v, s, eb.T, None, *SPLIT)):
            t += x
    for t, x in zip(total, assembled):
        assert np.abs(t - x).max() <= 1e-11 * np.abs(x).max()


@pytest.mark.parametrize("mutant", ["dispersion_sign", "six", "no_self"])
def test_mutants_are_far_off(system, assembled, mutant):
    """each wrong formula is off by at least 100 x the largest tolerance that a GPU test may have"""
    s, q, c, a = system
    F, UC, ULJ, W = assembled
    Fm, UCm, ULJm, Wm = lj.exact_lj_step(q, c, a, s, eb.T, None, *SPLIT, mutant=mutant)
    e = rel_l2(Fm, F), abs(ULJm[0] - ULJ[0]) / abs(ULJ[0]), rel_fro(Wm, W)
    print("mutant %-16s relative error of F %.3e, U_LJ %.3e, W %.3e" % ((mutant,) + e))
    assert UCm[0] == UC[0]
    if mutant == "no_self":
        assert e[1] >= 100 * LARGEST_GPU_TOLERANCE and e[0] == 0 and e[2] == 0
    elif mutant == "six":
        assert e[0] >= 100 * LARGEST_GPU_TOLERANCE and e[2] >= 100 * LARGEST_GPU_TOLERANCE and e[1] == 0
    else:
        assert min(e) >= 100 * LARGEST_GPU_TOLERANCE
