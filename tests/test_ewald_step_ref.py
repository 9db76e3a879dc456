"""CPU tests of the fused Ewald step: the resource figures of csrc/ewald_step.hip, the refusals of
nfft_ewald_step before any device work, the C ABI's validation, and the float64 restatement tests/ewald_step_ref.py -- a
composition of the committed restatements of the potential, the field and the virial -- against the converged sums, against
itself, and against five wrong formulas."""
import ctypes
import re

import numpy as np
import pytest
import torch

import ewald_box_ref as eb
import ewald_step_ref as es
import ewald_virial_ref as ev
from conftest import rel_l2


def test_kernel_resource_usage():
    """every instantiation of the two kernels: no scratch and no spills (the library's own flags; the VGPR, SGPR and LDS
    figures are recorded in DESIGN.md section 7q, not gated)"""
    from resource_usage import resource_usage
    usage = resource_usage("ewald_step.hip")
    seen = set()
    for name, u in sorted(usage.items()):
        m = re.search(r"(ewald_step_near_kernel)ILi(\d)ELb(\d)E|(ewald_step_spectral_kernel)ILi(\d)E", name)
        if not m:
            continue
        key = (m.group(1), int(m.group(2)), int(m.group(3))) if m.group(1) else (m.group(4), int(m.group(5)))
        seen.add(key)
        print(key, "VGPRs %d SGPRs %d occupancy %d LDS %d" % (u["VGPRs"], u["TotalSGPRs"], u["Occupancy"], u["LDS Size"]))
        assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (key, u)
    # (the unit cube runs as the identity box: BOX = true only)
    assert seen == {("ewald_step_near_kernel", cc, 1) for cc in (1, 2, 4)} | {("ewald_step_spectral_kernel", cc) for cc in (1, 2, 4)}


def test_refusals_without_gpu():
    import torch_nfft
    import torch_nfft_amd as tn
    assert "nfft_ewald_step" in tn.__all__ and torch_nfft.nfft_ewald_step is tn.nfft_ewald_step
    sp = tn.EwaldSplitting(12.0, 0.3, 16, box=eb.T, device="cpu")
    cube = tn.EwaldSplitting(12.0, 0.3, 16, device="cpu")
    q, pos = torch.zeros(5), torch.zeros(5, 3)
    with pytest.raises(ValueError, match="nfft_ewald_step: the charges must be real"):
        tn.nfft_ewald_step(q.to(torch.complex64), pos, splitting=sp)
    with pytest.raises(ValueError, match="nfft_ewald_step: .*three-dimensional"):
        tn.nfft_ewald_step(q, torch.zeros(5, 2), splitting=sp)
    with pytest.raises(ValueError, match="nfft_ewald_step: fractional=True needs"):
        tn.nfft_ewald_step(q, pos, splitting=cube, fractional=True)
    with pytest.raises(AssertionError, match="nfft_ewald_step: batch holds point-set indices and must not require grad"):
        tn.nfft_ewald_step(q, pos, torch.zeros(5, requires_grad=True), splitting=sp)
    with pytest.raises(TypeError, match="nfft_ewald_step: splitting must be an EwaldSplitting"):
        tn.nfft_ewald_step(q, pos)
    with pytest.raises(TypeError, match="nfft_ewald_step: splitting must be an EwaldSplitting"):
        tn.nfft_ewald_step(q, pos, splitting=tn.DispersionSplitting(4.0, 0.3, 16, device="cpu"))
    with pytest.raises(TypeError, match="exclusions must be an ExclusionList"):
        tn.nfft_ewald_step(q, pos, splitting=sp, exclusions=[(0, 1)])
    with pytest.raises(RuntimeError, match="is currently only implemented for GPU tensors"):
        tn.nfft_ewald_step(q, pos, splitting=sp)
    s = str(torch.ops.torch_nfft._nfft_ewald_step_near.default._schema)
    assert s == ("torch_nfft::_nfft_ewald_step_near(Tensor pos, Tensor x, Tensor? batch, float[] box, float alpha, "
                 "float r_cut) -> (Tensor, Tensor, Tensor)")
    s = str(torch.ops.torch_nfft._nfft_ewald_step_spectral.default._schema)
    assert s == "torch_nfft::_nfft_ewald_step_spectral(Tensor band, Tensor coeffs, float[] box, float alpha) -> (Tensor, Tensor)"
    with pytest.raises(RuntimeError, match="_nfft_ewald_step_near is currently only implemented for GPU tensors"):
        tn.ops.nfft_ewald_step_near(pos, q, None, sp.box6, 12.0, 0.3)
    with pytest.raises(RuntimeError, match="_nfft_ewald_step_spectral is currently only implemented for GPU tensors"):
        tn.ops.nfft_ewald_step_spectral(torch.zeros(1, 16, 16, 16, dtype=torch.complex64), sp.coeffs, sp.box6, 12.0)


def _six(A):
    A = np.asarray(A, dtype=np.float64)
    return (ctypes.c_double * 6)(A[0, 0], A[1, 0], A[1, 1], A[2, 0], A[2, 1], A[2, 2])


def test_c_abi_validation_without_gpu():
    """the checks, workspaces and error strings of the virial's two entry points (tests/test_ewald_virial_ref.py)"""
    from torch_nfft_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 7 and lib.nfft_hip_abi_version() == 7
    for name in ("nfft_hip_ewald_step_near_workspace_bytes", "nfft_hip_ewald_step_near",
                 "nfft_hip_ewald_step_spectral_workspace_bytes", "nfft_hip_ewald_step_spectral"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)

    def problem(A=eb.O, **kw):
        f = dict(cells=(4, 5, 3), with_field=1, num_points=1000, num_columns=2, batch_size=1, alpha=14.0, r_cut=0.25,
                 box=_six(A))
        f.update(kw)
        f["cells"] = (ctypes.c_int32 * 3)(*f["cells"])
        return _lib.EwaldBoxProblem(**f)

    ok = problem()
    need = lib.nfft_hip_ewald_step_near_workspace_bytes(ctypes.byref(ok))
    assert need == lib.nfft_hip_ewald_virial_near_workspace_bytes(ctypes.byref(ok)) > 0
    for bad in (problem(cells=(5, 5, 3)), problem(cells=(2, 5, 3)), problem(with_field=2), problem(num_points=-1),
                problem(num_columns=-1), problem(batch_size=0), problem(alpha=0.0), problem(r_cut=0.0),
                problem(num_columns=1 << 21), problem(batch_size=2048, num_columns=1 << 20)):
        assert lib.nfft_hip_ewald_step_near_workspace_bytes(ctypes.byref(bad)) == -1
        assert _lib.last_error().startswith("Input mismatch")
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(256)  # (never dereferenced: the checks come first)

    def near(q, ws=null, nbytes=0, points=one, index=one, z=one, f=one, out=one):
        return lib.nfft_hip_ewald_step_near(ctypes.byref(q), points, one, one, index, z, f, out, ws, nbytes, null)

    assert near(ok) == _lib.EWORKSPACE and _lib.last_error() == "workspace too small"
    assert near(ok, one, need - 1) == _lib.EWORKSPACE
    assert near(ok, out=null) == _lib.EINVAL and near(ok, points=null) == _lib.EINVAL
    assert near(problem(cells=(2, 5, 3))) == _lib.EINVAL
    assert near(problem(num_columns=0)) == _lib.OK  # nothing to do

    inv = _six(np.linalg.inv(eb.T))
    for N, B, C in ((6, 2, 3), (32, 2, 3), (256, 1, 1)):
        assert lib.nfft_hip_ewald_step_spectral_workspace_bytes(N, B, C) == lib.nfft_hip_ewald_virial_far_workspace_bytes(N, B, C) > 0
    for N, B, C in ((7, 1, 1), (0, 1, 1), (4096, 1, 1), (8, 0, 1), (8, 1, -1), (8, 1 << 14, 1), (8, 2, 1 << 20)):
        assert lib.nfft_hip_ewald_step_spectral_workspace_bytes(N, B, C) == -1
        assert _lib.last_error().startswith("Input mismatch")

    def spectral(N=8, B=1, C=1, band=one, coeffs=one, inv=inv, p2a2=0.1, spectra=one, out=one, ws=null, nbytes=0):
        return lib.nfft_hip_ewald_step_spectral(N, B, C, band, coeffs, inv, p2a2, spectra, out, ws, nbytes, null)

    assert spectral() == _lib.EWORKSPACE and _lib.last_error() == "workspace too small"
    assert spectral(ws=one, nbytes=lib.nfft_hip_ewald_step_spectral_workspace_bytes(8, 1, 1) - 1) == _lib.EWORKSPACE
    nan = np.linalg.inv(eb.T)
    nan[1, 0] = float("nan")
    for kw in (dict(N=7), dict(band=null), dict(coeffs=null), dict(spectra=null), dict(out=null), dict(p2a2=0.0),
               dict(p2a2=float("inf")), dict(inv=_six(nan)), dict(inv=_six(-np.eye(3))), dict(inv=None)):
        assert spectral(**kw) == _lib.EINVAL and _lib.last_error().startswith("Input mismatch")
    assert spectral(C=0) == _lib.OK  # nothing to do


@pytest.fixture(scope="module")
def charges():
    """300 float32 fractional positions with float64 charges of net charge 30 (those of tests/test_ewald_virial_ref.py's
    mutants), in two point sets"""
    rng = np.random.default_rng(0)
    s = (rng.random((300, 3)) - 0.5).astype(np.float32)
    q = rng.standard_normal(300)
    q -= q.mean()
    return s, q + 0.1, (np.arange(300) >= 140).astype(np.int64)


SPLIT = (12.0, 0.3, 32)  # in the box T: the first row of the truncation tables of sections 7h and 7i


@pytest.fixture(scope="module")
def assembled(charges):
    s, q, batch = charges
    return es.exact_step(q, s, eb.T, batch, *SPLIT)


def test_restatement_against_the_converged_sums(charges, assembled):
    """The composition that the GPU tests compare with, on two point sets in T, against the converged potential, field
    and virial.  The bounds are 1.5 x the truncation errors that tests/test_ewald_box_ref.py and
    tests/test_ewald_virial_ref.py record for this split on 300 charges (phi 1.03e-7, E 4.67e-7, W 3.34e-6): the same
    margin as there.  Then the composition against itself: U is the energy of phi, set by set, which a potential and a
    virial taken from different conventions (batch, units, background) would not satisfy."""
    s, q, batch = charges
    phi, E, U, W = assembled
    assert phi.shape == (300,) and E.shape == (300, 3) and U.shape == (2,) and W.shape == (2, 3, 3)
    cphi, cE, cU, cW = es.converged_step(q, s, eb.T, batch, nimg=1)
    e = rel_l2(phi, cphi), rel_l2(E, cE), ev.rel_fro(U, cU), ev.rel_fro(W, cW)
    print("restatement vs converged: phi %.3e E %.3e U %.3e W %.3e" % e)
    assert e[0] <= 1.5 * 1.03e-7 and e[1] <= 1.5 * 4.67e-7 and e[3] <= 1.5 * 3.34e-6
    want = es.energy_of(q, phi, batch)
    assert np.abs(U - want).max() <= 1e-10 * np.abs(want).max()
    assert e[2] <= 1e-10 + rel_l2(want, es.energy_of(q, cphi, batch))  # (U is cut off as phi is)
    assert np.abs(W - W.transpose(0, 2, 1)).max() <= 1e-12
    # tr W = U for the converged sum; the algorithm's own differ by its truncation of W and U
    tr = np.trace(W, axis1=1, axis2=2)
    assert np.abs(tr - U).max() <= np.sqrt(3.0) * np.linalg.norm(W - cW) + np.linalg.norm(U - cU) + 1e-9
    # excluded pairs come out of all four consistently: U stays the energy of phi
    pairs = np.array([[0, 1], [5, 9], [150, 170]])
    w = np.array([1.0, 0.5, 1.0 - 1.0 / 1.2])
    xphi, xE, xU, xW = es.exact_step(q, s, eb.T, batch, *SPLIT, pairs=pairs, weights=w)
    want = es.energy_of(q, xphi, batch)
    assert np.abs(xU - want).max() <= 1e-10 * np.abs(want).max()
    assert np.abs(xphi - phi).max() > 0 and np.abs(xE - E).max() > 0 and np.abs(xW - W).max() > 0


# the relative error of W that each wrong formula of ewald_virial_ref makes (header of tests/test_gpu_ewald_virial.py); the
# largest tolerance of tests/test_gpu_ewald_step.py is WHOLE_TOL["U"] = 5.5e-5, the largest on W 2 x 3.2e-6
MUTANTS = {"ds": 0.15, "AT": 0.16, "k": 2.7, "no_pi2": 2.5, "no_background": 0.036}
LARGEST_GPU_TOLERANCE = 1e-4


def test_mutants_are_far_off(charges, assembled):
    """on the charges as one point set, the configuration behind the recorded sizes"""
    s, q, _ = charges
    W = es.exact_step(q, s, eb.T, None, *SPLIT)[3]
    for mutant, recorded in MUTANTS.items():
        Wm = es.exact_step(q, s, eb.T, None, *SPLIT, mutant=mutant)[3]
        err = ev.rel_fro(Wm, W)
        print("mutant %-14s relative error of the assembled W %.3e (recorded %.2e)" % (mutant, err, recorded))
        assert err >= 100 * LARGEST_GPU_TOLERANCE
        assert 0.5 * recorded <= err <= 2.0 * recorded
    # a field with the wrong sign, a potential without its self term: what the composition of (phi, E) must not hide
    phi, E = assembled[0], assembled[1]
    assert rel_l2(-E, E) == 2.0
    assert rel_l2(phi + 2.0 * SPLIT[0] / np.sqrt(np.pi) * q, phi) >= 100 * LARGEST_GPU_TOLERANCE
