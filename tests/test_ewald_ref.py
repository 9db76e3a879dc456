"""CPU tests of the Ewald sum for the periodic 1/r (nfft_ewald): the float64 restatement
tests/ewald_ref.py against the fixed points of the lattice sums and against itself, the host-side pieces of
torch_nfft_amd/ewald.py against the restatement, the refusals and the C ABI's validation."""
import ctypes
import math

import numpy as np
import pytest
import torch

import ewald_ref as er
from conftest import rel_l2


@pytest.fixture(scope="module")
def charges():
    """300 float32 positions in the box with neutral float64 charges, and the converged sum at alpha = 6"""
    rng = np.random.default_rng(0)
    x = (rng.random((300, 3)) - 0.5).astype(np.float32)
    q = rng.standard_normal(300)
    q -= q.mean()
    return x, q, er.converged(q, x)


def test_madelung_and_single_charge():
    x, q = er.nacl()
    phi = er.converged(q, x)
    assert np.abs(phi * q * 0.5 + 1.747564594633).max() <= 1e-9
    assert abs(er.MADELUNG_NACL - 1.747564594633) < 1e-12
    # one charge and its background: the cubic-lattice constant, at any position
    for pos in ([0.0, 0.0, 0.0], [0.31, -0.47, 0.123]):
        phi = er.converged(np.array([1.5]), np.array([pos]))
        assert abs(phi[0] / 1.5 + 2.837297479) <= 1e-9
    assert abs(er.CUBIC_LATTICE + 2.837297479) < 1e-9


def test_converged_does_not_depend_on_alpha(charges):
    x, q, ref = charges
    assert rel_l2(er.converged(q, x, alpha=8.0), ref) <= 1e-12
    qn = np.random.default_rng(1).standard_normal(300)  # not neutral: the background term
    assert rel_l2(er.converged(qn, x, alpha=8.0), er.converged(qn, x)) <= 1e-12


def test_field_is_the_gradient_of_the_energy():
    """E_i q_i = -dU/dx_i with U = 1/2 sum q phi, by central differences (h = 1e-5: error O(h^2 U''') ~ 1e-7 relative)"""
    rng = np.random.default_rng(2)
    n = 12
    x = rng.random((n, 3)) - 0.5
    q = rng.standard_normal(n)
    _, E = er.converged(q, x, field=True)
    h = 1e-5
    for i, a in ((0, 0), (5, 1), (11, 2)):
        xp, xm = x.copy(), x.copy()
        xp[i, a] += h
        xm[i, a] -= h
        dU = (0.5 * (q * er.converged(q, xp)).sum() - 0.5 * (q * er.converged(q, xm)).sum()) / (2 * h)
        assert abs(-dU - q[i] * E[i, a]) <= 1e-6 * np.abs(q[:, None] * E).max()
    # the same for the algorithm's own field, near and far part (alpha = 7, r_c = 1/3, N = 16: a coarse split, exact gradient)
    phi_alg, E_alg = er.exact_algorithm(q, x, None, 7.0, 1.0 / 3.0, 16, field=True)
    assert rel_l2(phi_alg, er.exact_algorithm(q, x, None, 7.0, 1.0 / 3.0, 16)) <= 1e-13
    i, a = 3, 1
    xp, xm = x.copy(), x.copy()
    xp[i, a] += h
    xm[i, a] -= h
    # (no pair may cross r_c between the two evaluations: the truncated near sum jumps there by erfc(7/3)/r_c ~ 3e-3)
    dU = (0.5 * (q * er.exact_algorithm(q, xp, None, 7.0, 1.0 / 3.0, 16)).sum()
          - 0.5 * (q * er.exact_algorithm(q, xm, None, 7.0, 1.0 / 3.0, 16)).sum()) / (2 * h)
    d = x[i] - x
    d -= np.rint(d)
    r = np.sqrt((d * d).sum(-1))
    assert np.abs(r - 1.0 / 3.0).min() > 10 * h
    assert abs(-dU - q[i] * E_alg[i, a]) <= 1e-6 * np.abs(q[:, None] * E_alg).max()


@pytest.mark.parametrize("alpha,r_c,N,measured", [(12.0, 0.3, 32, 9.2e-8), (14.0, 0.25, 32, 2.2e-7)])
def test_exact_algorithm_against_converged(charges, alpha, r_c, N, measured):
    """the truncation error of the split, relative l2 of phi on 300 neutral charges: 9.2e-8 and 2.2e-7"""
    x, q, ref = charges
    err = rel_l2(er.exact_algorithm(q, x, None, alpha, r_c, N), ref)
    print("exact algorithm (%g, %g, %d): rel_l2 vs converged %.3e (recorded %.1e)" % (alpha, r_c, N, err, measured))
    assert err <= 1e-6


def test_splitting_coefficients_and_from_tolerance():
    import torch_nfft
    import torch_nfft_amd as tn
    assert torch_nfft.nfft_ewald is tn.nfft_ewald and torch_nfft.EwaldSplitting is tn.EwaldSplitting
    assert torch_nfft.nfft_ewald_energy is tn.nfft_ewald_energy
    for alpha, N in ((12.0, 32), (7.5, 16)):
        sp = tn.EwaldSplitting(alpha, 0.3, N, device="cpu")
        assert sp.coeffs.shape == (N, N, N) and sp.coeffs.dtype == torch.float32
        want = er.coeffs(alpha, N)
        assert np.abs(sp.coeffs.numpy() - want).max() <= 6e-8 * np.abs(want).max()  # (float32 rounding of float64 values)
        b = sp.coeffs.numpy()
        assert b[N // 2, N // 2, N // 2] == 0 and not b[0].any() and not b[:, 0].any() and not b[:, :, 0].any()
        assert (b[1:, 1:, 1:] == b[1:, 1:, 1:][::-1, ::-1, ::-1]).all()  # even: a real q gives a real phi
        fc = sp.field_coeffs()
        assert fc.shape == (N, N, N, 4) and fc.dtype == torch.complex64
        k = 2 * math.pi * np.arange(-(N // 2), N // 2)
        assert rel_l2(fc[..., 2].numpy(), 1j * want * k[None, :, None]) <= 2e-7
    sp = tn.EwaldSplitting.from_tolerance(1e-6, 0.3, device="cpu")
    s = math.sqrt(-math.log(1e-6))
    assert sp.r_cut == 0.3 and abs(sp.alpha - s / 0.3) <= 1e-12
    lower = 2 * sp.alpha * s / math.pi
    assert sp.bandwidth % 2 == 0 and lower <= sp.bandwidth < lower + 2
    assert abs(math.erfc(sp.alpha * sp.r_cut) / 1e-6) < 1 and math.exp(-(math.pi * sp.bandwidth / 2 / sp.alpha) ** 2) <= 1e-6


def test_refusals():
    import torch_nfft_amd as tn
    for bad in (dict(r_cut=0.34), dict(r_cut=0.0), dict(bandwidth=31), dict(bandwidth=0), dict(alpha=0.0), dict(alpha=-1.0)):
        kw = dict(alpha=12.0, r_cut=0.3, bandwidth=32, device="cpu")
        kw.update(bad)
        with pytest.raises(ValueError):
            tn.EwaldSplitting(**kw)
    with pytest.raises(ValueError):
        tn.EwaldSplitting.from_tolerance(1e-6, 0.34, device="cpu")
    assert tn.EwaldSplitting(12.0, 1.0 / 3.0, 32, device="cpu").r_cut == 1.0 / 3.0
    sp = tn.EwaldSplitting(12.0, 0.3, 16, device="cpu")
    q, pos = torch.zeros(5), torch.zeros(5, 3)
    for fn in (tn.nfft_ewald, tn.nfft_ewald_energy):
        with pytest.raises(ValueError, match="three-dimensional"):
            fn(q, torch.zeros(5, 2), splitting=sp)
        with pytest.raises(AssertionError, match="batch"):
            fn(q, pos, torch.zeros(5, requires_grad=True), splitting=sp)
        with pytest.raises(RuntimeError, match="is currently only implemented for GPU tensors"):
            fn(q, pos, splitting=sp)
        with pytest.raises(TypeError):
            fn(q, pos)
    with pytest.raises(RuntimeError, match="is currently only implemented for GPU tensors"):
        tn.nfft_ewald(q, pos, splitting=sp, field=True)
    s = str(torch.ops.torch_nfft._nfft_ewald_near.default._schema)
    assert s == ("torch_nfft::_nfft_ewald_near(Tensor pos, Tensor x, Tensor? batch, float alpha, float r_cut, "
                 "bool with_field) -> (Tensor, Tensor)")
    with pytest.raises(RuntimeError, match="torch_nfft._nfft_ewald_near is currently only implemented for GPU tensors"):
        tn.ops.nfft_ewald_near(pos, q, None, 12.0, 0.3, True)


def test_c_abi_validation_without_gpu():
    from torch_nfft_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 7 and lib.nfft_hip_abi_version() == 7
    for name in ("nfft_hip_ewald_near_cells", "nfft_hip_ewald_near_workspace_bytes", "nfft_hip_ewald_near"):
        assert name in _lib.SYMBOLS
    assert lib.nfft_hip_ewald_near_cells(0.3, 1) == 3
    assert lib.nfft_hip_ewald_near_cells(0.25, 1) == 4
    assert lib.nfft_hip_ewald_near_cells(1.0 / 3.0, 1) == 3
    assert lib.nfft_hip_ewald_near_cells(0.12, 1) == 8
    assert lib.nfft_hip_ewald_near_cells(0.01, 2) == 80  # 2 * 80^3 <= 2^20 < 2 * 81^3
    for r_cut, batch in ((0.34, 1), (0.0, 1), (-0.1, 1), (float("nan"), 1), (0.3, 0), (0.3, 1 << 20)):
        assert lib.nfft_hip_ewald_near_cells(r_cut, batch) == -1
        assert _lib.last_error().startswith("Input mismatch")

    def problem(**kw):
        f = dict(cells_per_axis=4, with_field=1, num_points=1000, num_columns=2, batch_size=1, alpha=14.0, r_cut=0.25)
        f.update(kw)
        return _lib.EwaldProblem(**f)

    ok = problem()
    need = lib.nfft_hip_ewald_near_workspace_bytes(ctypes.byref(ok))
    assert need == (1000 // 128 + 64 + 1) * 8 + 256
    assert lib.nfft_hip_ewald_near_workspace_bytes(ctypes.byref(problem(cells_per_axis=3))) > 0  # (coarser cells are valid)
    for bad in (problem(cells_per_axis=2), problem(cells_per_axis=5), problem(with_field=2), problem(num_points=-1),
                problem(num_columns=-1), problem(batch_size=0), problem(alpha=0.0), problem(alpha=float("nan")),
                problem(r_cut=0.34, cells_per_axis=3), problem(r_cut=0.0), problem(num_points=1 << 31),
                problem(batch_size=1 << 15)):
        assert lib.nfft_hip_ewald_near_workspace_bytes(ctypes.byref(bad)) == -1
        assert _lib.last_error().startswith("Input mismatch")
    assert lib.nfft_hip_ewald_near_workspace_bytes(None) == -1
    null = ctypes.c_void_p(0)
    one = ctypes.c_void_p(256)  # (never dereferenced: the checks come first)

    def call(q, ws=null, nbytes=0, z=one, field=one, points=one):
        return lib.nfft_hip_ewald_near(ctypes.byref(q), points, one, one, one, z, field, ws, nbytes, null)

    assert call(ok) == _lib.EWORKSPACE and _lib.last_error() == "workspace too small"
    assert call(ok, one, need - 1) == _lib.EWORKSPACE
    assert call(problem(with_field=0), field=null) == _lib.EWORKSPACE  # (the field is not asked for: no pointer needed)
    assert call(ok, field=null) == _lib.EINVAL and _lib.last_error().startswith("Input mismatch")
    assert call(ok, z=null) == _lib.EINVAL
    assert call(ok, points=null) == _lib.EINVAL
    assert call(problem(cells_per_axis=2)) == _lib.EINVAL
    assert call(problem(r_cut=0.34, cells_per_axis=3)) == _lib.EINVAL
    # nothing to do: no launch, no workspace needed
    assert call(problem(num_points=0)) == _lib.OK
    assert call(problem(num_columns=0)) == _lib.OK


def test_pair_kernel_resource_usage():
    """every instantiation <CC, FIELD, BOX> of the Ewald pair kernel, the cubic ones and those of the box: no scratch and no
    spills (the library's own flags; VGPRs are recorded in DESIGN.md sections 7g and 7h, not gated)"""
    import re
    from resource_usage import resource_usage
    usage = resource_usage("ewald_near.hip")
    by = {}
    for name, u in usage.items():
        m = re.search(r"ewald_near_kernelILi(\d)ELb(\d)ELb(\d)EE", name)
        if m:
            by[(int(m.group(1)), int(m.group(2)), int(m.group(3)))] = u
    assert set(by) == {(cc, f, box) for cc in (1, 2, 4) for f in (0, 1) for box in (0, 1)}
    for key, u in sorted(by.items()):
        print(key, "VGPRs %d occupancy %d LDS %d" % (u["VGPRs"], u["Occupancy"], u["LDS Size"]))
        assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (key, u)
