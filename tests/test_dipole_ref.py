"""CPU tests of the Ewald sum for point charges and point dipoles (nfft_ewald_dipole): the float64
restatement tests/dipole_ref.py against itself (two splittings, finite differences, a dipole as a pair of charges, forces,
the trace of T), against tests/ewald_box_ref.py for pure charges and against the mistakes a pair sweep can make; the exports,
schemas and refusals of the Python layer; the C ABI; the registers of the kernels."""
import ctypes
import math
import re

import numpy as np
import pytest
import torch

import dipole_ref as dp
import ewald_box_ref as eb
from conftest import rel_l2
from ewald_box_ref import O, T
from oracle import ndft

BOXES = {"cube": None, "T": T, "O": O}


def _random_sources(seed, n=12, cols=()):
    rng = np.random.default_rng(seed)
    return rng.random((n, 3)) - 0.5, rng.standard_normal((n,) + cols), rng.standard_normal((n, 3) + cols)


@pytest.mark.parametrize("box", ["cube", "T"])
def test_converged_does_not_depend_on_alpha(box):
    s, q, mu = _random_sources(1, cols=(2,))
    a, b = dp.converged(q, mu, s, BOXES[box], alpha=6.0), dp.converged(q, mu, s, BOXES[box], alpha=8.0)
    for what, x, y in zip(("phi", "E", "T"), a, b):
        print("converged in %s at alpha = 6 and 8: %s rel_l2 %.3e" % (box, what, rel_l2(x, y)))
        assert rel_l2(x, y) <= 1e-12


@pytest.mark.parametrize("box", ["cube", "T"])
def test_field_and_gradient_are_derivatives(box):
    """E = -grad phi and T_ab = d E_a / d x_b at a probe point that carries nothing, by central differences (h = 1e-5: O(h^2)
    truncation and 1e-16 / h rounding are both far below 1e-6 of the values)"""
    A = BOXES[box]
    inv = np.linalg.inv(np.eye(3) if A is None else A)
    s, q, mu = _random_sources(2)
    q[0], mu[0] = 0.0, 0.0
    phi, E, Tn = dp.converged(q, mu, s, A)
    h = 1e-5
    for b in range(3):
        e = np.zeros(3)
        e[b] = h
        sp, sm = s.copy(), s.copy()
        sp[0] += e @ inv
        sm[0] -= e @ inv
        (pp, Ep, _), (pm, Em, _) = dp.converged(q, mu, sp, A, order=1), dp.converged(q, mu, sm, A, order=1)
        assert abs(-(pp[0] - pm[0]) / (2 * h) - E[0, b]) <= 1e-6 * np.abs(E[0]).max()
        assert np.abs((Ep[0] - Em[0]) / (2 * h) - Tn[0, :, b]).max() <= 1e-6 * np.abs(Tn[0]).max()
    assert np.abs(Tn - Tn.transpose(0, 2, 1)).max() <= 1e-12 * np.abs(Tn).max()


def test_dipole_is_a_pair_of_charges():
    """a dipole mu at x_0 against the charges +-1/h at x_0 +- h mu / 2 (error O(h^2)), seen from every other source"""
    s, q, mu = _random_sources(3)
    q[0] = 0.0
    want = dp.converged(q, mu, s, T)
    h = 1e-4
    d = 0.5 * h * mu[0] @ np.linalg.inv(T)
    s2 = np.concatenate([s, [s[0] + d, s[0] - d]])
    q2 = np.concatenate([q, [1.0 / h, -1.0 / h]])
    mu2 = np.concatenate([mu, np.zeros((2, 3))])
    mu2[0] = 0.0
    got = dp.converged(q2, mu2, s2, T)
    for what, x, y in zip(("phi", "E", "T"), got, want):
        print("a dipole as a pair of charges: %s rel_l2 %.3e" % (what, rel_l2(x[1:12], y[1:])))
        assert rel_l2(x[1:12], y[1:]) <= 1e-6


@pytest.mark.parametrize("box", ["cube", "T"])
def test_force_is_minus_the_energy_gradient(box):
    A = BOXES[box]
    inv = np.linalg.inv(np.eye(3) if A is None else A)
    s, q, mu = _random_sources(4)
    phi, E, Tn = dp.converged(q, mu, s, A)
    F = dp.force(q, mu, E, Tn)
    h = 1e-5
    for i, a in ((0, 0), (5, 1), (11, 2)):
        e = np.zeros(3)
        e[a] = h
        sp, sm = s.copy(), s.copy()
        sp[i] += e @ inv
        sm[i] -= e @ inv
        U = [dp.energy(q, mu, *dp.converged(q, mu, x, A, order=1)[:2])[0] for x in (sp, sm)]
        assert abs(-(U[0] - U[1]) / (2 * h) - F[i, a]) <= 1e-6 * np.abs(F).max()


@pytest.mark.parametrize("box", ["cube", "T", "O"])
def test_trace_of_the_field_gradient(box):
    """tr T_i = -4 pi Q / V: Poisson's equation with the neutralising background (every source is a point: no density at i)"""
    A = BOXES[box]
    s, q, mu = _random_sources(5)
    V = 1.0 if A is None else float(np.linalg.det(A))
    Tn = dp.converged(q, mu, s, A)[2]
    tr = Tn[:, 0, 0] + Tn[:, 1, 1] + Tn[:, 2, 2]
    assert np.abs(tr + 4.0 * math.pi * q.sum() / V).max() <= 1e-11 * np.abs(Tn).max()


@pytest.mark.parametrize("box", ["cube", "T"])
def test_pure_charges_reproduce_the_coulomb_restatement(box):
    A = np.eye(3) if BOXES[box] is None else BOXES[box]
    s, q, _ = _random_sources(6, n=40, cols=(2,))
    batch = (np.arange(40) >= 17).astype(np.int64)
    phi, E, _ = dp.exact_algorithm(q, None, s, BOXES[box], batch, 7.0, 0.3, 16, order=1)
    want = eb.exact_algorithm(q, s, A, batch, 7.0, 0.3, 16, field=True)
    assert rel_l2(phi, want[0]) <= 1e-12 and rel_l2(E, want[1]) <= 1e-12


@pytest.mark.parametrize("box", ["cube", "T"])
def test_spectral_table_composes_the_far_part(box):
    """the far part as the operators compose it -- adjoint transform of the packed sources, the table, forward transform --
    is the dense far sum (exact transforms of oracle/ndft.py in float64)"""
    A = BOXES[box]
    s, q, mu = _random_sources(7, n=20, cols=(2,))
    batch = (np.arange(20) >= 8).astype(np.int64)
    N = 8
    xs = np.concatenate([q[:, None], mu], 1)  # [n, 4, 2]
    band = ndft.ndft_adjoint(xs.reshape(20, 8), s, batch, N=N).reshape(2, N, N, N, 4, 2)
    spectra = np.einsum("xyzsr,bxyzrc->bxyzsc", dp.spectral_table(A, 5.0, N), band)
    got = ndft.ndft_forward(spectra.reshape(2, N, N, N, 20), s, batch).real.reshape(20, 10, 2)
    phi, E, Tn = dp.far(q, mu, s, A, batch, 5.0, N)
    assert rel_l2(got[:, 0], phi) <= 1e-12 and rel_l2(got[:, 1:4], E) <= 1e-12 and rel_l2(got[:, 4:], dp.voigt(Tn)) <= 1e-12


# (alpha, r_c) of the GPU near-sweep tests: alpha r_c ~ 1.5, G = 3, 4, 8 cells per axis
NEAR_CASES = [(5.0, 0.3), (6.0, 0.25), (12.0, 0.12)]


@pytest.mark.parametrize("alpha,r_c", NEAR_CASES)
def test_near_sum_is_sensitive_to_mistakes(alpha, r_c):
    """On the points and sources of the GPU near-sweep test four mistakes of a pair sweep each move some output by at least ten
    times the gate that the device run is held to (tests/test_gpu_dipole.py: max(4 x the float32 emulation's error, the
    committed Coulomb figure) per quantity): the B_3 term dropped, the m delta_ab B_2 term dropped, no wrap, a cut at 0.95 r_c.
    These (alpha, r_c) have alpha r_c = 1.5, 1.5 and 1.44: the pairs at the cut still weigh erfc(1.5) = 3e-2 of a near one."""
    from test_gpu_ewald import NEAR_TOL
    x = dp.near_points()
    q, mu = dp.near_sources(1, 512, ())
    ref = dp.near(q, mu, x, None, None, alpha, r_c)
    emu = dp.near_f32(q, mu, x, None, None, alpha, r_c)
    gates = [dp.near_gate(w, e, r, NEAR_TOL[k])[0] for w, e, r, k in zip("pET", emu, ref, ("value", "field", "field"))]
    print("(%g, %g) gates: phi %.3e, E %.3e, T %.3e" % ((alpha, r_c) + tuple(gates)))
    for what, kw, rc in (("no B_3", dict(b3=False), r_c), ("no m delta B_2", dict(mdelta=False), r_c), ("no wrap", dict(wrap=False), r_c),
                         ("0.95 r_c", {}, 0.95 * r_c)):
        moved = [rel_l2(a, b) for a, b in zip(dp.near(q, mu, x, None, None, alpha, rc, **kw), ref)]
        print("(%g, %g) %s: phi moves by %.3e, E by %.3e, T by %.3e" % ((alpha, r_c, what) + tuple(moved)))
        assert max(m / g for m, g in zip(moved, gates)) >= 10.0


def test_float32_emulation_is_float32():
    x = dp.near_points()
    q, mu = dp.near_sources(2, 512, (2,))
    ref, emu = dp.near(q, mu, x, T, None, 6.0, 0.25), dp.near_f32(q, mu, x, T, None, 6.0, 0.25)
    for what, a, b in zip(("phi", "E", "T"), emu, ref):
        e = rel_l2(a.astype(np.float64), b)
        print("float32 emulation in T at (6, 0.25): %s rel_l2 %.3e" % (what, e))
        assert a.dtype == np.float32 and 1e-9 < e < 1e-5  # (float32 indeed, and nothing worse)


def test_exports_schemas_and_refusals():
    import torch_nfft
    import torch_nfft_amd as tn
    for name in ("nfft_ewald_dipole", "nfft_ewald_dipole_energy"):
        assert name in tn.__all__ and getattr(torch_nfft, name) is getattr(tn, name)
    s = str(torch.ops.torch_nfft._nfft_ewald_dipole_near.default._schema)
    assert s == ("torch_nfft::_nfft_ewald_dipole_near(Tensor pos, Tensor xs, Tensor? batch, float[] box, float alpha, "
                 "float r_cut, int order) -> Tensor")
    s = str(torch.ops.torch_nfft._nfft_ewald_dipole_spectral.default._schema)
    assert s == "torch_nfft::_nfft_ewald_dipole_spectral(Tensor band, Tensor coeffs, float[] box, int order) -> Tensor"
    sp = tn.EwaldSplitting(6.0, 0.3, 16, device="cpu")
    spb = tn.EwaldSplitting(6.0, 0.25, 16, box=[1.0, 1.3, 0.8], device="cpu")
    q, mu, pos = torch.zeros(5), torch.zeros(5, 3), torch.zeros(5, 3)
    with pytest.raises(RuntimeError, match="torch_nfft._nfft_ewald_dipole_near is currently only implemented for GPU tensors"):
        tn.ops.nfft_ewald_dipole_near(pos, torch.zeros(5, 4), None, (), 6.0, 0.3, 2)
    with pytest.raises(RuntimeError, match="torch_nfft._nfft_ewald_dipole_near is currently only implemented for GPU tensors"):
        tn.ops.nfft_ewald_dipole_near(pos, torch.zeros(5, 4), None, spb.box6, 6.0, 0.25, 1)
    with pytest.raises(RuntimeError, match="torch_nfft._nfft_ewald_dipole_spectral is currently only implemented for GPU tensors"):
        tn.ops.nfft_ewald_dipole_spectral(torch.zeros(1, 16, 16, 16, 4, dtype=torch.complex64), sp.coeffs, (), 2)
    for fn in (tn.nfft_ewald_dipole, tn.nfft_ewald_dipole_energy):
        with pytest.raises(TypeError, match="EwaldSplitting"):
            fn(q, mu, pos)
        with pytest.raises(TypeError, match="EwaldSplitting"):
            fn(q, mu, pos, splitting=tn.DispersionSplitting(6.0, 0.3, 16, device="cpu"))
        with pytest.raises(ValueError, match="complex"):
            fn(q.to(torch.complex64), mu, pos, splitting=sp)
        with pytest.raises(ValueError, match="complex"):
            fn(q, mu.to(torch.complex64), pos, splitting=sp)
        with pytest.raises(ValueError, match="float32"):
            fn(q.double(), mu, pos, splitting=sp)
        with pytest.raises(ValueError, match="three-dimensional"):
            fn(q, mu, torch.zeros(5, 2), splitting=sp)
        with pytest.raises(ValueError, match="mu must be"):
            fn(q, torch.zeros(5, 2), pos, splitting=sp)
        with pytest.raises(ValueError, match="same columns"):
            fn(torch.zeros(5, 2), mu, pos, splitting=sp)
        with pytest.raises(ValueError, match="both be None"):
            fn(None, None, pos, splitting=sp)
        with pytest.raises(ValueError, match="fractional"):
            fn(q, mu, pos, splitting=sp, fractional=True)
        with pytest.raises(AssertionError, match="batch"):
            fn(q, mu, pos, torch.zeros(5, requires_grad=True), splitting=sp)
        for kw in (dict(splitting=sp), dict(splitting=spb), dict(splitting=spb, fractional=True)):
            with pytest.raises(RuntimeError, match="is currently only implemented for GPU tensors"):
                fn(q, mu, pos, **kw)
        with pytest.raises(RuntimeError, match="is currently only implemented for GPU tensors"):
            fn(None, mu, pos, splitting=sp)
        with pytest.raises(RuntimeError, match="is currently only implemented for GPU tensors"):
            fn(q, None, pos, splitting=sp)
    with pytest.raises(RuntimeError, match="is currently only implemented for GPU tensors"):
        tn.nfft_ewald_dipole(q, mu, pos, splitting=sp, gradient=True)


def test_c_abi_validation_without_gpu():
    """the three symbols; the near entry points validate as their Coulomb twins do, refuse an order other than 1 or 2 and take
    the workspace that the shared size functions report"""
    from torch_nfft_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 7 and lib.nfft_hip_abi_version() == 7
    for name in ("nfft_hip_ewald_dipole_near", "nfft_hip_ewald_dipole_near_box", "nfft_hip_ewald_dipole_spectral"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(256)  # (never dereferenced: the checks come first)

    def problem(**kw):
        f = dict(cells_per_axis=4, with_field=1, num_points=1000, num_columns=2, batch_size=1, alpha=6.0, r_cut=0.25)
        f.update(kw)
        return _lib.EwaldProblem(**f)

    def call(q, order=2, ws=null, nbytes=0, out=one, points=one):
        return lib.nfft_hip_ewald_dipole_near(ctypes.byref(q), points, one, one, one, order, out, ws, nbytes, null)

    ok = problem()
    need = lib.nfft_hip_ewald_near_workspace_bytes(ctypes.byref(ok))
    assert need > 0
    for order in (1, 2):
        assert call(ok, order) == _lib.EWORKSPACE and _lib.last_error() == "workspace too small"
        assert call(ok, order, one, need - 1) == _lib.EWORKSPACE
    assert call(problem(with_field=0)) == _lib.EWORKSPACE
    for order in (0, 3, -1):
        assert call(ok, order) == _lib.EINVAL and _lib.last_error() == "Input mismatch: order must be 1 or 2"
    assert call(ok, out=null) == _lib.EINVAL and call(ok, points=null) == _lib.EINVAL
    for bad in (problem(cells_per_axis=2), problem(cells_per_axis=5), problem(with_field=2), problem(num_points=-1),
                problem(alpha=0.0), problem(r_cut=0.34, cells_per_axis=3), problem(batch_size=0)):
        assert call(bad) == _lib.EINVAL and _lib.last_error().startswith("Input mismatch")
    assert call(problem(num_points=0)) == _lib.OK and call(problem(num_columns=0)) == _lib.OK

    def box_problem(**kw):
        f = dict(cells=(ctypes.c_int32 * 3)(4, 5, 3), with_field=1, num_points=1000, num_columns=2, batch_size=1, alpha=6.0,
                 r_cut=0.25, box=(ctypes.c_double * 6)(1.0, 0.0, 1.3, 0.0, 0.0, 0.8))
        f.update(kw)
        return _lib.EwaldBoxProblem(**f)

    def box_call(q, order=2, ws=null, nbytes=0, out=one):
        return lib.nfft_hip_ewald_dipole_near_box(ctypes.byref(q), one, one, one, one, order, out, ws, nbytes, null)

    okb = box_problem()
    needb = lib.nfft_hip_ewald_near_box_workspace_bytes(ctypes.byref(okb))
    assert needb > 0
    assert box_call(okb) == _lib.EWORKSPACE and box_call(okb, 1, one, needb - 1) == _lib.EWORKSPACE
    assert box_call(okb, 0) == _lib.EINVAL and box_call(okb, 3) == _lib.EINVAL and box_call(okb, out=null) == _lib.EINVAL
    for bad in (box_problem(cells=(ctypes.c_int32 * 3)(4, 6, 3)), box_problem(r_cut=0.3), box_problem(alpha=float("nan")),
                box_problem(box=(ctypes.c_double * 6)(1.0, 0.0, -1.3, 0.0, 0.0, 0.8))):
        assert box_call(bad) == _lib.EINVAL and _lib.last_error().startswith("Input mismatch")
    assert box_call(box_problem(num_points=0)) == _lib.OK

    inv = (ctypes.c_double * 6)(1, 0, 1, 0, 0, 1)

    def spectral(N=8, B=1, C=1, order=2, band=one, coeffs=one, inv=inv, out=one):
        return lib.nfft_hip_ewald_dipole_spectral(N, B, C, order, band, coeffs, inv, out, null)

    for kw in (dict(order=0), dict(order=3), dict(N=7), dict(N=0), dict(B=0), dict(C=-1), dict(N=2048, C=1), dict(band=null),
               dict(coeffs=null), dict(out=null), dict(inv=None), dict(inv=(ctypes.c_double * 6)(1, 0, -1, 0, 0, 1))):
        assert spectral(**kw) == _lib.EINVAL and _lib.last_error().startswith("Input mismatch"), kw
    assert spectral(C=0) == _lib.OK


def test_kernel_resource_usage():
    """exactly the twelve instantiations <CC, ORDER, BOX> of the pair kernel and the two of the spectral kernel, each without
    scratch and without spills (the library's own flags); the tile of <4, 2, BOX> is 4 KiB of positions and 16 KiB of values
    (VGPRs and occupancy are recorded in DESIGN.md section 7l, not gated)"""
    from resource_usage import resource_usage
    usage = resource_usage("ewald_dipole.hip")
    by, spectral = {}, set()
    for name, u in usage.items():
        m = re.search(r"ewald_dipole_near_kernelILi(\d)ELi(\d)ELb(\d)EE", name)
        if m:
            by[(int(m.group(1)), int(m.group(2)), int(m.group(3)))] = u
        else:
            m = re.search(r"ewald_dipole_spectral_kernelILi(\d)EE", name)
            assert m, name  # (nothing else in that file)
            spectral.add(int(m.group(1)))
        assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
    assert set(by) == {(cc, o, box) for cc in (1, 2, 4) for o in (1, 2) for box in (0, 1)} and spectral == {1, 2}
    assert len(usage) == 14
    for key, u in sorted(by.items()):
        print(key, "VGPRs %d occupancy %d LDS %d" % (u["VGPRs"], u["Occupancy"], u["LDS Size"]))
        assert u["LDS Size"] == 4096 + 4096 * key[0]
