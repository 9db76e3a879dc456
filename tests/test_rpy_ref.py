"""CPU tests of the periodic Rotne-Prager-Yamakawa sum (nfft_ewald_rpy): the float64 restatement
tests/rpy_ref.py against itself (two splittings, the periodic self mobility of one sphere, continuity at contact, finite
differences, a symmetric positive definite mobility) and against the mistakes a pair sweep can make; rpy_splitting against the
converged sum; rpy_coeffs; the exports, schema and refusals of the Python layer; the C ABI; the registers of the kernels."""
import ctypes
import math
import re

import numpy as np
import pytest
import torch

import dispersion_ref as dr
import rpy_ref as rr
import stokeslet_ref as sr
from conftest import rel_l2
from ewald_box_ref import O, T

BOXES = {"cube": None, "T": T, "O": O}
HASIMOTO = 2.8372974795  # the simple-cubic lattice constant of Hasimoto (1959)


def _spheres(seed, n=12, cols=(), radius=0.05, box="cube"):
    """n random fractional points of which 1 is moved to 1.1 a from 0, 3 to 0.5 a from 2 and 5 to 1.9 a from 4 in the metric of
    the box (three overlapping pairs), with forces"""
    rng = np.random.default_rng(seed)
    s = rng.random((n, 3)) - 0.5
    for i, sep in ((0, 1.1), (2, 0.5), (4, 1.9)):
        e = rng.standard_normal(3)
        s[i + 1] = s[i] + sep * radius * e / np.linalg.norm(e) @ np.linalg.inv(rr._box(BOXES[box]))
    return s, rng.standard_normal((n, 3) + cols)


@pytest.mark.parametrize("box", ["cube", "T"])
def test_sum_does_not_depend_on_alpha(box):
    s, f = _spheres(1, cols=(2,), box=box)
    A = BOXES[box]
    assert 3 <= _overlaps(s, A, 0.05) <= 6
    got = [rr.converged(f, s, A, 0.05, alpha=alpha) for alpha in (5.0, 6.0)]
    for what, x, y in zip(("u", "G"), *got):
        print("near + far + terms in %s at alpha = 5 and 6: %s rel_l2 %.3e" % (box, what, rel_l2(x, y)))
        assert rel_l2(x, y) <= 1e-12


def _overlaps(s, A, radius):
    """the number of pairs closer than 2 a"""
    ds = s[:, None, :] - s[None, :, :]
    d = (ds - np.rint(ds)) @ rr._box(A)
    r = np.sqrt((d * d).sum(-1))
    return int(((r > 0) & (r < 2 * radius)).sum()) // 2


@pytest.mark.parametrize("radius", [0.05, 0.1])
def test_single_sphere_mobility(radius):
    """one sphere in the unit cube: u = (4 / (3 a)) (1 - 2.8372974795 a + (4 pi / 3) a^3) f, Hasimoto's periodic self mobility,
    and G = 0 (the lattice of images is symmetric about the sphere)"""
    f = np.array([[0.3, -1.1, 0.7]])
    u, G = rr.converged(f, np.array([[0.1, -0.2, 0.35]]), None, radius)
    want = 4.0 / (3.0 * radius) * (1.0 - HASIMOTO * radius + 4.0 * math.pi / 3.0 * radius ** 3)
    print("one sphere of radius %g in the unit cube: u / f = %s, want %.10f" % (radius, u / f, want))
    assert np.abs(u - want * f).max() <= 1e-9 * want
    assert np.abs(G).max() <= 1e-9


@pytest.mark.parametrize("form", rr.FORMS)
def test_weights_are_continuous_at_contact(form):
    """W1, W2, D1 and D2 on the two sides of r = 2 a (R is C^1 there): the jump is of the order of the step"""
    a, alpha = 0.03, 6.0
    h = 1e-9
    lo, hi = rr.weights(np.array([2 * a - h]), alpha, a, form=form), rr.weights(np.array([2 * a + h]), alpha, a, form=form)
    off = rr.weights(np.array([2 * a - h]), alpha, a, overlap=False)
    for name, x, y, z in zip(("W1", "W2", "D1", "D2"), lo, hi, off):
        print("%s at 2 a -+ 1e-9 (%s): %.9e %.9e" % (name, form, x[0], y[0]))
        assert abs(x[0] - y[0]) <= 1e-6 * abs(y[0])
        assert abs(x[0] - z[0]) <= 1e-6 * abs(y[0])  # (the branch adds nothing at contact)
    # and the two ways of writing the branch are the same numbers
    r = np.linspace(0.2 * a, 2 * a, 50)
    for x, y in zip(rr.weights(r, alpha, a), rr.weights(r, alpha, a, form="far")):
        assert np.abs(x - y).max() <= 1e-10 * np.abs(x).max()
    # the overlap form itself: W1 + r^2 W2 of the unscreened tensor at alpha -> 0 is (4 / (3 a)) (1 - 3 r / (16 a))
    W1, W2, _, _ = rr.weights(r, 1e-4, a)
    assert np.abs(W1 + r * r * W2 - 4 / (3 * a) * (1 - 3 * r / (16 * a))).max() <= 1e-3


@pytest.mark.parametrize("box", ["cube", "T"])
def test_gradient_is_the_derivative_and_gives_dL_dpos(box):
    """G_ab = d u_a / d x_b at a probe that carries no force -- one with an overlapping partner (0, at 1.1 a; 3, at a / 2) and one
    without (8) -- and dL/dpos of L = sum g . u[f], both against central differences (h = 1e-5)"""
    A = BOXES[box]
    inv = np.linalg.inv(np.eye(3) if A is None else A)
    a = 0.05
    s, f = _spheres(2, box=box)
    g = _spheres(3)[1]
    h = 1e-5

    def moved(i, b, sign):
        e = np.zeros(3)
        e[b] = sign * h
        x = s.copy()
        x[i] += e @ inv
        return x

    for i in (0, 3, 8):
        f0 = f.copy()
        f0[i] = 0.0
        G = rr.converged(f0, s, A, a)[1]
        for b in range(3):
            up, um = (rr.converged(f0, moved(i, b, sign), A, a, order=1)[0] for sign in (1, -1))
            err = np.abs((up[i] - um[i]) / (2 * h) - G[i, :, b]).max() / np.abs(G[i]).max()
            print("G[%d, :, %d] in %s against differences: %.3e" % (i, b, box, err))
            assert err <= 1e-6
    want = rr.position_gradient(f, g, rr.converged(f, s, A, a)[1], rr.converged(g, s, A, a)[1])
    for i, b in ((0, 0), (3, 1), (11, 2)):
        L = [(g * rr.converged(f, moved(i, b, sign), A, a, order=1)[0]).sum() for sign in (1, -1)]
        print("dL/dpos[%d, %d] in %s: formula %.9e, differences %.9e" % (i, b, box, want[i, b], (L[0] - L[1]) / (2 * h)))
        assert abs((L[0] - L[1]) / (2 * h) - want[i, b]) <= 1e-6 * np.abs(want).max()


@pytest.mark.parametrize("box", ["cube", "T"])
def test_mobility_is_symmetric_positive_definite(box):
    """12 spheres, three overlapping pairs among them: the 36 x 36 matrix of the converged sum.  The Stokeslet sum's own matrix
    on the same points is not positive definite: that is what the sphere terms are for."""
    A = BOXES[box]
    s, _ = _spheres(4, box=box)
    assert _overlaps(s, A, 0.05) >= 3
    M = rr.mobility(s, A, 0.05)
    eig = np.linalg.eigvalsh(0.5 * (M + M.T))
    print("mobility in %s: asymmetry %.3e, eigenvalues in [%.4f, %.4f]" % (box, np.abs(M - M.T).max(), eig[0], eig[-1]))
    assert np.abs(M - M.T).max() <= 1e-12 * np.abs(M).max()
    assert eig[0] > 0.0
    f = np.eye(36).reshape(12, 3, 36)
    S = sr.converged(f, s, A, order=1)[0].reshape(36, 36)
    assert np.linalg.eigvalsh(0.5 * (S + S.T))[0] < 0.0


# (alpha, r_c) of the GPU near-sweep tests
NEAR_CASES = [(5.0, 0.3), (6.0, 0.25), (12.0, 0.12)]


@pytest.mark.parametrize("alpha,r_c", NEAR_CASES)
def test_near_sum_is_sensitive_to_mistakes(alpha, r_c):
    """Four mistakes each move some output by at least ten times the gate that the device run is held to
    (tests/test_gpu_rpy.py: max(4 x the float32 emulation's error, the committed figure of the Coulomb field loop) per
    quantity): on the points of the near-sweep test with a = 0.03 the a^2 term of W2 and D2 dropped and no wrap; on the dimers
    with a = 0.02 the overlap branch dropped; and in the whole sum the Stokeslet's self term kept beside 4 / (3 a)."""
    from test_gpu_ewald import NEAR_TOL
    x = rr.near_points()
    f = rr.near_forces(1, 512, ())
    a = 0.03
    ref = rr.near(f, x, None, None, alpha, r_c, a)
    emu = rr.near_f32(f, x, None, None, alpha, r_c, a)
    gates = [rr.near_gate(w, e, r, NEAR_TOL["field"])[0] for w, e, r in zip("uG", emu, ref)]
    print("(%g, %g) gates: u %.3e, G %.3e" % ((alpha, r_c) + tuple(gates)))
    for what, kw in (("no a^2 term", dict(a2_term=False)), ("no wrap", dict(wrap=False))):
        moved = [rel_l2(p, q) for p, q in zip(rr.near(f, x, None, None, alpha, r_c, a, **kw), ref)]
        print("(%g, %g) %s: u moves by %.3e, G by %.3e" % ((alpha, r_c, what) + tuple(moved)))
        assert max(m / g for m, g in zip(moved, gates)) >= 10.0
    # the self term: its mistake against the whole sum's near part (the gate is relative to it)
    wrong = rr.self_coefficient(alpha, a, a2_term=False) - rr.self_coefficient(alpha, a)
    moved = abs(wrong) * np.linalg.norm(f) / np.linalg.norm(ref[0])
    print("(%g, %g) Stokeslet self term: u moves by %.3e of the near part" % (alpha, r_c, moved))
    assert moved >= 10.0 * gates[0]
    xd, _ = rr.dimers()
    ref = rr.near(f, xd, None, None, alpha, r_c, 0.02)
    emu = rr.near_f32(f, xd, None, None, alpha, r_c, 0.02)
    gates = [rr.near_gate(w, e, r, NEAR_TOL["field"])[0] for w, e, r in zip("uG", emu, ref)]
    moved = [rel_l2(p, q) for p, q in zip(rr.near(f, xd, None, None, alpha, r_c, 0.02, overlap=False), ref)]
    print("(%g, %g) dimers, no overlap branch: u moves by %.3e, G by %.3e; gates %.3e, %.3e" % ((alpha, r_c) + tuple(moved + gates)))
    assert min(m / g for m, g in zip(moved, gates)) >= 10.0


def test_float32_emulation_and_the_two_overlap_forms():
    """the emulation is float32 and nothing worse; at r = a / 2 the far-kernel form of the overlap branch (the kernel's) is
    better than the direct one in every weight (DESIGN.md section 7n records the figures)"""
    x = rr.near_points()
    f = rr.near_forces(2, 512, (2,))
    ref, emu = rr.near(f, x, T, None, 6.0, 0.25, 0.03), rr.near_f32(f, x, T, None, 6.0, 0.25, 0.03)
    for what, p, q in zip(("u", "G"), emu, ref):
        e = rel_l2(p.astype(np.float64), q)
        print("float32 emulation in T at (6, 0.25), a = 0.03: %s rel_l2 %.3e" % (what, e))
        assert p.dtype == np.float32 and 1e-9 < e < 1e-5
    a, alpha = 0.02, 5.0
    r = (0.5 * a * (1.0 + 0.05 * (np.random.default_rng(3).random(4000) - 0.5))).astype(np.float32)
    want = rr.weights(r.astype(np.float64), alpha, a)
    errs = {form: [rel_l2(w.astype(np.float64), v) for w, v in zip(rr.weights(r, alpha, a, form=form), want)] for form in rr.FORMS}
    for form in rr.FORMS:
        print("float32 at r = a / 2, a = 0.02, alpha = 5, %-6s: W1 %.2e W2 %.2e D1 %.2e D2 %.2e" % ((form,) + tuple(errs[form])))
    assert all(x < y for x, y in zip(errs["far"], errs["direct"]))
    assert rr.near_f32.__defaults__[-1] == "far"


def _cluster():
    """the 4^3 cluster across the box corner of the Stokeslet tests' converged-sum case, with forces; a = 0.03 makes the
    closest of its pairs overlap"""
    s = dr.jittered_lattice(np.random.default_rng(9), 4, 0.1, 0.02, centre=0.45).reshape(-1, 3)
    return s, rr.near_forces(10, 64, ())


_CONVERGED = {}


def _converged_cluster(box, radius):
    if (box, radius) not in _CONVERGED:
        s, f = _cluster()
        _CONVERGED[(box, radius)] = rr.converged(f, s, BOXES[box], radius)
    return _CONVERGED[(box, radius)]


@pytest.mark.parametrize("box", ["cube", "T", "O"])
@pytest.mark.parametrize("tol", [1e-3, 1e-5])
def test_rpy_splitting_meets_its_tolerance(box, tol):
    """alpha and the bandwidth of rpy_splitting(tol, r_cut, radius): the truncated algorithm in float64 is within tol (relative
    l2) of the converged sum, for u and for G"""
    import torch_nfft_amd as tn
    A = BOXES[box]
    r_cut = 0.25 if box == "O" else 0.3
    radius = 0.035
    sp = tn.rpy_splitting(tol, r_cut, radius, box=None if A is None else torch.from_numpy(A), device="cpu")
    assert isinstance(sp, tn.EwaldSplitting) and sp.r_cut == r_cut and sp.bandwidth % 2 == 0
    s, f = _cluster()
    if box == "cube" and tol == 1e-3:
        assert _overlaps(s, A, radius) >= 1
    got = rr.exact_algorithm(f, s, A, None, sp.alpha, sp.r_cut, sp.bandwidth, radius)
    for what, x, y in zip(("u", "G"), got, _converged_cluster(box, radius)):
        err = rel_l2(x, y)
        print("rpy_splitting(%g, %g, %g) in %s: alpha %.4f, N %d, %s rel_l2 %.3e = %.3f tol"
              % (tol, r_cut, radius, box, sp.alpha, sp.bandwidth, what, err, err / tol))
        assert err <= tol


def test_rpy_coeffs():
    import torch_nfft_amd as tn
    for box in ("cube", "T"):
        A = BOXES[box]
        sp = tn.EwaldSplitting(6.0, 0.25, 16, box=None if A is None else torch.from_numpy(A), device="cpu")
        c = tn.rpy_coeffs(sp, 0.03)
        assert c.dtype == torch.float32 and c.shape == (16, 16, 16) and c is tn.rpy_coeffs(sp, 0.03)
        assert tn.rpy_coeffs(sp, 0.05) is not c and tn.rpy_coeffs(sp, 0.03) is c  # (one table per radius)
        want = 0.5 * np.trace(rr.spectral_table(A, 6.0, 16, 0.03, order=1).real, axis1=3, axis2=4)  # tr (c_k P) = 2 c_k
        assert rel_l2(c.numpy().astype(np.float64), want) <= 1e-7
        assert float(c[8, 8, 8]) == 0.0 and not c[0].any() and not c[:, 0].any() and not c[:, :, 0].any()
        assert torch.equal(c == 0, sp.stokeslet_coeffs == 0)
    # a table whose float32 Stokeslet coefficients underflow far out: the same exact zeros
    sp = tn.EwaldSplitting(2.0, 0.3, 32, device="cpu")
    assert int((sp.stokeslet_coeffs[1:, 1:, 1:] == 0).sum()) > 1
    assert torch.equal(tn.rpy_coeffs(sp, 0.1) == 0, sp.stokeslet_coeffs == 0)
    with pytest.raises(ValueError, match="radius"):
        tn.rpy_coeffs(sp, 0.0)
    with pytest.raises(TypeError, match="EwaldSplitting"):
        tn.rpy_coeffs(None, 0.1)


def test_spectral_table_composes_the_far_part():
    """the far part as the operators compose it -- adjoint transform, table, forward transform (exact ones in float64) -- is
    the dense far sum"""
    from oracle import ndft
    s, f = _spheres(7, n=20, cols=(2,))
    batch = (np.arange(20) >= 8).astype(np.int64)
    N = 8
    band = ndft.ndft_adjoint(f.reshape(20, 6), s, batch, N=N).reshape(2, N, N, N, 3, 2)
    spectra = np.einsum("xyzsr,bxyzrc->bxyzsc", rr.spectral_table(T, 5.0, N, 0.05), band)
    got = ndft.ndft_forward(spectra.reshape(2, N, N, N, 24), s, batch).real.reshape(20, 12, 2)
    u, G = rr.far(f, s, T, batch, 5.0, 0.05, N)
    assert rel_l2(got[:, :3], u) <= 1e-12 and rel_l2(got[:, 3:].reshape(20, 3, 3, 2), G) <= 1e-12


def test_exports_schemas_and_refusals():
    import torch_nfft
    import torch_nfft_amd as tn
    from torch_nfft_amd import _lib
    assert _lib.ABI_VERSION == 7
    for name in ("nfft_ewald_rpy", "nfft_ewald_rpy_power", "rpy_coeffs", "rpy_splitting"):
        assert name in tn.__all__ and getattr(torch_nfft, name) is getattr(tn, name)
    assert torch_nfft.rpy is tn.rpy
    s = str(torch.ops.torch_nfft._nfft_ewald_rpy_near.default._schema)
    assert s == ("torch_nfft::_nfft_ewald_rpy_near(Tensor pos, Tensor f, Tensor? batch, float[] box, float alpha, float r_cut, "
                 "float radius, int order) -> Tensor")
    sp = tn.EwaldSplitting(6.0, 0.3, 16, device="cpu")
    spb = tn.EwaldSplitting(6.0, 0.25, 16, box=[1.0, 1.3, 0.8], device="cpu")
    f, pos = torch.zeros(5, 3), torch.zeros(5, 3)
    with pytest.raises(RuntimeError, match="torch_nfft._nfft_ewald_rpy_near is currently only implemented for GPU tensors"):
        tn.ops.nfft_ewald_rpy_near(pos, f, None, (), 6.0, 0.3, 0.05, 2)
    with pytest.raises(RuntimeError, match="torch_nfft._nfft_ewald_rpy_near is currently only implemented for GPU tensors"):
        tn.ops.nfft_ewald_rpy_near(pos, f, None, spb.box6, 6.0, 0.25, 0.05, 1)
    for fn in (tn.nfft_ewald_rpy, tn.nfft_ewald_rpy_power):
        with pytest.raises(TypeError, match="EwaldSplitting"):
            fn(f, pos, radius=0.05)
        with pytest.raises(TypeError, match="EwaldSplitting"):
            fn(f, pos, splitting=tn.DispersionSplitting(6.0, 0.3, 16, device="cpu"), radius=0.05)
        with pytest.raises(ValueError, match="complex"):
            fn(f.to(torch.complex64), pos, splitting=sp, radius=0.05)
        with pytest.raises(ValueError, match="float32"):
            fn(f.double(), pos, splitting=sp, radius=0.05)
        with pytest.raises(ValueError, match="three-dimensional"):
            fn(f, torch.zeros(5, 2), splitting=sp, radius=0.05)
        with pytest.raises(ValueError, match="f must be"):
            fn(torch.zeros(5, 2), pos, splitting=sp, radius=0.05)
        with pytest.raises(ValueError, match="f must be"):
            fn(torch.zeros(4, 3), pos, splitting=sp, radius=0.05)
        with pytest.raises(ValueError, match="fractional"):
            fn(f, pos, splitting=sp, radius=0.05, fractional=True)
        with pytest.raises(AssertionError, match="batch"):
            fn(f, pos, torch.zeros(5, requires_grad=True), splitting=sp, radius=0.05)
        for bad in (None, 0.0, -0.1, float("nan"), 0.16):  # missing, not positive, 2 a > r_cut = 0.3
            with pytest.raises(ValueError, match="radius"):
                fn(f, pos, splitting=sp, radius=bad)
        with pytest.raises(ValueError, match="radius"):
            fn(f, pos, splitting=spb, radius=0.13)
        for kw in (dict(splitting=sp), dict(splitting=spb), dict(splitting=spb, fractional=True), dict(splitting=sp, radius=0.15)):
            kw.setdefault("radius", 0.05)
            with pytest.raises(RuntimeError, match="is currently only implemented for GPU tensors"):
                fn(f, pos, **kw)
    with pytest.raises(RuntimeError, match="is currently only implemented for GPU tensors"):
        tn.nfft_ewald_rpy(f, pos, splitting=sp, radius=0.05, gradient=True)
    with pytest.raises(ValueError, match="tol"):
        tn.rpy_splitting(2.0, 0.3, 0.05, device="cpu")
    with pytest.raises(ValueError, match="r_cut"):
        tn.rpy_splitting(1e-3, 0.3, 0.05, box=[1.0, 1.3, 0.8], device="cpu")
    for bad in (0.0, -1.0, 0.16):
        with pytest.raises(ValueError, match="radius"):
            tn.rpy_splitting(1e-3, 0.3, bad, device="cpu")
    assert tn.rpy.SAFETY == tn.stokeslet.SAFETY


def test_c_abi_validation_without_gpu():
    """the two symbols; they validate as their Stokeslet twins do, refuse an order other than 1 or 2 and a radius that is not
    finite, not positive or above r_cut / 2, all before any device access, and take the workspace that the shared size
    functions report"""
    from torch_nfft_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 7 and lib.nfft_hip_abi_version() == 7
    for name in ("nfft_hip_ewald_rpy_near", "nfft_hip_ewald_rpy_near_box"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(256)  # (never dereferenced: the checks come first)
    bad_radii = (0.0, -0.05, float("nan"), float("inf"), 0.126)

    def problem(**kw):
        f = dict(cells_per_axis=4, with_field=1, num_points=1000, num_columns=2, batch_size=1, alpha=6.0, r_cut=0.25)
        f.update(kw)
        return _lib.EwaldProblem(**f)

    def call(q, order=2, radius=0.05, ws=null, nbytes=0, out=one, points=one, xs=one):
        return lib.nfft_hip_ewald_rpy_near(ctypes.byref(q), points, xs, one, one, order, radius, out, ws, nbytes, null)

    ok = problem()
    need = lib.nfft_hip_ewald_near_workspace_bytes(ctypes.byref(ok))
    assert need > 0
    for order in (1, 2):
        assert call(ok, order) == _lib.EWORKSPACE and _lib.last_error() == "workspace too small"
        assert call(ok, order, ws=one, nbytes=need - 1) == _lib.EWORKSPACE
    assert call(ok, radius=0.125) == _lib.EWORKSPACE  # (2 a = r_cut is allowed)
    for order in (0, 3, -1):
        assert call(ok, order) == _lib.EINVAL and _lib.last_error() == "Input mismatch: order must be 1 or 2"
    for radius in bad_radii:
        assert call(ok, radius=radius) == _lib.EINVAL and _lib.last_error().startswith("Input mismatch:"), radius
        assert "radius" in _lib.last_error()
        assert call(problem(num_points=0), radius=radius) == _lib.EINVAL  # (before the early return too)
    assert call(ok, out=null) == _lib.EINVAL and call(ok, points=null) == _lib.EINVAL and call(ok, xs=null) == _lib.EINVAL
    for bad in (problem(cells_per_axis=2), problem(cells_per_axis=5), problem(with_field=2), problem(num_points=-1),
                problem(alpha=0.0), problem(r_cut=0.34, cells_per_axis=3), problem(batch_size=0)):
        assert call(bad) == _lib.EINVAL and _lib.last_error().startswith("Input mismatch")
    assert call(problem(num_points=0)) == _lib.OK and call(problem(num_columns=0)) == _lib.OK
    assert lib.nfft_hip_ewald_rpy_near(None, one, one, one, one, 2, 0.05, one, null, 0, null) == _lib.EINVAL

    def box_problem(**kw):
        f = dict(cells=(ctypes.c_int32 * 3)(4, 5, 3), with_field=1, num_points=1000, num_columns=2, batch_size=1, alpha=6.0,
                 r_cut=0.25, box=(ctypes.c_double * 6)(1.0, 0.0, 1.3, 0.0, 0.0, 0.8))
        f.update(kw)
        return _lib.EwaldBoxProblem(**f)

    def box_call(q, order=2, radius=0.05, ws=null, nbytes=0, out=one):
        return lib.nfft_hip_ewald_rpy_near_box(ctypes.byref(q), one, one, one, one, order, radius, out, ws, nbytes, null)

    okb = box_problem()
    needb = lib.nfft_hip_ewald_near_box_workspace_bytes(ctypes.byref(okb))
    assert needb > 0
    assert box_call(okb) == _lib.EWORKSPACE and box_call(okb, 1, ws=one, nbytes=needb - 1) == _lib.EWORKSPACE
    assert box_call(okb, 0) == _lib.EINVAL and box_call(okb, 3) == _lib.EINVAL and box_call(okb, out=null) == _lib.EINVAL
    for radius in bad_radii:
        assert box_call(okb, radius=radius) == _lib.EINVAL and "radius" in _lib.last_error(), radius
    for bad in (box_problem(cells=(ctypes.c_int32 * 3)(4, 6, 3)), box_problem(r_cut=0.3), box_problem(alpha=float("nan"))):
        assert box_call(bad) == _lib.EINVAL and _lib.last_error().startswith("Input mismatch")
    assert box_call(box_problem(num_points=0)) == _lib.OK and box_call(box_problem(num_columns=0)) == _lib.OK


def test_kernel_resource_usage():
    """exactly the twelve instantiations <CC, ORDER, BOX> of the pair kernel and nothing else in that file, each without scratch
    and without spills (the library's own flags); the tile is 4 KiB of positions and 4 KiB of forces per column (VGPRs and
    occupancy are recorded in DESIGN.md section 7n, not gated)"""
    from resource_usage import resource_usage
    usage = resource_usage("ewald_rpy.hip")
    by = {}
    for name, u in usage.items():
        m = re.search(r"ewald_rpy_near_kernelILi(\d)ELi(\d)ELb(\d)EE", name)
        assert m, name  # (nothing else in that file)
        by[(int(m.group(1)), int(m.group(2)), int(m.group(3)))] = u
        assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
    assert set(by) == {(cc, o, box) for cc in (1, 2, 4) for o in (1, 2) for box in (0, 1)}
    assert len(usage) == 12
    for key, u in sorted(by.items()):
        print(key, "VGPRs %d occupancy %d LDS %d" % (u["VGPRs"], u["Occupancy"], u["LDS Size"]))
        assert u["LDS Size"] == 4096 + 4096 * key[0]
