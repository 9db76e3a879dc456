"""CPU tests of the periodic Stokeslet sum (nfft_ewald_stokeslet): the float64 restatement
tests/stokeslet_ref.py against itself (two splittings, Hasimoto's constant, the trace of G, symmetry, finite differences), against
the mistakes a pair sweep can make and against the exact transforms of oracle/ndft.py; stokeslet_splitting against the
converged sum; the exports, schemas and refusals of the Python layer; the C ABI; the registers of the kernels."""
import ctypes
import math
import re

import numpy as np
import pytest
import torch

import dispersion_ref as dr
import stokeslet_ref as sr
from conftest import rel_l2
from ewald_box_ref import O, T
from oracle import ndft

BOXES = {"cube": None, "T": T, "O": O}
HASIMOTO = 2.8372974795  # the simple-cubic lattice constant of Hasimoto (1959): u = -(4/3) x this x f for one force per unit cube


def _random_forces(seed, n=12, cols=()):
    rng = np.random.default_rng(seed)
    return rng.random((n, 3)) - 0.5, rng.standard_normal((n, 3) + cols)


@pytest.mark.parametrize("box", ["cube", "T"])
def test_sum_does_not_depend_on_alpha(box):
    s, f = _random_forces(1, cols=(2,))
    terms = []
    for alpha in (5.0, 6.0):  # (both converged over 5^3 images and |k|_inf <= 14, in T too: e^(-pi^2 kappa^2 / alpha^2) < 1e-15)
        parts = (sr.near(f, s, BOXES[box], None, alpha, None, nimg=2), sr.far(f, s, BOXES[box], None, alpha, kmax=14),
                 sr.terms(f, 12, alpha))
        terms.append([sum(p) for p in zip(*parts)])
    for what, x, y in zip(("u", "G"), *terms):
        print("near + far + terms in %s at alpha = 5 and 6: %s rel_l2 %.3e" % (box, what, rel_l2(x, y)))
        assert rel_l2(x, y) <= 1e-12


def test_hasimoto_constant():
    f = np.array([[0.3, -1.1, 0.7]])
    u, G = sr.converged(f, np.array([[0.1, -0.2, 0.35]]), None)
    print("one force in the unit cube: u / f = %s" % (u / f))
    assert np.abs(u + (4.0 / 3.0) * HASIMOTO * f).max() <= 1e-9
    assert np.abs(G).max() <= 1e-9  # (the lattice of images is symmetric about the source)


@pytest.mark.parametrize("box", ["cube", "T", "O"])
def test_velocity_gradient_is_traceless(box):
    s, f = _random_forces(5)
    G = sr.converged(f, s, BOXES[box])[1]
    tr = G[:, 0, 0] + G[:, 1, 1] + G[:, 2, 2]
    print("tr G in %s: %.3e of |G|" % (box, np.abs(tr).max() / np.abs(G).max()))
    assert np.abs(tr).max() <= 1e-12 * np.abs(G).max()
    assert np.abs(G - G.transpose(0, 2, 1)).max() >= 1e-3 * np.abs(G).max()  # (and G is not symmetric)


@pytest.mark.parametrize("box", ["cube", "T"])
def test_operator_is_symmetric(box):
    s, f = _random_forces(6)
    g = _random_forces(7)[1]
    uf, ug = sr.converged(f, s, BOXES[box], order=1)[0], sr.converged(g, s, BOXES[box], order=1)[0]
    assert abs((g * uf).sum() - (f * ug).sum()) <= 1e-12 * np.abs(g * uf).sum()


@pytest.mark.parametrize("box", ["cube", "T"])
def test_gradient_is_the_derivative_and_gives_dL_dpos(box):
    """G_ab = d u_a / d x_b at a probe that carries no force, and dL/dpos of L = sum g . u[f] by the formula of section 7m, both
    against central differences (h = 1e-5: O(h^2) truncation and 1e-16 / h rounding are both far below 1e-6 of the values)"""
    A = BOXES[box]
    inv = np.linalg.inv(np.eye(3) if A is None else A)
    s, f = _random_forces(2)
    g = _random_forces(3)[1]
    h = 1e-5

    def moved(i, b, sign):
        e = np.zeros(3)
        e[b] = sign * h
        x = s.copy()
        x[i] += e @ inv
        return x

    f0 = f.copy()
    f0[0] = 0.0
    G = sr.converged(f0, s, A)[1]
    for b in range(3):
        up, um = (sr.converged(f0, moved(0, b, sign), A, order=1)[0] for sign in (1, -1))
        assert np.abs((up[0] - um[0]) / (2 * h) - G[0, :, b]).max() <= 1e-6 * np.abs(G[0]).max()
    want = sr.position_gradient(f, g, sr.converged(f, s, A)[1], sr.converged(g, s, A)[1])
    for i, b in ((0, 0), (5, 1), (11, 2)):
        L = [(g * sr.converged(f, moved(i, b, sign), A, order=1)[0]).sum() for sign in (1, -1)]
        print("dL/dpos[%d, %d] in %s: formula %.9e, differences %.9e" % (i, b, box, want[i, b], (L[0] - L[1]) / (2 * h)))
        assert abs((L[0] - L[1]) / (2 * h) - want[i, b]) <= 1e-6 * np.abs(want).max()


@pytest.mark.parametrize("box", ["cube", "T"])
def test_spectral_table_composes_the_far_part(box):
    """the far part as the operators compose it -- adjoint transform of the forces, the table, forward transform -- is the
    dense far sum (exact transforms of oracle/ndft.py in float64): the sign of the rows of G is the transforms'"""
    A = BOXES[box]
    s, f = _random_forces(7, n=20, cols=(2,))
    batch = (np.arange(20) >= 8).astype(np.int64)
    N = 8
    band = ndft.ndft_adjoint(f.reshape(20, 6), s, batch, N=N).reshape(2, N, N, N, 3, 2)
    spectra = np.einsum("xyzsr,bxyzrc->bxyzsc", sr.spectral_table(A, 5.0, N), band)
    got = ndft.ndft_forward(spectra.reshape(2, N, N, N, 24), s, batch).real.reshape(20, 12, 2)
    u, G = sr.far(f, s, A, batch, 5.0, N)
    assert rel_l2(got[:, :3], u) <= 1e-12 and rel_l2(got[:, 3:].reshape(20, 3, 3, 2), G) <= 1e-12


# (alpha, r_c) of the GPU near-sweep tests: alpha r_c ~ 1.5, G = 3, 4, 8 cells per axis
NEAR_CASES = [(5.0, 0.3), (6.0, 0.25), (12.0, 0.12)]


@pytest.mark.parametrize("alpha,r_c", NEAR_CASES)
def test_near_sum_is_sensitive_to_mistakes(alpha, r_c):
    """On the points of the GPU near-sweep test five mistakes of a pair sweep each move some output by at least ten times the
    gate that the device run is held to (tests/test_gpu_stokeslet.py: max(4 x the float32 emulation's error, the committed
    figure of the Coulomb field loop) per quantity): the -g term dropped, the m delta_ab term dropped, the B_2 term dropped, no
    wrap, a cut at 0.95 r_c."""
    from test_gpu_ewald import NEAR_TOL
    x = sr.near_points()
    f = sr.near_forces(1, 512, ())
    ref = sr.near(f, x, None, None, alpha, r_c)
    emu = sr.near_f32(f, x, None, None, alpha, r_c)
    gates = [sr.near_gate(w, e, r, NEAR_TOL["field"])[0] for w, e, r in zip("uG", emu, ref)]
    print("(%g, %g) gates: u %.3e, G %.3e" % ((alpha, r_c) + tuple(gates)))
    for what, kw, rc in (("no -g", dict(minus_g=False), r_c), ("no m delta", dict(mdelta=False), r_c), ("no B_2", dict(b2=False), r_c),
                         ("no wrap", dict(wrap=False), r_c), ("0.95 r_c", {}, 0.95 * r_c)):
        moved = [rel_l2(a, b) for a, b in zip(sr.near(f, x, None, None, alpha, rc, **kw), ref)]
        print("(%g, %g) %s: u moves by %.3e, G by %.3e" % ((alpha, r_c, what) + tuple(moved)))
        assert max(m / g for m, g in zip(moved, gates)) >= 10.0


def test_float32_emulation_is_float32():
    x = sr.near_points()
    f = sr.near_forces(2, 512, (2,))
    ref, emu = sr.near(f, x, T, None, 6.0, 0.25), sr.near_f32(f, x, T, None, 6.0, 0.25)
    for what, a, b in zip(("u", "G"), emu, ref):
        e = rel_l2(a.astype(np.float64), b)
        print("float32 emulation in T at (6, 0.25): %s rel_l2 %.3e" % (what, e))
        assert a.dtype == np.float32 and 1e-9 < e < 1e-5  # (float32 indeed, and nothing worse)


def _cluster():
    """the 4^3 cluster across the box corner of the dipole tests' converged-sum case, with forces"""
    s = dr.jittered_lattice(np.random.default_rng(9), 4, 0.1, 0.02, centre=0.45).reshape(-1, 3)
    return s, sr.near_forces(10, 64, ())


_CONVERGED = {}


def _converged_cluster(box):
    if box not in _CONVERGED:
        s, f = _cluster()
        _CONVERGED[box] = sr.converged(f, s, BOXES[box])
    return _CONVERGED[box]


@pytest.mark.parametrize("box", ["cube", "T", "O"])
@pytest.mark.parametrize("tol", [1e-3, 1e-5])
def test_stokeslet_splitting_meets_its_tolerance(box, tol):
    """alpha and the bandwidth of stokeslet_splitting(tol, r_cut): the truncated algorithm in float64 is within tol (relative
    l2) of the converged sum, for u and for G"""
    import torch_nfft_amd as tn
    A = BOXES[box]
    r_cut = 0.25 if box == "O" else 0.3
    sp = tn.stokeslet_splitting(tol, r_cut, box=None if A is None else torch.from_numpy(A), device="cpu")
    assert isinstance(sp, tn.EwaldSplitting) and sp.r_cut == r_cut and sp.bandwidth % 2 == 0
    s, f = _cluster()
    got = sr.exact_algorithm(f, s, A, None, sp.alpha, sp.r_cut, sp.bandwidth)
    for what, x, y in zip(("u", "G"), got, _converged_cluster(box)):
        err = rel_l2(x, y)
        print("stokeslet_splitting(%g, %g) in %s: alpha %.4f, N %d, %s rel_l2 %.3e = %.3f tol"
              % (tol, r_cut, box, sp.alpha, sp.bandwidth, what, err, err / tol))
        assert err <= tol


def test_stokeslet_coeffs():
    import torch_nfft_amd as tn
    for box in ("cube", "T"):
        A = BOXES[box]
        sp = tn.EwaldSplitting(6.0, 0.25, 16, box=None if A is None else torch.from_numpy(A), device="cpu")
        c = sp.stokeslet_coeffs
        assert c.dtype == torch.float32 and c.shape == (16, 16, 16) and c is sp.stokeslet_coeffs
        want = 0.5 * np.trace(sr.spectral_table(A, 6.0, 16, order=1).real, axis1=3, axis2=4)  # tr (c_k P) = 2 c_k
        assert rel_l2(c.numpy().astype(np.float64), want) <= 1e-7
        assert float(c[8, 8, 8]) == 0.0 and not c[0].any() and not c[:, 0].any() and not c[:, :, 0].any()


def test_exports_schemas_and_refusals():
    import torch_nfft
    import torch_nfft_amd as tn
    from torch_nfft_amd import _lib
    assert _lib.ABI_VERSION == 7
    for name in ("nfft_ewald_stokeslet", "nfft_ewald_stokeslet_power", "stokeslet_splitting"):
        assert name in tn.__all__ and getattr(torch_nfft, name) is getattr(tn, name)
    assert torch_nfft.stokeslet is tn.stokeslet
    s = str(torch.ops.torch_nfft._nfft_ewald_stokeslet_near.default._schema)
    assert s == ("torch_nfft::_nfft_ewald_stokeslet_near(Tensor pos, Tensor f, Tensor? batch, float[] box, float alpha, "
                 "float r_cut, int order) -> Tensor")
    s = str(torch.ops.torch_nfft._nfft_ewald_stokeslet_spectral.default._schema)
    assert s == "torch_nfft::_nfft_ewald_stokeslet_spectral(Tensor band, Tensor coeffs, float[] box, int order) -> Tensor"
    sp = tn.EwaldSplitting(6.0, 0.3, 16, device="cpu")
    spb = tn.EwaldSplitting(6.0, 0.25, 16, box=[1.0, 1.3, 0.8], device="cpu")
    f, pos = torch.zeros(5, 3), torch.zeros(5, 3)
    with pytest.raises(RuntimeError, match="torch_nfft._nfft_ewald_stokeslet_near is currently only implemented for GPU tensors"):
        tn.ops.nfft_ewald_stokeslet_near(pos, f, None, (), 6.0, 0.3, 2)
    with pytest.raises(RuntimeError, match="torch_nfft._nfft_ewald_stokeslet_near is currently only implemented for GPU tensors"):
        tn.ops.nfft_ewald_stokeslet_near(pos, f, None, spb.box6, 6.0, 0.25, 1)
    with pytest.raises(RuntimeError, match="torch_nfft._nfft_ewald_stokeslet_spectral is currently only implemented for GPU tensors"):
        tn.ops.nfft_ewald_stokeslet_spectral(torch.zeros(1, 16, 16, 16, 3, dtype=torch.complex64), sp.stokeslet_coeffs, (), 2)
    for fn in (tn.nfft_ewald_stokeslet, tn.nfft_ewald_stokeslet_power):
        with pytest.raises(TypeError, match="EwaldSplitting"):
            fn(f, pos)
        with pytest.raises(TypeError, match="EwaldSplitting"):
            fn(f, pos, splitting=tn.DispersionSplitting(6.0, 0.3, 16, device="cpu"))
        with pytest.raises(ValueError, match="complex"):
            fn(f.to(torch.complex64), pos, splitting=sp)
        with pytest.raises(ValueError, match="float32"):
            fn(f.double(), pos, splitting=sp)
        with pytest.raises(ValueError, match="three-dimensional"):
            fn(f, torch.zeros(5, 2), splitting=sp)
        with pytest.raises(ValueError, match="f must be"):
            fn(torch.zeros(5, 2), pos, splitting=sp)
        with pytest.raises(ValueError, match="f must be"):
            fn(torch.zeros(4, 3), pos, splitting=sp)
        with pytest.raises(ValueError, match="fractional"):
            fn(f, pos, splitting=sp, fractional=True)
        with pytest.raises(AssertionError, match="batch"):
            fn(f, pos, torch.zeros(5, requires_grad=True), splitting=sp)
        for kw in (dict(splitting=sp), dict(splitting=spb), dict(splitting=spb, fractional=True)):
            with pytest.raises(RuntimeError, match="is currently only implemented for GPU tensors"):
                fn(f, pos, **kw)
    with pytest.raises(RuntimeError, match="is currently only implemented for GPU tensors"):
        tn.nfft_ewald_stokeslet(f, pos, splitting=sp, gradient=True)
    with pytest.raises(ValueError, match="tol"):
        tn.stokeslet_splitting(2.0, 0.3, device="cpu")
    with pytest.raises(ValueError, match="r_cut"):
        tn.stokeslet_splitting(1e-3, 0.3, box=[1.0, 1.3, 0.8], device="cpu")


def test_c_abi_validation_without_gpu():
    """the three symbols; the near entry points validate as their dipole twins do, refuse an order other than 1 or 2 and take
    the workspace that the shared size functions report"""
    from torch_nfft_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 7 and lib.nfft_hip_abi_version() == 7
    for name in ("nfft_hip_ewald_stokeslet_near", "nfft_hip_ewald_stokeslet_near_box", "nfft_hip_ewald_stokeslet_spectral"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(256)  # (never dereferenced: the checks come first)

    def problem(**kw):
        f = dict(cells_per_axis=4, with_field=1, num_points=1000, num_columns=2, batch_size=1, alpha=6.0, r_cut=0.25)
        f.update(kw)
        return _lib.EwaldProblem(**f)

    def call(q, order=2, ws=null, nbytes=0, out=one, points=one, xs=one):
        return lib.nfft_hip_ewald_stokeslet_near(ctypes.byref(q), points, xs, one, one, order, out, ws, nbytes, null)

    ok = problem()
    need = lib.nfft_hip_ewald_near_workspace_bytes(ctypes.byref(ok))
    assert need > 0
    for order in (1, 2):
        assert call(ok, order) == _lib.EWORKSPACE and _lib.last_error() == "workspace too small"
        assert call(ok, order, one, need - 1) == _lib.EWORKSPACE
    for order in (0, 3, -1):
        assert call(ok, order) == _lib.EINVAL and _lib.last_error() == "Input mismatch: order must be 1 or 2"
    assert call(ok, out=null) == _lib.EINVAL and call(ok, points=null) == _lib.EINVAL and call(ok, xs=null) == _lib.EINVAL
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
        return lib.nfft_hip_ewald_stokeslet_near_box(ctypes.byref(q), one, one, one, one, order, out, ws, nbytes, null)

    okb = box_problem()
    needb = lib.nfft_hip_ewald_near_box_workspace_bytes(ctypes.byref(okb))
    assert needb > 0
    assert box_call(okb) == _lib.EWORKSPACE and box_call(okb, 1, one, needb - 1) == _lib.EWORKSPACE
    assert box_call(okb, 0) == _lib.EINVAL and box_call(okb, 3) == _lib.EINVAL and box_call(okb, out=null) == _lib.EINVAL
    for bad in (box_problem(cells=(ctypes.c_int32 * 3)(4, 6, 3)), box_problem(r_cut=0.3), box_problem(alpha=float("nan"))):
        assert box_call(bad) == _lib.EINVAL and _lib.last_error().startswith("Input mismatch")
    assert box_call(box_problem(num_points=0)) == _lib.OK and box_call(box_problem(num_columns=0)) == _lib.OK

    inv = (ctypes.c_double * 6)(1, 0, 1, 0, 0, 1)

    def spectral(N=8, B=1, C=1, order=2, band=one, coeffs=one, inv=inv, out=one):
        return lib.nfft_hip_ewald_stokeslet_spectral(N, B, C, order, band, coeffs, inv, out, null)

    for kw in (dict(order=0), dict(order=3), dict(N=7), dict(N=0), dict(B=0), dict(C=-1), dict(N=2048, C=1), dict(band=null),
               dict(coeffs=null), dict(out=null), dict(inv=None), dict(inv=(ctypes.c_double * 6)(1, 0, -1, 0, 0, 1))):
        assert spectral(**kw) == _lib.EINVAL and _lib.last_error().startswith("Input mismatch"), kw
    assert spectral(C=0) == _lib.OK


def test_kernel_resource_usage():
    """exactly the twelve instantiations <CC, ORDER, BOX> of the pair kernel and the two of the spectral kernel, each without
    scratch and without spills (the library's own flags); the tile of <4, 2, BOX>, the one with 48 sums, is 4 KiB of positions
    and 16 KiB of forces (VGPRs and occupancy are recorded in DESIGN.md section 7m, not gated)"""
    from resource_usage import resource_usage
    usage = resource_usage("ewald_stokeslet.hip")
    by, spectral = {}, set()
    for name, u in usage.items():
        m = re.search(r"ewald_stokeslet_near_kernelILi(\d)ELi(\d)ELb(\d)EE", name)
        if m:
            by[(int(m.group(1)), int(m.group(2)), int(m.group(3)))] = u
        else:
            m = re.search(r"ewald_stokeslet_spectral_kernelILi(\d)EE", name)
            assert m, name  # (nothing else in that file)
            spectral.add(int(m.group(1)))
        assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
    assert set(by) == {(cc, o, box) for cc in (1, 2, 4) for o in (1, 2) for box in (0, 1)} and spectral == {1, 2}
    assert len(usage) == 14
    for key, u in sorted(by.items()):
        print(key, "VGPRs %d occupancy %d LDS %d" % (u["VGPRs"], u["Occupancy"], u["LDS Size"]))
        assert u["LDS Size"] == 4096 + 4096 * key[0]
