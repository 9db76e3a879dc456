"""GPU tests of the periodic Stokeslet sum: the wrapped pair sweep and the spectral step of
csrc/ewald_stokeslet.hip, and nfft_ewald_stokeslet / nfft_ewald_stokeslet_power with their gradients, against the float64
restatement tests/stokeslet_ref.py on the same float32 positions.  Modelled on tests/test_gpu_dipole.py, case for case.

The gates hold no numbers of their own.
* A pair sweep is held, per quantity (u, G), to rel_l2 <= max(4 x rel_l2(float32 emulation, float64), the committed figure of
  the Coulomb field loop): the emulation (stokeslet_ref.near_f32) is the number format's own rounding on these points, the
  committed figure (tests/test_gpu_ewald.py: NEAR_TOL["field"]) what the erfcf / __expf pair loop measured on this hardware,
  4 x the project's margin.  tests/test_stokeslet_ref.py shows that a dropped -g, m delta_ab or B_2 term, a missing wrap or a
  cut at 0.95 r_c each move some output by more than ten times that.
* The spectral kernel against the einsum of stokeslet_ref.spectral_table in torch complex64 on the device: rel_l2 <= 1e-6,
  the dipole spectral test's figure; the projection adds two roundings and |P rho| ~ sqrt(2/3) |rho|.
* The whole sum, per quantity: |device - algorithm| <= 2 e_far + gate_near |near|, where e_far is the absolute l2 error of the
  far part composed in the test from nfft_adjoint, a torch product and nfft_forward (the 2 covers the run-to-run scatter of the
  transforms' float atomics between that run and the function's own) and gate_near the pair sweep's gate.
* Against the converged sum, Hasimoto's constant and in the gradients the bounds are composed from these by the triangle and
  Cauchy-Schwarz inequalities.
Every case prints the terms of its gate beside the device's figure.
"""
import math

import numpy as np
import pytest
import torch

import dispersion_ref as dr
import stokeslet_ref as sr
from conftest import rel_l2
from ewald_box_ref import O, T
from test_gpu_ewald import NEAR_TOL

pytestmark = pytest.mark.gpu

BOXES = {"cube": None, "T": T, "O": O}
COMMITTED = (NEAR_TOL["field"], NEAR_TOL["field"])  # u, G
NAMES = ("u", "G")


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _box6(A):
    return () if A is None else (A[0, 0], A[1, 0], A[1, 1], A[2, 0], A[2, 1], A[2, 2])


def _parts(out):
    """(u, G as a matrix or None) of a device result [n, 3 or 12, *cols]"""
    out = out.cpu().numpy()
    return out[:, :3], out[:, 3:].reshape((out.shape[0], 3, 3) + out.shape[2:]) if out.shape[1] == 12 else None


def _sweep(box, x, f, batch, alpha, r_c, order):
    import torch_nfft_amd as tn
    out = tn.ops.nfft_ewald_stokeslet_near(_cuda(x), _cuda(f), _cuda(batch), _box6(BOXES[box]), alpha, r_c, order)
    tn.ops.check_status()
    assert out.shape == (x.shape[0], 12 if order == 2 else 3) + f.shape[2:] and out.dtype == torch.float32
    return out


def _near_gates(f, x, A, batch, alpha, r_c, order):
    """(float64 pair sums, [(gate, emulation term)] per quantity)"""
    ref = sr.near(f, x, A, batch, alpha, r_c, order)
    emu = sr.near_f32(f, x, A, batch, alpha, r_c, order)
    return ref, [sr.near_gate(w, e, r, c) for w, e, r, c in zip(NAMES[:order], emu, ref, COMMITTED)]


RAGGED = np.concatenate([np.zeros(230, np.int64), np.full(282, 2, np.int64)])  # three point sets, the middle one empty

# box, alpha, r_c (cube: G = 3, 4, 8), ragged, cols (CC = 1, 2, 4 and 4 with a tail), order
CASES = [
    ("cube", 5.0, 0.3, False, (), 2),
    ("cube", 5.0, 0.3, True, (2,), 1),
    ("cube", 5.0, 0.3, False, (5,), 2),
    ("cube", 6.0, 0.25, True, (), 1),
    ("cube", 6.0, 0.25, False, (3,), 2),
    ("cube", 6.0, 0.25, True, (5,), 1),
    ("cube", 12.0, 0.12, False, (2,), 2),
    ("cube", 12.0, 0.12, True, (3,), 2),
    ("cube", 12.0, 0.12, True, (), 1),
    ("T", 5.0, 0.3, True, (), 2),
    ("T", 5.0, 0.3, False, (2,), 1),
    ("T", 6.0, 0.25, False, (3,), 1),
    ("T", 6.0, 0.25, True, (5,), 2),
    ("T", 12.0, 0.12, True, (2,), 2),
    ("O", 6.0, 0.25, True, (), 1),
    ("O", 6.0, 0.25, False, (2,), 2),
    ("O", 12.0, 0.12, True, (3,), 2),
    ("O", 12.0, 0.12, False, (5,), 1),
]


@pytest.mark.parametrize("box,alpha,r_c,ragged,cols,order", CASES)
def test_near_sweep_against_brute_force(box, alpha, r_c, ragged, cols, order):
    x = sr.near_points()
    A = BOXES[box]
    assert x.shape == (512, 3) and dr.min_separation(x, A) >= 0.03 * (1.0 if A is None else 0.8)
    f = sr.near_forces(int(alpha) * 100 + len(cols) + 10 * ragged + order, 512, cols)
    batch = RAGGED if ragged else None
    got = _parts(_sweep(box, x, f, batch, alpha, r_c, order))
    ref, gates = _near_gates(f, x, A, batch, alpha, r_c, order)
    for what, g, r, (gate, emu), committed in zip(NAMES[:order], got, ref, gates, COMMITTED):
        err = rel_l2(g, r)
        print("stokeslet near %s (%g, %g) ragged=%d cols=%s order=%d: %s rel_l2 %.3e, gate %.3e = max(4 x %.3e, %.3e)"
              % (box, alpha, r_c, ragged, cols, order, what, err, gate, emu, committed))
        assert np.linalg.norm(r) > 0 and err <= gate


@pytest.fixture(scope="module")
def crowded():
    """14^3 points on a jittered lattice of spacing 0.017 (jitter 20 %: no two closer than 0.01) in a cube of edge 0.24 centred
    on the box corner (1/2, 1/2, 1/2), the crowded corner of the dipole sum's tests: ~343 points in each of the eight corner
    cells of the 3^3 grid -- several LDS tiles and work items per cell -- and most pairs through a wrap.  Five columns of
    forces, their float64 sums at (5, 0.3) and the float32 emulation's."""
    rng = np.random.default_rng(7)
    x = dr.jittered_lattice(rng, 14, 0.017, 0.2 * 0.017, centre=0.5).reshape(-1, 3)
    f = sr.near_forces(8, x.shape[0], (5,))
    return x, f, sr.near(f, x, None, None, 5.0, 0.3), sr.near_f32(f, x, None, None, 5.0, 0.3)


@pytest.mark.parametrize("columns", [1, 2, 5])
def test_crowded_corner(crowded, columns):
    x, f, ref, emu = crowded
    assert x.shape == (2744, 3) and (x > 0.5).any(0).all() and (x < 0.5).any(0).all() and dr.min_separation(x) >= 0.01
    f = f[:, :, :columns]
    out = _sweep("cube", x, f, None, 5.0, 0.3, 2)
    got, gates = _parts(out), []
    for what, g, r, e, committed in zip(NAMES, got, ref, emu, COMMITTED):
        r, e = r[..., :columns], e[..., :columns]
        gate, term = sr.near_gate(what, e, r, committed)
        gates.append(gate)
        err = rel_l2(g, r)
        print("stokeslet near, crowded corner, %d columns: %s rel_l2 %.3e, gate %.3e = max(4 x %.3e, %.3e)"
              % (columns, what, err, gate, term, committed))
        assert err <= gate
    # no atomics: the same bits again; the order-1 instantiation adds the same pairs
    again = _sweep("cube", x, f, None, 5.0, 0.3, 2)
    assert torch.equal(again, out)
    first = _parts(_sweep("cube", x, f, None, 5.0, 0.3, 1))[0]
    print("stokeslet near, crowded corner, %d columns: order 1 against order 2, u rel_l2 %.3e" % (columns, rel_l2(first, got[0])))
    assert rel_l2(first, got[0]) <= gates[0]


@pytest.mark.parametrize("N,box,order,C", [(N, box, order, C) for N in (8, 16) for box in ("cube", "T") for order in (1, 2)
                                           for C in (1, 3)])
def test_spectral_kernel(N, box, order, C):
    """against the einsum of the table in torch complex64 on the device: rel_l2 <= 1e-6, the dipole spectral test's figure (the
    projection adds two roundings and |P rho| ~ sqrt(2/3) |rho|); exact zeros where c_k = 0; equal bits on a second call"""
    import torch_nfft_amd as tn
    A = BOXES[box]
    alpha = 6.0
    sp = tn.EwaldSplitting(alpha, 0.25, N, box=None if A is None else torch.from_numpy(A))
    rng = np.random.default_rng(N + order + C)
    band = (rng.standard_normal((2, N, N, N, 3, C)) + 1j * rng.standard_normal((2, N, N, N, 3, C))).astype(np.complex64)
    got = tn.ops.nfft_ewald_stokeslet_spectral(_cuda(band), sp.stokeslet_coeffs, _box6(A), order)
    tn.ops.check_status()
    assert got.shape == (2, N, N, N, 12 if order == 2 else 3, C) and got.dtype == torch.complex64
    table = _cuda(sr.spectral_table(A, alpha, N, order).astype(np.complex64))
    want = torch.einsum("xyzsr,bxyzrc->bxyzsc", table, _cuda(band))
    err = float((got - want).norm() / want.norm())
    print("stokeslet spectral N=%d %s order=%d C=%d: rel_l2 %.3e" % (N, box, order, C, err))
    assert err <= 1e-6
    h = N // 2  # (c_0 = 0 and the unpaired planes)
    assert all(bool((part == 0).all()) for part in (got[:, 0], got[:, :, 0], got[:, :, :, 0], got[:, h, h, h]))
    assert torch.equal(tn.ops.nfft_ewald_stokeslet_spectral(_cuda(band), sp.stokeslet_coeffs, _box6(A), order), got)
    tn.ops.check_status()


# ---- the whole sum ----------------------------------------------------------------------------------------------------
# (alpha, r_c, N) = (8, 0.3, 32) in the cube and in T; O has the perpendicular width 0.8 and admits r_c <= 0.8 / 3 only, so it runs
# at (8, 0.25, 32)
WHOLE = {"cube": (8.0, 0.3, 32), "T": (8.0, 0.3, 32), "O": (8.0, 0.25, 32)}


def _splitting(box):
    import torch_nfft_amd as tn
    A = BOXES[box]
    alpha, r_c, N = WHOLE[box]
    return tn.EwaldSplitting(alpha, r_c, N, box=None if A is None else torch.from_numpy(A))


def _whole_sources():
    """7^3 points on a jittered lattice (spacing 1/7, jitter 0.03) in two point sets; two columns of forces f and of weights g"""
    rng = np.random.default_rng(3)
    s = rng.permutation(dr.jittered_lattice(rng, 7, 1.0 / 7, 0.03).reshape(-1, 3))
    n = s.shape[0]
    f, g = rng.standard_normal((n, 3, 2)).astype(np.float32), rng.standard_normal((n, 3, 2)).astype(np.float32)
    return s, f, g, (np.arange(n) >= 160).astype(np.int64)


_REFERENCE = {}


def _reference(box, cartesian=False):
    """The float64 parts of the algorithm for the forces and the weights side by side, columns [2 (f, g), 2]: (fractional
    float32 positions, Cartesian positions or None, near, far, terms), each (u, G).  Computed once per box and kind of input."""
    key = (box, cartesian)
    if key not in _REFERENCE:
        s, f, g, batch = _whole_sources()
        A = BOXES[box]
        xc = None
        if cartesian:  # x = s A in float32 has lost the last bits of s: the reference stands on the s that x stands for
            xc = (s.astype(np.float64) @ A).astype(np.float32)
            s = (xc.astype(np.float64) @ np.linalg.inv(A)).astype(np.float32)
        alpha, r_c, N = WHOLE[box]
        f4 = np.stack([f, g], 2)  # [n, 3, 2, 2]
        _REFERENCE[key] = (s, xc, sr.near(f4, s, A, batch, alpha, r_c), sr.far(f4, s, A, batch, alpha, N),
                           sr.terms(f4, s.shape[0], alpha))
    return _REFERENCE[key]


def _yardstick_far(box, f, s, batch):
    """the far part composed from the operators of the parent commit: nfft_adjoint of the forces, the table of
    stokeslet_ref.spectral_table as a torch product in complex64, nfft_forward: (u, G) as numpy"""
    import torch_nfft_amd as tn
    alpha, r_c, N = WHOLE[box]
    table = _cuda(sr.spectral_table(BOXES[box], alpha, N).astype(np.complex64))
    band = tn.nfft_adjoint(_cuda(f), _cuda(s), _cuda(batch), bandwidth=N, cutoff=4)
    spectra = torch.einsum("xyzsr,bxyzr...->bxyzs...", table, band).contiguous()
    out = tn.nfft_forward(spectra, _cuda(s), _cuda(batch), cutoff=4, real_output=True)
    tn.ops.check_status()
    return _parts(out)


def _whole_bounds(box, f, s, batch, near, far, label):
    """per quantity the absolute l2 bound 2 e_far + gate_near |near| of a device evaluation of these forces"""
    alpha, r_c, N = WHOLE[box]
    emu = sr.near_f32(f, s, BOXES[box], batch, alpha, r_c)
    yard = _yardstick_far(box, f, s, batch)
    bounds = []
    for what, e, r, y, ff, committed in zip(NAMES, emu, near, yard, far, COMMITTED):
        nr = float(np.linalg.norm(r))
        gate, term = sr.near_gate(what, e, r, committed) if nr > 0 else (committed, 0.0)
        e_far = float(np.linalg.norm(y - ff))
        bounds.append(2.0 * e_far + gate * nr)
        print("%s %s: e_far %.3e (rel %.3e), near gate %.3e = max(4 x %.3e, %.3e), |near| %.3e, bound %.3e"
              % (label, what, e_far, e_far / max(np.linalg.norm(ff), 1e-300), gate, term, committed, nr, bounds[-1]))
    return bounds


def _trace(M):
    return M[:, 0, 0] + M[:, 1, 1] + M[:, 2, 2]


@pytest.mark.parametrize("box,cartesian", [("cube", False), ("T", False), ("T", True), ("O", False)])
def test_whole_sum(box, cartesian):
    import torch_nfft_amd as tn
    _, f, _, batch = _whole_sources()
    s, xc, near, far, terms = _reference(box, cartesian)
    near, far, terms = ([p[:, ..., 0, :] for p in part] for part in (near, far, terms))  # the forces' columns
    A = BOXES[box]
    label = "nfft_ewald_stokeslet in %s%s" % (box, ", Cartesian input" if cartesian else "")
    bounds = _whole_bounds(box, f, s, batch, near, far, label)
    sp = _splitting(box)
    kw = dict(splitting=sp, cutoff=4, fractional=A is not None and not cartesian)
    pos = xc if cartesian else s
    got = tn.nfft_ewald_stokeslet(_cuda(f), _cuda(pos), _cuda(batch), gradient=True, **kw)
    first = tn.nfft_ewald_stokeslet(_cuda(f), _cuda(pos), _cuda(batch), **kw)
    tn.ops.check_status()
    assert len(got) == 2 and isinstance(first, torch.Tensor)
    assert got[0].shape == (343, 3, 2) and got[1].shape == (343, 3, 3, 2) and first.shape == (343, 3, 2)
    assert all(g.dtype == torch.float32 and not g.requires_grad for g in got)
    for what, g, n_, f_, t_, bound in zip(NAMES, got, near, far, terms, bounds):
        want = n_ + f_ + t_
        err = float(np.linalg.norm(g.cpu().numpy() - want))
        print("%s %s: |device - algorithm| %.3e (rel %.3e), bound %.3e" % (label, what, err, err / np.linalg.norm(want), bound))
        assert err <= bound
    uw = near[0] + far[0] + terms[0]
    assert float(np.linalg.norm(first.cpu().numpy() - uw)) <= bounds[0]
    # tr G = 0: the bound of G summed over the diagonal (Cauchy-Schwarz: sqrt(3)) beside what the truncated algorithm itself
    # misses, in float64
    own = float(np.linalg.norm(_trace(near[1] + far[1] + terms[1])))
    err = float(np.linalg.norm(_trace(got[1].cpu().numpy().astype(np.float64))))
    print("%s tr G: %.3e, bound %.3e + the algorithm's own %.3e" % (label, err, math.sqrt(3.0) * bounds[1], own))
    assert abs(err - own) <= math.sqrt(3.0) * bounds[1]  # (both sides of the triangle inequality)
    # the power: a sum of products, each u good to its bound (Cauchy-Schwarz per point set, all columns together)
    P = tn.nfft_ewald_stokeslet_power(_cuda(f), _cuda(pos), _cuda(batch), **kw).cpu().numpy()
    tn.ops.check_status()
    want = sr.power(f, uw, batch)
    assert P.shape == (2, 2)
    bound = 0.5 * np.linalg.norm(f, axis=1).max() * bounds[0] * math.sqrt(343.0)
    print("%s power: |error| %.3e, bound %.3e" % (label, np.abs(P - want).max(), bound))
    assert np.abs(P - want).max() <= bound


@pytest.mark.parametrize("box", ["cube", "T"])
def test_converged_sum(box):
    """One small set against the sum carried to convergence: |device - converged| <= |device - algorithm| + |algorithm -
    converged|, the first within the whole sum's bound, the second computed here in float64.  The set is the 4^3 cluster
    across the box corner of the dipole tests."""
    import torch_nfft_amd as tn
    A = BOXES[box]
    rng = np.random.default_rng(9)
    s = dr.jittered_lattice(rng, 4, 0.1, 0.02, centre=0.45).reshape(-1, 3)
    assert (s > 0.5).any(0).all() and dr.min_separation(s, A) >= 0.04
    f = sr.near_forces(10, 64, ())
    alpha, r_c, N = WHOLE[box]
    near, far = sr.near(f, s, A, None, alpha, r_c), sr.far(f, s, A, None, alpha, N)
    terms = sr.terms(f, 64, alpha)
    conv = sr.converged(f, s, A)
    bounds = _whole_bounds(box, f, s, None, near, far, "converged sum in %s" % box)
    got = tn.nfft_ewald_stokeslet(_cuda(f), _cuda(s), splitting=_splitting(box), cutoff=4, gradient=True, fractional=A is not None)
    tn.ops.check_status()
    for what, g, n_, f_, t_, c, bound in zip(NAMES, got, near, far, terms, conv, bounds):
        own = float(np.linalg.norm(n_ + f_ + t_ - c))
        err = float(np.linalg.norm(g.cpu().numpy() - c))
        print("nfft_ewald_stokeslet %s in %s: |device - converged| %.3e (rel %.3e), bound %.3e + the algorithm's own %.3e"
              % (what, box, err, err / np.linalg.norm(c), bound, own))
        assert abs(err - own) <= bound  # (both sides of the triangle inequality: own - bound <= err <= own + bound)


def test_hasimoto_constant():
    """One force in the unit cube at (8, 0.3, 32): u = -(4/3) 2.8372974795 f = -3.783063306 f, within the whole sum's bound (no
    pair: the far part's alone) plus the algorithm's own truncation in float64"""
    import torch_nfft_amd as tn
    s = np.array([[0.1, -0.2, 0.35]], np.float32)
    f = np.array([[0.3, -1.1, 0.7]], np.float32)
    alpha, r_c, N = WHOLE["cube"]
    near, far = sr.near(f, s, None, None, alpha, r_c, order=2), sr.far(f, s, None, None, alpha, N)
    assert np.linalg.norm(near[0]) == 0.0
    bound = _whole_bounds("cube", f, s, None, near, far, "one force in the unit cube")[0]
    want = -3.783063306 * f.astype(np.float64)
    own = float(np.linalg.norm(far[0] + sr.terms(f, 1, alpha)[0] - want))
    u = tn.nfft_ewald_stokeslet(_cuda(f), _cuda(s), splitting=_splitting("cube"), cutoff=4)
    tn.ops.check_status()
    err = float(np.linalg.norm(u.cpu().numpy() - want))
    print("one force in the unit cube: u / f = %s, |u + 3.783063306 f| %.3e, bound %.3e + the algorithm's own %.3e"
          % (u.cpu().numpy() / f, err, bound, own))
    assert err <= bound + own


@pytest.mark.parametrize("box,cartesian", [("cube", False), ("T", False), ("T", True)])
def test_autograd(box, cartesian):
    """(df, dpos) of (u g).sum() and dpos of the power against the formulas of section 7m evaluated with stokeslet_ref.  The
    backward is ONE order-2 evaluation of the forces f and the weights g side by side; with dX the error of its quantity X,
    within the whole sum's bound b_X for those four columns:
        |df - u[g]| <= b_u,
        |dpos - want| <= sqrt(4) max |f_i, g_i| b_G   (Cauchy-Schwarz over the four columns),
    times |A|_2 for fractional input."""
    import torch_nfft_amd as tn
    _, f, g, batch = _whole_sources()
    s, xc, near, far, terms = _reference(box, cartesian)
    A = BOXES[box]
    f4 = np.stack([f, g], 2)
    label = "autograd in %s%s" % (box, ", Cartesian input" if cartesian else "")
    b_u, b_G = _whole_bounds(box, f4, s, batch, near, far, label)
    u, G = (n_ + f_ + t_ for n_, f_, t_ in zip(near, far, terms))  # [n, 3, (3,) 2 (f, g), 2]
    fractional = A is not None and not cartesian
    kw = dict(splitting=_splitting(box), cutoff=4, fractional=fractional)
    fd = _cuda(f).requires_grad_(True)
    xd = _cuda(xc if cartesian else s).requires_grad_(True)
    v = tn.nfft_ewald_stokeslet(fd, xd, _cuda(batch), **kw)
    df, dx = torch.autograd.grad((v * _cuda(g)).sum(), (fd, xd))
    tn.ops.check_status()
    assert df.shape == f.shape and dx.shape == s.shape
    scale = np.linalg.norm(A, 2) if fractional else 1.0
    weight = max(np.linalg.norm(f, axis=1).max(), np.linalg.norm(g, axis=1).max())
    want = sr.position_gradient(f, g, G[:, :, :, 0], G[:, :, :, 1])
    if fractional:
        want = want @ A.T
    for what, got, ref, bound in (("df", df, u[:, :, 1], b_u), ("dpos", dx, want, 2.0 * weight * b_G * scale)):
        err = float(np.linalg.norm(got.cpu().numpy() - ref))
        print("%s %s: |error| %.3e (rel %.3e), bound %.3e" % (label, what, err, err / np.linalg.norm(ref), bound))
        assert err <= bound
    # only the forces' gradient asked for: one order-1 evaluation of the weights
    v = tn.nfft_ewald_stokeslet(fd, xd.detach(), _cuda(batch), **kw)
    df1, = torch.autograd.grad((v * _cuda(g)).sum(), (fd,))
    tn.ops.check_status()
    assert float(np.linalg.norm(df1.cpu().numpy() - u[:, :, 1])) <= b_u
    # the power: g = f / 2, dP/dpos_i,b = sum_a f_i,a G[f]_i,ab summed over the columns.  The backward evaluates f and f / 2 side by
    # side: with the bound b of the forces' two columns alone, the columns of f carry b and the weights 1/2, those of f / 2 carry
    # b / 2 (the bound is homogeneous) and the weights 1: sqrt(2) max |f_i| b_G
    _, s_G = _whole_bounds(box, f, s, batch, [p[:, ..., 0, :] for p in near], [p[:, ..., 0, :] for p in far],
                           label + ", the forces alone")
    xe = _cuda(xc if cartesian else s).requires_grad_(True)
    P = tn.nfft_ewald_stokeslet_power(_cuda(f), xe, _cuda(batch), **kw)
    de, = torch.autograd.grad(P.sum(), xe)
    tn.ops.check_status()
    want = (f.astype(np.float64)[:, :, None] * G[:, :, :, 0]).sum(1).sum(2)
    if fractional:
        want = want @ A.T
    bound = math.sqrt(2.0) * np.linalg.norm(f, axis=1).max() * s_G * scale
    err = float(np.linalg.norm(de.cpu().numpy() - want))
    print("%s power dpos: |error| %.3e (rel %.3e), bound %.3e" % (label, err, err / np.linalg.norm(want), bound))
    assert err <= bound


def test_second_derivative_refusals_and_empty_input():
    import torch_nfft_amd as tn
    s, f, _, batch = _whole_sources()
    sp = _splitting("cube")
    fd, xd, bd = _cuda(f).requires_grad_(True), _cuda(s).requires_grad_(True), _cuda(batch)
    u, G = tn.nfft_ewald_stokeslet(fd, xd, bd, splitting=sp, gradient=True)
    assert u.requires_grad and not G.requires_grad
    df, dx = torch.autograd.grad(u.square().sum(), (fd, xd), create_graph=True)
    with pytest.raises(RuntimeError, match="differentiate twice|once_differentiable"):
        dx.square().sum().backward()
    tn.ops.check_status()
    with pytest.raises(AssertionError, match="batch"):
        tn.nfft_ewald_stokeslet(fd, xd, torch.zeros(343, device="cuda", requires_grad=True), splitting=sp)
    with pytest.raises(TypeError, match="EwaldSplitting"):
        tn.nfft_ewald_stokeslet(fd, xd, bd, splitting=tn.DispersionSplitting(8.0, 0.3, 32))
    with pytest.raises(ValueError, match="complex"):
        tn.nfft_ewald_stokeslet(fd.detach().to(torch.complex64), xd, bd, splitting=sp)
    with pytest.raises(ValueError, match="fractional"):
        tn.nfft_ewald_stokeslet(fd, xd, bd, splitting=sp, fractional=True)
    fs = fd.detach()
    with pytest.raises(RuntimeError, match="Input mismatch"):
        tn.ops.nfft_ewald_stokeslet_near(xd.detach(), fs, bd, (), 5.0, 0.34, 2)
    with pytest.raises(RuntimeError, match="Input mismatch"):
        tn.ops.nfft_ewald_stokeslet_near(xd.detach(), fs, bd, (), 5.0, 0.3, 3)
    with pytest.raises(RuntimeError, match="Input mismatch"):
        tn.ops.nfft_ewald_stokeslet_near(xd.detach(), fs[:, :2].contiguous(), bd, (), 5.0, 0.3, 1)
    with pytest.raises(RuntimeError, match="Input mismatch"):
        tn.ops.nfft_ewald_stokeslet_near(xd.detach(), fs, bd, _box6(O), 5.0, 0.3, 1)
    tn.ops.check_status()
    # empty input
    f0 = torch.zeros(0, 3, 2, device="cuda", requires_grad=True)
    x0 = torch.zeros(0, 3, device="cuda", requires_grad=True)
    u, G = tn.nfft_ewald_stokeslet(f0, x0, splitting=sp, gradient=True)
    assert u.shape == (0, 3, 2) and G.shape == (0, 3, 3, 2)
    df0, dx0 = torch.autograd.grad(u.sum(), (f0, x0))
    assert df0.shape == (0, 3, 2) and dx0.shape == (0, 3)
    assert tn.nfft_ewald_stokeslet_power(f0, x0, splitting=sp).shape == (1, 2)
    out = tn.ops.nfft_ewald_stokeslet_near(x0.detach(), torch.zeros(0, 3, 2, device="cuda"), None, (), 5.0, 0.3, 2)
    assert out.shape == (0, 12, 2)
    tn.ops.check_status()
