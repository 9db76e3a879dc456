"""GPU tests of the Ewald sum for point charges and point dipoles: the wrapped pair sweep and the
spectral step of csrc/ewald_dipole.hip, and nfft_ewald_dipole / nfft_ewald_dipole_energy with their gradients, against the
float64 restatement tests/dipole_ref.py on the same float32 positions.

The gates hold no numbers of their own.
* A pair sweep is held, per quantity (phi, E, T), to rel_l2 <= max(4 x rel_l2(float32 emulation, float64), the committed
  figure of the Coulomb pair loop): the emulation (dipole_ref.near_f32) is the number format's own rounding on these points,
  the committed figure (tests/test_gpu_ewald.py: NEAR_TOL["value"] for phi, ["field"] for E and T) what the erfcf / __expf pair
  loop measured on this hardware, 4 x the project's margin.  tests/test_dipole_ref.py shows that a dropped B_3 or m delta_ab B_2
  term, a missing wrap or a cut at 0.95 r_c each move some output by more than ten times that.
* The spectral kernel against the same expression in torch complex64 on the device: rel_l2 <= 1e-6, a few float32 roundings
  (6e-8 each) of products of exactly representable inputs.
* The whole sum, per quantity: |device - algorithm| <= 2 e_far + gate_near |near|, where e_far is the absolute l2 error of the
  far part composed in the test from nfft_adjoint, torch multiplications and nfft_forward (the 2 covers the run-to-run scatter
  of the transforms' float atomics between that run and the function's own) and gate_near the pair sweep's gate.
* Against the converged sum and in the gradients the bounds are composed from these by the triangle and Cauchy-Schwarz
  inequalities.
Every case prints the terms of its gate beside the device's figure.
"""
import math

import numpy as np
import pytest
import torch

import dipole_ref as dp
import dispersion_ref as dr
import ewald_ref as er
from conftest import rel_l2
from ewald_box_ref import O, T
from test_gpu_ewald import NEAR_TOL, WHOLE_TOL

pytestmark = pytest.mark.gpu

BOXES = {"cube": None, "T": T, "O": O}
COMMITTED = (NEAR_TOL["value"], NEAR_TOL["field"], NEAR_TOL["field"])  # phi, E, T
NAMES = ("phi", "E", "T")


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _box6(A):
    return () if A is None else (A[0, 0], A[1, 0], A[1, 1], A[2, 0], A[2, 1], A[2, 2])


def _matrix(six):
    """[n, 6, *cols] in the order of dipole_ref.VOIGT as the symmetric [n, 3, 3, *cols]"""
    M = np.zeros((six.shape[0], 3, 3) + six.shape[2:], six.dtype)
    for e, (a, b) in enumerate(dp.VOIGT):
        M[:, a, b] = M[:, b, a] = six[:, e]
    return M


def _parts(out):
    """(phi, E, T as a matrix or None) of a device result [n, 4 or 10, *cols]"""
    out = out.cpu().numpy()
    return out[:, 0], out[:, 1:4], _matrix(out[:, 4:]) if out.shape[1] == 10 else None


def _sweep(box, x, q, mu, batch, alpha, r_c, order):
    import torch_nfft_amd as tn
    xs = np.concatenate([q[:, None], mu], 1)
    out = tn.ops.nfft_ewald_dipole_near(_cuda(x), _cuda(xs), _cuda(batch), _box6(BOXES[box]), alpha, r_c, order)
    tn.ops.check_status()
    assert out.shape == (x.shape[0], 10 if order == 2 else 4) + q.shape[1:] and out.dtype == torch.float32
    return out


def _near_gates(q, mu, x, A, batch, alpha, r_c, order):
    """(float64 pair sums, [(gate, emulation term)] per quantity)"""
    ref = dp.near(q, mu, x, A, batch, alpha, r_c, order)
    emu = dp.near_f32(q, mu, x, A, batch, alpha, r_c, order)
    return ref, [dp.near_gate(w, e, r, c) for w, e, r, c in zip(NAMES[:order + 1], emu, ref, COMMITTED)]


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
    x = dp.near_points()
    A = BOXES[box]
    assert x.shape == (512, 3) and dr.min_separation(x, A) >= 0.03 * (1.0 if A is None else 0.8)
    q, mu = dp.near_sources(int(alpha) * 100 + len(cols) + 10 * ragged + order, 512, cols)
    batch = RAGGED if ragged else None
    got = _parts(_sweep(box, x, q, mu, batch, alpha, r_c, order))
    ref, gates = _near_gates(q, mu, x, A, batch, alpha, r_c, order)
    for what, g, r, (gate, emu), committed in zip(NAMES[:order + 1], got, ref, gates, COMMITTED):
        err = rel_l2(g, r)
        print("dipole near %s (%g, %g) ragged=%d cols=%s order=%d: %s rel_l2 %.3e, gate %.3e = max(4 x %.3e, %.3e)"
              % (box, alpha, r_c, ragged, cols, order, what, err, gate, emu, committed))
        assert np.linalg.norm(r) > 0 and err <= gate


@pytest.fixture(scope="module")
def crowded():
    """14^3 points on a jittered lattice of spacing 0.017 (jitter 20 %: no two closer than 0.01) in a cube of edge 0.24 centred
    on the box corner (1/2, 1/2, 1/2), the crowded corner of the dispersion sum's tests: ~343 points in each of the eight
    corner cells of the 3^3 grid -- several LDS tiles and work items per cell -- and most pairs through a wrap.  Five columns
    of sources, their float64 sums at (5, 0.3) and the float32 emulation's."""
    rng = np.random.default_rng(7)
    x = dr.jittered_lattice(rng, 14, 0.017, 0.2 * 0.017, centre=0.5).reshape(-1, 3)
    q, mu = dp.near_sources(8, x.shape[0], (5,))
    return x, q, mu, dp.near(q, mu, x, None, None, 5.0, 0.3), dp.near_f32(q, mu, x, None, None, 5.0, 0.3)


@pytest.mark.parametrize("columns", [1, 2, 5])
def test_crowded_corner(crowded, columns):
    x, q, mu, ref, emu = crowded
    assert x.shape == (2744, 3) and (x > 0.5).any(0).all() and (x < 0.5).any(0).all() and dr.min_separation(x) >= 0.01
    q, mu = q[:, :columns], mu[:, :, :columns]
    out = _sweep("cube", x, q, mu, None, 5.0, 0.3, 2)
    got, gates = _parts(out), []
    for what, g, r, e, committed in zip(NAMES, got, ref, emu, COMMITTED):
        r, e = r[..., :columns], e[..., :columns]
        gate, term = dp.near_gate(what, e, r, committed)
        gates.append(gate)
        err = rel_l2(g, r)
        print("dipole near, crowded corner, %d columns: %s rel_l2 %.3e, gate %.3e = max(4 x %.3e, %.3e)"
              % (columns, what, err, gate, term, committed))
        assert err <= gate
    # no atomics: the same bits again; the order-1 instantiation adds the same pairs
    again = _sweep("cube", x, q, mu, None, 5.0, 0.3, 2)
    assert torch.equal(again, out)
    first = _parts(_sweep("cube", x, q, mu, None, 5.0, 0.3, 1))
    for what, a, b, gate in zip(NAMES[:2], first, got, gates):
        print("dipole near, crowded corner, %d columns: order 1 against order 2, %s rel_l2 %.3e" % (columns, what, rel_l2(a, b)))
        assert rel_l2(a, b) <= gate


@pytest.mark.parametrize("N,box,order,C", [(N, box, order, C) for N in (8, 16) for box in ("cube", "T") for order in (1, 2)
                                           for C in (1, 3)])
def test_spectral_kernel(N, box, order, C):
    """against the same expression in torch complex64 on the device: rel_l2 <= 1e-6 is a few float32 roundings (6e-8 each) of
    products of exactly representable inputs; equal bits on a second call"""
    import torch_nfft_amd as tn
    A = BOXES[box]
    alpha = 6.0
    sp = tn.EwaldSplitting(alpha, 0.25, N, box=None if A is None else torch.from_numpy(A))
    rng = np.random.default_rng(N + order + C)
    band = (rng.standard_normal((2, N, N, N, 4, C)) + 1j * rng.standard_normal((2, N, N, N, 4, C))).astype(np.complex64)
    got = tn.ops.nfft_ewald_dipole_spectral(_cuda(band), sp.coeffs, _box6(A), order)
    tn.ops.check_status()
    assert got.shape == (2, N, N, N, 10 if order == 2 else 4, C) and got.dtype == torch.complex64
    table = _cuda(dp.spectral_table(A, alpha, N, order).astype(np.complex64))
    want = torch.einsum("xyzsr,bxyzrc->bxyzsc", table, _cuda(band))
    err = float((got - want).norm() / want.norm())
    print("dipole spectral N=%d %s order=%d C=%d: rel_l2 %.3e" % (N, box, order, C, err))
    assert err <= 1e-6
    h = N // 2  # (b_0 = 0 and the unpaired planes)
    assert all(bool((part == 0).all()) for part in (got[:, 0], got[:, :, 0], got[:, :, :, 0], got[:, h, h, h]))
    assert torch.equal(tn.ops.nfft_ewald_dipole_spectral(_cuda(band), sp.coeffs, _box6(A), order), got)
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
    """7^3 points on a jittered lattice (spacing 1/7, jitter 0.03) in two point sets; two columns of sources (q, mu) and of
    weights (g1, g2) for phi and E"""
    rng = np.random.default_rng(3)
    s = rng.permutation(dr.jittered_lattice(rng, 7, 1.0 / 7, 0.03).reshape(-1, 3))
    n = s.shape[0]
    q, mu = rng.standard_normal((n, 2)).astype(np.float32), rng.standard_normal((n, 3, 2)).astype(np.float32)
    g1, g2 = rng.standard_normal((n, 2)).astype(np.float32), rng.standard_normal((n, 3, 2)).astype(np.float32)
    return s, q, mu, g1, g2, (np.arange(n) >= 160).astype(np.int64)


_REFERENCE = {}


def _reference(box, cartesian=False):
    """The float64 parts of the algorithm for the sources and the weights (g1, -g2) side by side, columns [2 (sources,
    weights), 2]: (fractional float32 positions, Cartesian positions or None, near, far, terms), each (phi, E, T).  Computed
    once per box and kind of input."""
    key = (box, cartesian)
    if key not in _REFERENCE:
        s, q, mu, g1, g2, batch = _whole_sources()
        A = BOXES[box]
        xc = None
        if cartesian:  # x = s A in float32 has lost the last bits of s: the reference stands on the s that x stands for
            xc = (s.astype(np.float64) @ A).astype(np.float32)
            s = (xc.astype(np.float64) @ np.linalg.inv(A)).astype(np.float32)
        alpha, r_c, N = WHOLE[box]
        q4, mu4 = np.stack([q, g1], 1), np.stack([mu, -g2], 2)
        _REFERENCE[key] = (s, xc, dp.near(q4, mu4, s, A, batch, alpha, r_c), dp.far(q4, mu4, s, A, batch, alpha, N),
                           dp.terms(q4, mu4, s.shape[0], A, batch, alpha))
    return _REFERENCE[key]


def _yardstick_far(box, xs, s, batch):
    """the far part composed from the operators of the parent commit: nfft_adjoint of the packed sources, the table of
    dipole_ref.spectral_table as a torch product in complex64, nfft_forward: (phi, E, T) as numpy"""
    import torch_nfft_amd as tn
    alpha, r_c, N = WHOLE[box]
    table = _cuda(dp.spectral_table(BOXES[box], alpha, N).astype(np.complex64))
    band = tn.nfft_adjoint(_cuda(xs), _cuda(s), _cuda(batch), bandwidth=N, cutoff=4)
    spectra = torch.einsum("xyzsr,bxyzr...->bxyzs...", table, band).contiguous()
    out = tn.nfft_forward(spectra, _cuda(s), _cuda(batch), cutoff=4, real_output=True)
    tn.ops.check_status()
    return _parts(out)


def _whole_bounds(box, q, mu, s, batch, near, far, label):
    """per quantity the absolute l2 bound 2 e_far + gate_near |near| of a device evaluation of these sources"""
    alpha, r_c, N = WHOLE[box]
    emu = dp.near_f32(q, mu, s, BOXES[box], batch, alpha, r_c)
    yard = _yardstick_far(box, np.concatenate([q[:, None], mu], 1), s, batch)
    bounds = []
    for what, e, r, y, f, committed in zip(NAMES, emu, near, yard, far, COMMITTED):
        gate, term = dp.near_gate(what, e, r, committed)
        e_far = float(np.linalg.norm(y - f))
        bounds.append(2.0 * e_far + gate * float(np.linalg.norm(r)))
        print("%s %s: e_far %.3e (rel %.3e), near gate %.3e = max(4 x %.3e, %.3e), |near| %.3e, bound %.3e"
              % (label, what, e_far, e_far / np.linalg.norm(f), gate, term, committed, np.linalg.norm(r), bounds[-1]))
    return bounds


@pytest.mark.parametrize("box,cartesian", [("cube", False), ("T", False), ("T", True), ("O", False)])
def test_whole_sum(box, cartesian):
    import torch_nfft_amd as tn
    _, q, mu, _, _, batch = _whole_sources()
    s, xc, near, far, terms = _reference(box, cartesian)
    near, far, terms = ([p[:, ..., 0, :] for p in part] for part in (near, far, terms))  # the sources' columns
    A = BOXES[box]
    label = "nfft_ewald_dipole in %s%s" % (box, ", Cartesian input" if cartesian else "")
    bounds = _whole_bounds(box, q, mu, s, batch, near, far, label)
    sp = _splitting(box)
    kw = dict(splitting=sp, cutoff=4, fractional=A is not None and not cartesian)
    pos = xc if cartesian else s
    got = tn.nfft_ewald_dipole(_cuda(q), _cuda(mu), _cuda(pos), _cuda(batch), gradient=True, **kw)
    first = tn.nfft_ewald_dipole(_cuda(q), _cuda(mu), _cuda(pos), _cuda(batch), **kw)
    tn.ops.check_status()
    assert len(got) == 3 and len(first) == 2
    assert got[0].shape == (343, 2) and got[1].shape == (343, 3, 2) and got[2].shape == (343, 3, 3, 2)
    assert all(g.dtype == torch.float32 and not g.requires_grad for g in got)
    assert torch.equal(got[2], got[2].transpose(1, 2))
    for what, g, n_, f_, t_, bound in zip(NAMES, got, near, far, terms, bounds):
        want = n_ + f_ + t_
        err = float(np.linalg.norm(g.cpu().numpy() - want))
        print("%s %s: |device - algorithm| %.3e (rel %.3e), bound %.3e" % (label, what, err, err / np.linalg.norm(want), bound))
        assert err <= bound
    for what, g, n_, f_, t_, bound in zip(NAMES[:2], first, near, far, terms, bounds):
        assert float(np.linalg.norm(g.cpu().numpy() - (n_ + f_ + t_))) <= bound
    # tr T = -4 pi Q / V: the bound of T summed over the diagonal (Cauchy-Schwarz: sqrt(3)) beside what the truncated algorithm
    # itself misses, in float64
    V = 1.0 if A is None else float(np.linalg.det(A))
    Q = np.stack([q[batch == b].astype(np.float64).sum(0) for b in (0, 1)])[batch]
    Tw = near[2] + far[2] + terms[2]
    tr = lambda M: M[:, 0, 0] + M[:, 1, 1] + M[:, 2, 2]  # noqa: E731
    own = float(np.linalg.norm(tr(Tw) + 4.0 * math.pi * Q / V))
    err = float(np.linalg.norm(tr(got[2].cpu().numpy().astype(np.float64)) + 4.0 * math.pi * Q / V))
    print("%s tr T + 4 pi Q / V: %.3e, bound %.3e + the algorithm's own %.3e" % (label, err, math.sqrt(3.0) * bounds[2], own))
    assert abs(err - own) <= math.sqrt(3.0) * bounds[2]  # (both sides of the triangle inequality)
    # the energy: a sum of products, each factor good to its bound (Cauchy-Schwarz per point set, all columns together)
    U = tn.nfft_ewald_dipole_energy(_cuda(q), _cuda(mu), _cuda(pos), _cuda(batch), **kw).cpu().numpy()
    tn.ops.check_status()
    want = dp.energy(q, mu, near[0] + far[0] + terms[0], near[1] + far[1] + terms[1], batch)
    assert U.shape == (2, 2)
    bound = 0.5 * (np.abs(q).max() * bounds[0] + np.linalg.norm(mu, axis=1).max() * bounds[1]) * math.sqrt(343.0)
    print("%s energy: |error| %.3e, bound %.3e" % (label, np.abs(U - want).max(), bound))
    assert np.abs(U - want).max() <= bound


def test_pure_charges_agree_with_nfft_ewald():
    """mu = None: phi and E are within WHOLE_TOL of the float64 algorithm of nfft_ewald (tests/ewald_ref.py)"""
    import torch_nfft_amd as tn
    s, q, _, _, _, batch = _whole_sources()
    alpha, r_c, N = WHOLE["cube"]
    phi, E = tn.nfft_ewald_dipole(_cuda(q), None, _cuda(s), _cuda(batch), splitting=_splitting("cube"), cutoff=4)
    tn.ops.check_status()
    want = er.exact_algorithm(q, s, batch, alpha, r_c, N, field=True)
    ev, ef = rel_l2(phi.cpu().numpy(), want[0]), rel_l2(E.cpu().numpy(), want[1])
    print("nfft_ewald_dipole, pure charges: phi rel_l2 %.3e (gate %.3e), E rel_l2 %.3e (gate %.3e)"
          % (ev, WHOLE_TOL["value"], ef, WHOLE_TOL["field"]))
    assert ev <= WHOLE_TOL["value"] and ef <= WHOLE_TOL["field"]


def test_pure_dipoles():
    """q = None: the whole sum's bound for the dipoles alone"""
    import torch_nfft_amd as tn
    s, _, mu, _, _, batch = _whole_sources()
    alpha, r_c, N = WHOLE["cube"]
    near, far = dp.near(None, mu, s, None, batch, alpha, r_c), dp.far(None, mu, s, None, batch, alpha, N)
    terms = dp.terms(None, mu, 343, None, batch, alpha)
    bounds = _whole_bounds("cube", np.zeros((343, 2), np.float32), mu, s, batch, near, far, "nfft_ewald_dipole, pure dipoles")
    got = tn.nfft_ewald_dipole(None, _cuda(mu), _cuda(s), _cuda(batch), splitting=_splitting("cube"), cutoff=4, gradient=True)
    tn.ops.check_status()
    for what, g, n_, f_, t_, bound in zip(NAMES, got, near, far, terms, bounds):
        err = float(np.linalg.norm(g.cpu().numpy() - (n_ + f_ + t_)))
        print("nfft_ewald_dipole, pure dipoles, %s: |device - algorithm| %.3e, bound %.3e" % (what, err, bound))
        assert err <= bound


@pytest.mark.parametrize("box", ["cube", "T"])
def test_converged_sum(box):
    """One small set against the sum carried to convergence: |device - converged| <= |device - algorithm| + |algorithm -
    converged|, the first within the whole sum's bound, the second computed here in float64.  The set is a 4^3 cluster across
    the box corner."""
    import torch_nfft_amd as tn
    A = BOXES[box]
    rng = np.random.default_rng(9)
    s = dr.jittered_lattice(rng, 4, 0.1, 0.02, centre=0.45).reshape(-1, 3)
    assert (s > 0.5).any(0).all() and dr.min_separation(s, A) >= 0.04
    q, mu = dp.near_sources(10, 64, ())
    alpha, r_c, N = WHOLE[box]
    near, far = dp.near(q, mu, s, A, None, alpha, r_c), dp.far(q, mu, s, A, None, alpha, N)
    terms = dp.terms(q, mu, 64, A, None, alpha)
    conv = dp.converged(q, mu, s, A)
    bounds = _whole_bounds(box, q, mu, s, None, near, far, "converged sum in %s" % box)
    got = tn.nfft_ewald_dipole(_cuda(q), _cuda(mu), _cuda(s), splitting=_splitting(box), cutoff=4, gradient=True,
                               fractional=A is not None)
    tn.ops.check_status()
    for what, g, n_, f_, t_, c, bound in zip(NAMES, got, near, far, terms, conv, bounds):
        own = float(np.linalg.norm(n_ + f_ + t_ - c))
        err = float(np.linalg.norm(g.cpu().numpy() - c))
        print("nfft_ewald_dipole %s in %s: |device - converged| %.3e (rel %.3e), bound %.3e + the algorithm's own %.3e"
              % (what, box, err, err / np.linalg.norm(c), bound, own))
        assert abs(err - own) <= bound  # (both sides of the triangle inequality: own - bound <= err <= own + bound)


@pytest.mark.parametrize("box,cartesian", [("cube", False), ("T", False), ("T", True)])
def test_autograd(box, cartesian):
    """(dq, dmu, dpos) of (phi g1).sum() + (E g2).sum() and of the energy against the formulas of section 7l evaluated with
    dipole_ref.  The backward is ONE order-2 evaluation of the sources s and the weights s~ = (g1, -g2) side by side; with
    dX the error of its quantity X, within the whole sum's bound b_X for those four columns:
        |dq - phi[s~]| <= b_phi,  |dmu + E[s~]| <= b_E,
        |dpos - want| <= sqrt(4) (max |q, q~| b_E + max |mu, mu~| b_T)   (Cauchy-Schwarz over the four columns),
    times |A|_2 for fractional input."""
    import torch_nfft_amd as tn
    _, q, mu, g1, g2, batch = _whole_sources()
    s, xc, near, far, terms = _reference(box, cartesian)
    A = BOXES[box]
    q4, mu4 = np.stack([q, g1], 1), np.stack([mu, -g2], 2)
    label = "autograd in %s%s" % (box, ", Cartesian input" if cartesian else "")
    b_phi, b_E, b_T = _whole_bounds(box, q4, mu4, s, batch, near, far, label)
    phi, E, Tm = (n_ + f_ + t_ for n_, f_, t_ in zip(near, far, terms))  # [n, (3, (3,)) 2 (sources, weights), 2]
    fractional = A is not None and not cartesian
    kw = dict(splitting=_splitting(box), cutoff=4, fractional=fractional)
    qd, md = _cuda(q).requires_grad_(True), _cuda(mu).requires_grad_(True)
    xd = _cuda(xc if cartesian else s).requires_grad_(True)
    p, e = tn.nfft_ewald_dipole(qd, md, xd, _cuda(batch), **kw)
    dq, dmu, dx = torch.autograd.grad((p * _cuda(g1)).sum() + (e * _cuda(g2)).sum(), (qd, md, xd))
    tn.ops.check_status()
    assert dq.shape == q.shape and dmu.shape == mu.shape and dx.shape == s.shape
    scale = np.linalg.norm(A, 2) if fractional else 1.0
    weight_q = max(np.abs(q).max(), np.abs(g1).max())
    weight_mu = max(np.linalg.norm(mu, axis=1).max(), np.linalg.norm(g2, axis=1).max())
    want = -(g1[:, None] * E[:, :, 0] + (Tm[:, :, :, 0] * -g2[:, None]).sum(2) + q[:, None] * E[:, :, 1]
             + (Tm[:, :, :, 1] * mu[:, None]).sum(2)).sum(2)
    if fractional:
        want = want @ A.T
    bound_x = 2.0 * (weight_q * b_E + weight_mu * b_T) * scale
    for what, got, ref, bound in (("dq", dq, phi[:, 1], b_phi), ("dmu", dmu, -E[:, :, 1], b_E), ("dpos", dx, want, bound_x)):
        err = float(np.linalg.norm(got.cpu().numpy() - ref))
        print("%s %s: |error| %.3e (rel %.3e), bound %.3e" % (label, what, err, err / np.linalg.norm(ref), bound))
        assert err <= bound
    # only the sources' gradients asked for: one order-1 evaluation of the weights
    p, e = tn.nfft_ewald_dipole(qd, md, xd.detach(), _cuda(batch), **kw)
    dq1, dmu1 = torch.autograd.grad((p * _cuda(g1)).sum() + (e * _cuda(g2)).sum(), (qd, md))
    assert float(np.linalg.norm(dq1.cpu().numpy() - phi[:, 1])) <= b_phi
    assert float(np.linalg.norm(dmu1.cpu().numpy() + E[:, :, 1])) <= b_E
    # the energy: s~ = s / 2, dU/dpos_i = -(q_i E_i + T_i mu_i) summed over the columns.  The backward evaluates s and s / 2
    # side by side: with the bounds b of the sources' two columns alone, the columns of s carry b and the weights 1/2, those
    # of s / 2 carry b / 2 (the bound is homogeneous) and the weights 1: sqrt(2) (max |q| b_E + max |mu| b_T)
    _, s_E, s_T = _whole_bounds(box, q, mu, s, batch, [p[:, ..., 0, :] for p in near], [p[:, ..., 0, :] for p in far],
                                label + ", the sources alone")
    xe = _cuda(xc if cartesian else s).requires_grad_(True)
    U = tn.nfft_ewald_dipole_energy(_cuda(q), _cuda(mu), xe, _cuda(batch), **kw)
    de, = torch.autograd.grad(U.sum(), xe)
    tn.ops.check_status()
    want = -dp.force(q, mu, E[:, :, 0], Tm[:, :, :, 0]).sum(2)
    if fractional:
        want = want @ A.T
    bound = math.sqrt(2.0) * (np.abs(q).max() * s_E + np.linalg.norm(mu, axis=1).max() * s_T) * scale
    err = float(np.linalg.norm(de.cpu().numpy() - want))
    print("%s energy dpos: |error| %.3e (rel %.3e), bound %.3e" % (label, err, err / np.linalg.norm(want), bound))
    assert err <= bound


def test_second_derivative_refusals_and_empty_input():
    import torch_nfft_amd as tn
    s, q, mu, _, _, batch = _whole_sources()
    sp = _splitting("cube")
    qd, md, xd, bd = _cuda(q).requires_grad_(True), _cuda(mu).requires_grad_(True), _cuda(s).requires_grad_(True), _cuda(batch)
    phi, E, Tm = tn.nfft_ewald_dipole(qd, md, xd, bd, splitting=sp, gradient=True)
    assert phi.requires_grad and E.requires_grad and not Tm.requires_grad
    dq, dx = torch.autograd.grad(phi.square().sum() + E.square().sum(), (qd, xd), create_graph=True)
    with pytest.raises(RuntimeError, match="differentiate twice|once_differentiable"):
        dx.square().sum().backward()
    tn.ops.check_status()
    with pytest.raises(AssertionError, match="batch"):
        tn.nfft_ewald_dipole(qd, md, xd, torch.zeros(343, device="cuda", requires_grad=True), splitting=sp)
    with pytest.raises(TypeError, match="EwaldSplitting"):
        tn.nfft_ewald_dipole(qd, md, xd, bd, splitting=tn.DispersionSplitting(8.0, 0.3, 32))
    with pytest.raises(ValueError, match="complex"):
        tn.nfft_ewald_dipole(qd.detach().to(torch.complex64), md, xd, bd, splitting=sp)
    with pytest.raises(ValueError, match="fractional"):
        tn.nfft_ewald_dipole(qd, md, xd, bd, splitting=sp, fractional=True)
    xs = torch.cat([qd.detach().unsqueeze(1), md.detach()], 1)
    with pytest.raises(RuntimeError, match="Input mismatch"):
        tn.ops.nfft_ewald_dipole_near(xd.detach(), xs, bd, (), 5.0, 0.34, 2)
    with pytest.raises(RuntimeError, match="Input mismatch"):
        tn.ops.nfft_ewald_dipole_near(xd.detach(), xs, bd, (), 5.0, 0.3, 3)
    with pytest.raises(RuntimeError, match="Input mismatch"):
        tn.ops.nfft_ewald_dipole_near(xd.detach(), xs[:, :3].contiguous(), bd, (), 5.0, 0.3, 1)
    with pytest.raises(RuntimeError, match="Input mismatch"):
        tn.ops.nfft_ewald_dipole_near(xd.detach(), xs, bd, _box6(O), 5.0, 0.3, 1)
    tn.ops.check_status()
    # empty input
    q0 = torch.zeros(0, 2, device="cuda", requires_grad=True)
    m0 = torch.zeros(0, 3, 2, device="cuda", requires_grad=True)
    x0 = torch.zeros(0, 3, device="cuda", requires_grad=True)
    phi, E, Tm = tn.nfft_ewald_dipole(q0, m0, x0, splitting=sp, gradient=True)
    assert phi.shape == (0, 2) and E.shape == (0, 3, 2) and Tm.shape == (0, 3, 3, 2)
    dq, dm, dx0 = torch.autograd.grad(phi.sum() + E.sum(), (q0, m0, x0))
    assert dq.shape == (0, 2) and dm.shape == (0, 3, 2) and dx0.shape == (0, 3)
    assert tn.nfft_ewald_dipole_energy(q0, m0, x0, splitting=sp).shape == (1, 2)
    out = tn.ops.nfft_ewald_dipole_near(x0.detach(), torch.zeros(0, 4, 2, device="cuda"), None, (), 5.0, 0.3, 2)
    assert out.shape == (0, 10, 2)
    tn.ops.check_status()
