"""GPU tests of the periodic Rotne-Prager-Yamakawa sum: the wrapped pair sweep of csrc/ewald_rpy.hip
with its overlap branch, and nfft_ewald_rpy / nfft_ewald_rpy_power with their gradients, against the float64 restatement
tests/rpy_ref.py on the same float32 positions.  Modelled on tests/test_gpu_stokeslet.py, case for case.

The gates hold no numbers of their own and are the constructions of that file.
* A pair sweep is held, per quantity (u, G), to rel_l2 <= max(4 x rel_l2(float32 emulation, float64), the committed figure of
  the Coulomb field loop): the emulation (rpy_ref.near_f32) is the number format's own rounding of the formula that the kernel
  uses on these points, the committed figure (tests/test_gpu_ewald.py: NEAR_TOL["field"]) what the erfcf / __expf pair loop
  measured on this hardware.  tests/test_rpy_ref.py shows that a dropped a^2 term, a dropped overlap branch, a wrong self
  term or a missing wrap each move some output by more than ten times that.
* The whole sum, per quantity: |device - algorithm| <= 2 e_far + gate_near |near|, where e_far is the absolute l2 error of the
  far part composed in the test from nfft_adjoint, a torch product with rpy_ref.spectral_table and nfft_forward.
* Against the converged sum, the periodic self mobility of one sphere, in the gradients and for the mobility matrix the bounds
  are composed from these by the triangle and Cauchy-Schwarz inequalities.
Every case prints the terms of its gate beside the device's figure.
"""
import math

import numpy as np
import pytest
import torch

import dispersion_ref as dr
import rpy_ref as rr
from conftest import rel_l2
from ewald_box_ref import O, T
from test_gpu_ewald import NEAR_TOL

pytestmark = pytest.mark.gpu

BOXES = {"cube": None, "T": T, "O": O}
COMMITTED = (NEAR_TOL["field"], NEAR_TOL["field"])  # u, G
NAMES = ("u", "G")
HASIMOTO = 2.8372974795


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _box6(A):
    return () if A is None else (A[0, 0], A[1, 0], A[1, 1], A[2, 0], A[2, 1], A[2, 2])


def _parts(out):
    """(u, G as a matrix or None) of a device result [n, 3 or 12, *cols]"""
    out = out.cpu().numpy()
    return out[:, :3], out[:, 3:].reshape((out.shape[0], 3, 3) + out.shape[2:]) if out.shape[1] == 12 else None


def _sweep(box, x, f, batch, alpha, r_c, a, order):
    import torch_nfft_amd as tn
    out = tn.ops.nfft_ewald_rpy_near(_cuda(x), _cuda(f), _cuda(batch), _box6(BOXES[box]), alpha, r_c, a, order)
    tn.ops.check_status()
    assert out.shape == (x.shape[0], 12 if order == 2 else 3) + f.shape[2:] and out.dtype == torch.float32
    return out


def _overlapping(x, A, a):
    """per point: does it have a partner closer than 2 a; and the pairs' count and smallest r / a"""
    x = np.asarray(x, dtype=np.float64)
    has, count, closest = np.zeros(x.shape[0], bool), 0, np.inf
    for r0 in range(0, x.shape[0], 512):
        ds = x[r0:r0 + 512, None, :] - x[None, :, :]
        d = (ds - np.rint(ds)) @ rr._box(A)
        r = np.sqrt((d * d).sum(-1))
        ov = (r > 0) & (r < 2 * a)
        has[r0:r0 + 512] = ov.any(1)
        count += int(ov.sum())
        closest = min(closest, r[ov].min() / a) if ov.any() else closest
    return has, count // 2, closest


RAGGED = np.concatenate([np.zeros(230, np.int64), np.full(282, 2, np.int64)])  # three point sets, the middle one empty

# box, alpha, r_c (cube: G = 3, 4, 8), ragged, cols (CC = 1, 2, 4 and 4 with a tail), order: the grid of the Stokeslet sweep
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
    """the non-overlap weights, the tilings and the wraps on the 512 points of the Stokeslet sweep with a = 0.03 (a handful of
    its pairs overlap)"""
    x = rr.near_points()
    A = BOXES[box]
    a = 0.03
    assert x.shape == (512, 3) and 1 <= _overlapping(x, A, a)[1] <= 20
    f = rr.near_forces(int(alpha) * 100 + len(cols) + 10 * ragged + order, 512, cols)
    batch = RAGGED if ragged else None
    got = _parts(_sweep(box, x, f, batch, alpha, r_c, a, order))
    ref = rr.near(f, x, A, batch, alpha, r_c, a, order)
    emu = rr.near_f32(f, x, A, batch, alpha, r_c, a, order)
    for what, g, r, e, committed in zip(NAMES[:order], got, ref, emu, COMMITTED):
        gate, term = rr.near_gate(what, e, r, committed)
        err = rel_l2(g, r)
        print("rpy near %s (%g, %g) ragged=%d cols=%s order=%d: %s rel_l2 %.3e, gate %.3e = max(4 x %.3e, %.3e)"
              % (box, alpha, r_c, ragged, cols, order, what, err, gate, term, committed))
        assert np.linalg.norm(r) > 0 and err <= gate


@pytest.mark.parametrize("box", ["cube", "T"])
def test_overlap_branch_on_dimers(box):
    """256 dimers with separations from a / 2 to 2.5 a, a = 0.02: the overlap branch carries most of every sum.  The gate per
    quantity, and again over the points with an overlapping partner alone."""
    A = BOXES[box]
    a, alpha, r_c = 0.02, 6.0, 0.25
    x, sep = rr.dimers(A, a)
    assert x.shape == (512, 3) and int((sep < 2 * a).sum()) >= 150 and int((sep > 2 * a).sum()) >= 30
    assert sep.min() >= 0.49 * a and sep.max() <= 2.51 * a
    has, count, closest = _overlapping(x, A, a)
    assert count == int((sep < 2 * a).sum()) and int(has.sum()) == 2 * count  # (no overlaps but the dimers' own)
    f = rr.near_forces(21, 512, (2,))
    got = _parts(_sweep(box, x, f, None, alpha, r_c, a, 2))
    ref = rr.near(f, x, A, None, alpha, r_c, a)
    emu = rr.near_f32(f, x, A, None, alpha, r_c, a)
    for what, g, r, e, committed in zip(NAMES, got, ref, emu, COMMITTED):
        for label, rows in (("all points", slice(None)), ("overlapping points", has)):
            gate, term = rr.near_gate(what, e[rows], r[rows], committed)
            err = rel_l2(g[rows], r[rows])
            print("rpy dimers in %s (%d below 2 a, smallest r / a %.3f), %s: %s rel_l2 %.3e, gate %.3e = max(4 x %.3e, %.3e)"
                  % (box, count, closest, label, what, err, gate, term, committed))
            assert err <= gate


@pytest.fixture(scope="module")
def crowded():
    """the crowded corner of the Stokeslet tests (14^3 points on a jittered lattice of spacing 0.017 across the box corner, no
    two closer than 0.01) with a = 0.01: thousands of overlapping pairs.  Five columns of forces, their float64 sums at
    (5, 0.3) and the float32 emulation's."""
    rng = np.random.default_rng(7)
    x = dr.jittered_lattice(rng, 14, 0.017, 0.2 * 0.017, centre=0.5).reshape(-1, 3)
    f = rr.near_forces(8, x.shape[0], (5,))
    return x, f, rr.near(f, x, None, None, 5.0, 0.3, 0.01), rr.near_f32(f, x, None, None, 5.0, 0.3, 0.01)


@pytest.mark.parametrize("columns", [1, 2, 5])
def test_crowded_corner(crowded, columns):
    x, f, ref, emu = crowded
    a = 0.01
    _, count, closest = _overlapping(x, None, a)
    assert x.shape == (2744, 3) and count >= 5000 and 1.0 <= closest <= 1.2
    f = f[:, :, :columns]
    out = _sweep("cube", x, f, None, 5.0, 0.3, a, 2)
    got, gates = _parts(out), []
    for what, g, r, e, committed in zip(NAMES, got, ref, emu, COMMITTED):
        r, e = r[..., :columns], e[..., :columns]
        gate, term = rr.near_gate(what, e, r, committed)
        gates.append(gate)
        err = rel_l2(g, r)
        print("rpy near, crowded corner (%d overlapping pairs, smallest r / a %.2f), %d columns: %s rel_l2 %.3e, gate %.3e = "
              "max(4 x %.3e, %.3e)" % (count, closest, columns, what, err, gate, term, committed))
        assert err <= gate
    # no atomics: the same bits again; the order-1 instantiation adds the same pairs
    again = _sweep("cube", x, f, None, 5.0, 0.3, a, 2)
    assert torch.equal(again, out)
    first = _parts(_sweep("cube", x, f, None, 5.0, 0.3, a, 1))[0]
    print("rpy near, crowded corner, %d columns: order 1 against order 2, u rel_l2 %.3e" % (columns, rel_l2(first, got[0])))
    assert rel_l2(first, got[0]) <= gates[0]


# ---- the whole sum ----------------------------------------------------------------------------------------------------
WHOLE = {"cube": (8.0, 0.3, 32), "T": (8.0, 0.3, 32)}  # (alpha, r_c, N), those of the Stokeslet tests
RADIUS = 0.05  # 2 a = 0.1: the closest of the 7^3 lattice's pairs (>= 0.083 apart) overlap


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


def _reference(box):
    """The float64 parts of the algorithm for the forces and the weights side by side, columns [2 (f, g), 2]: (near, far,
    terms), each (u, G).  Computed once per box."""
    if box not in _REFERENCE:
        s, f, g, batch = _whole_sources()
        A = BOXES[box]
        alpha, r_c, N = WHOLE[box]
        f4 = np.stack([f, g], 2)  # [n, 3, 2, 2]
        _REFERENCE[box] = (rr.near(f4, s, A, batch, alpha, r_c, RADIUS), rr.far(f4, s, A, batch, alpha, RADIUS, N),
                           rr.terms(f4, s.shape[0], alpha, RADIUS))
    return _REFERENCE[box]


def _yardstick_far(box, f, s, batch, a):
    """the far part composed from operators that the sum does not add: nfft_adjoint of the forces, the table of
    rpy_ref.spectral_table as a torch product in complex64, nfft_forward: (u, G) as numpy"""
    import torch_nfft_amd as tn
    alpha, r_c, N = WHOLE[box]
    table = _cuda(rr.spectral_table(BOXES[box], alpha, N, a).astype(np.complex64))
    band = tn.nfft_adjoint(_cuda(f), _cuda(s), _cuda(batch), bandwidth=N, cutoff=4)
    spectra = torch.einsum("xyzsr,bxyzr...->bxyzs...", table, band).contiguous()
    out = tn.nfft_forward(spectra, _cuda(s), _cuda(batch), cutoff=4, real_output=True)
    tn.ops.check_status()
    return _parts(out)


def _whole_bounds(box, f, s, batch, near, far, label, a=RADIUS):
    """per quantity the absolute l2 bound 2 e_far + gate_near |near| of a device evaluation of these forces"""
    alpha, r_c, N = WHOLE[box]
    emu = rr.near_f32(f, s, BOXES[box], batch, alpha, r_c, a)
    yard = _yardstick_far(box, f, s, batch, a)
    bounds = []
    for what, e, r, y, ff, committed in zip(NAMES, emu, near, yard, far, COMMITTED):
        nr = float(np.linalg.norm(r))
        gate, term = rr.near_gate(what, e, r, committed) if nr > 0 else (committed, 0.0)
        e_far = float(np.linalg.norm(y - ff))
        bounds.append(2.0 * e_far + gate * nr)
        print("%s %s: e_far %.3e (rel %.3e), near gate %.3e = max(4 x %.3e, %.3e), |near| %.3e, bound %.3e"
              % (label, what, e_far, e_far / max(np.linalg.norm(ff), 1e-300), gate, term, committed, nr, bounds[-1]))
    return bounds


@pytest.mark.parametrize("box", ["cube", "T"])
def test_whole_sum(box):
    import torch_nfft_amd as tn
    s, f, _, batch = _whole_sources()
    near, far, terms = ([p[:, ..., 0, :] for p in part] for part in _reference(box))  # the forces' columns
    A = BOXES[box]
    assert _overlapping(s, A, RADIUS)[1] >= 1
    label = "nfft_ewald_rpy in %s" % box
    bounds = _whole_bounds(box, f, s, batch, near, far, label)
    kw = dict(splitting=_splitting(box), radius=RADIUS, cutoff=4, fractional=A is not None)
    got = tn.nfft_ewald_rpy(_cuda(f), _cuda(s), _cuda(batch), gradient=True, **kw)
    first = tn.nfft_ewald_rpy(_cuda(f), _cuda(s), _cuda(batch), **kw)
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
    # the power: a sum of products, each u good to its bound (Cauchy-Schwarz per point set, all columns together); positive
    P = tn.nfft_ewald_rpy_power(_cuda(f), _cuda(s), _cuda(batch), **kw).cpu().numpy()
    tn.ops.check_status()
    want = rr.power(f, uw, batch)
    assert P.shape == (2, 2) and (want > 0).all()
    bound = 0.5 * np.linalg.norm(f, axis=1).max() * bounds[0] * math.sqrt(343.0)
    print("%s power: %s, |error| %.3e, bound %.3e" % (label, P.ravel(), np.abs(P - want).max(), bound))
    assert np.abs(P - want).max() <= bound and (P > 0).all()


@pytest.mark.parametrize("box", ["cube", "T"])
def test_converged_sum(box):
    """One small set against the sum carried to convergence: |device - converged| <= |device - algorithm| + |algorithm -
    converged|, the first within the whole sum's bound, the second computed here in float64.  The set is the 4^3 cluster
    across the box corner of the Stokeslet tests; with a = 0.035 the closest of its pairs overlap."""
    import torch_nfft_amd as tn
    A = BOXES[box]
    a = 0.035
    rng = np.random.default_rng(9)
    s = dr.jittered_lattice(rng, 4, 0.1, 0.02, centre=0.45).reshape(-1, 3)
    assert (s > 0.5).any(0).all() and dr.min_separation(s, A) >= 0.04 and _overlapping(s, A, a)[1] >= 1
    f = rr.near_forces(10, 64, ())
    alpha, r_c, N = WHOLE[box]
    near, far = rr.near(f, s, A, None, alpha, r_c, a), rr.far(f, s, A, None, alpha, a, N)
    terms = rr.terms(f, 64, alpha, a)
    conv = rr.converged(f, s, A, a)
    bounds = _whole_bounds(box, f, s, None, near, far, "converged sum in %s" % box, a)
    got = tn.nfft_ewald_rpy(_cuda(f), _cuda(s), splitting=_splitting(box), radius=a, cutoff=4, gradient=True, fractional=A is not None)
    tn.ops.check_status()
    for what, g, n_, f_, t_, c, bound in zip(NAMES, got, near, far, terms, conv, bounds):
        own = float(np.linalg.norm(n_ + f_ + t_ - c))
        err = float(np.linalg.norm(g.cpu().numpy() - c))
        print("nfft_ewald_rpy %s in %s: |device - converged| %.3e (rel %.3e), bound %.3e + the algorithm's own %.3e"
              % (what, box, err, err / np.linalg.norm(c), bound, own))
        assert abs(err - own) <= bound  # (both sides of the triangle inequality: own - bound <= err <= own + bound)


@pytest.mark.parametrize("a", [0.05, 0.1])
def test_single_sphere_mobility(a):
    """One sphere in the unit cube at (8, 0.3, 32): u = (4 / (3 a)) (1 - 2.8372974795 a + (4 pi / 3) a^3) f, within the whole sum's
    bound (no pair: the far part's alone) plus the algorithm's own truncation in float64"""
    import torch_nfft_amd as tn
    s = np.array([[0.1, -0.2, 0.35]], np.float32)
    f = np.array([[0.3, -1.1, 0.7]], np.float32)
    alpha, r_c, N = WHOLE["cube"]
    near, far = rr.near(f, s, None, None, alpha, r_c, a, order=2), rr.far(f, s, None, None, alpha, a, N)
    assert np.linalg.norm(near[0]) == 0.0
    bound = _whole_bounds("cube", f, s, None, near, far, "one sphere of radius %g in the unit cube" % a, a)[0]
    coefficient = 4.0 / (3.0 * a) * (1.0 - HASIMOTO * a + 4.0 * math.pi / 3.0 * a ** 3)
    want = coefficient * f.astype(np.float64)
    own = float(np.linalg.norm(far[0] + rr.terms(f, 1, alpha, a)[0] - want))
    u = tn.nfft_ewald_rpy(_cuda(f), _cuda(s), splitting=_splitting("cube"), radius=a, cutoff=4)
    tn.ops.check_status()
    err = float(np.linalg.norm(u.cpu().numpy() - want))
    print("one sphere of radius %g in the unit cube: u / f = %s, want %.7f, |error| %.3e, bound %.3e + the algorithm's own %.3e"
          % (a, u.cpu().numpy() / f, coefficient, err, bound, own))
    assert err <= bound + own


@pytest.mark.parametrize("box", ["cube", "T"])
def test_autograd(box):
    """(df, dpos) of (u g).sum() and dpos of the power against the formulas of section 7m evaluated with rpy_ref, with the
    bounds of tests/test_gpu_stokeslet.py::test_autograd:
        |df - u[g]| <= b_u,     |dpos - want| <= sqrt(4) max |f_i, g_i| b_G,
    times |A|_2 for fractional input."""
    import torch_nfft_amd as tn
    s, f, g, batch = _whole_sources()
    near, far, terms = _reference(box)
    A = BOXES[box]
    f4 = np.stack([f, g], 2)
    label = "rpy autograd in %s" % box
    b_u, b_G = _whole_bounds(box, f4, s, batch, near, far, label)
    u, G = (n_ + f_ + t_ for n_, f_, t_ in zip(near, far, terms))  # [n, 3, (3,) 2 (f, g), 2]
    fractional = A is not None
    kw = dict(splitting=_splitting(box), radius=RADIUS, cutoff=4, fractional=fractional)
    fd = _cuda(f).requires_grad_(True)
    xd = _cuda(s).requires_grad_(True)
    v = tn.nfft_ewald_rpy(fd, xd, _cuda(batch), **kw)
    df, dx = torch.autograd.grad((v * _cuda(g)).sum(), (fd, xd))
    tn.ops.check_status()
    assert df.shape == f.shape and dx.shape == s.shape
    scale = np.linalg.norm(A, 2) if fractional else 1.0
    weight = max(np.linalg.norm(f, axis=1).max(), np.linalg.norm(g, axis=1).max())
    want = rr.position_gradient(f, g, G[:, :, :, 0], G[:, :, :, 1])
    if fractional:
        want = want @ A.T
    for what, got, ref, bound in (("df", df, u[:, :, 1], b_u), ("dpos", dx, want, 2.0 * weight * b_G * scale)):
        err = float(np.linalg.norm(got.cpu().numpy() - ref))
        print("%s %s: |error| %.3e (rel %.3e), bound %.3e" % (label, what, err, err / np.linalg.norm(ref), bound))
        assert err <= bound
    # only the forces' gradient asked for: one order-1 evaluation of the weights
    v = tn.nfft_ewald_rpy(fd, xd.detach(), _cuda(batch), **kw)
    df1, = torch.autograd.grad((v * _cuda(g)).sum(), (fd,))
    tn.ops.check_status()
    assert float(np.linalg.norm(df1.cpu().numpy() - u[:, :, 1])) <= b_u
    # the power: g = f / 2, dP/dpos_i,b = sum_a f_i,a G[f]_i,ab summed over the columns: sqrt(2) max |f_i| b_G with the bound of
    # the forces' two columns alone (see the Stokeslet test)
    _, s_G = _whole_bounds(box, f, s, batch, [p[:, ..., 0, :] for p in near], [p[:, ..., 0, :] for p in far],
                           label + ", the forces alone")
    xe = _cuda(s).requires_grad_(True)
    P = tn.nfft_ewald_rpy_power(_cuda(f), xe, _cuda(batch), **kw)
    de, = torch.autograd.grad(P.sum(), xe)
    tn.ops.check_status()
    want = (f.astype(np.float64)[:, :, None] * G[:, :, :, 0]).sum(1).sum(2)
    if fractional:
        want = want @ A.T
    bound = math.sqrt(2.0) * np.linalg.norm(f, axis=1).max() * s_G * scale
    err = float(np.linalg.norm(de.cpu().numpy() - want))
    print("%s power dpos: |error| %.3e (rel %.3e), bound %.3e" % (label, err, err / np.linalg.norm(want), bound))
    assert err <= bound


def test_mobility_is_positive_definite_on_the_device():
    """32 spheres, four overlapping pairs among them, and the 96 unit forces as 96 columns of one call: the matrix is within
    the whole sum's bound b of the float64 algorithm's (Frobenius norm), symmetric within b, and its smallest eigenvalue
    is within sqrt(96) b of the reference's, which is positive"""
    import torch_nfft_amd as tn
    rng = np.random.default_rng(5)
    s = dr.jittered_lattice(rng, 4, 0.25, 0.05).reshape(-1, 3)[:32].copy()
    for i, sep in ((0, 0.5), (2, 1.0), (4, 1.5), (6, 1.9)):
        e = rng.standard_normal(3)
        s[i + 1] = s[i] + (sep * RADIUS * e / np.linalg.norm(e)).astype(np.float32)
    assert _overlapping(s, None, RADIUS)[1] == 4
    f = np.eye(96, dtype=np.float32).reshape(32, 3, 96)
    alpha, r_c, N = WHOLE["cube"]
    near, far = rr.near(f, s, None, None, alpha, r_c, RADIUS, order=1), rr.far(f, s, None, None, alpha, RADIUS, N, order=1)
    M = (near[0] + far[0] + rr.terms(f, 32, alpha, RADIUS, order=1)[0]).reshape(96, 96)
    lowest = np.linalg.eigvalsh(0.5 * (M + M.T))[0]
    assert lowest > 0.0 and np.abs(M - M.T).max() <= 1e-12 * np.abs(M).max()
    # (the bound of u alone: the order-2 emulation and yardstick give the same first entry)
    emu = rr.near_f32(f, s, None, None, alpha, r_c, RADIUS, order=1)[0]
    gate, term = rr.near_gate("u", emu, near[0], COMMITTED[0])
    yard = _yardstick_far("cube", f, s, None, RADIUS)[0]
    e_far = float(np.linalg.norm(yard - far[0]))
    bound = 2.0 * e_far + gate * float(np.linalg.norm(near[0]))
    got = tn.nfft_ewald_rpy(_cuda(f), _cuda(s), splitting=_splitting("cube"), radius=RADIUS, cutoff=4)
    tn.ops.check_status()
    D = got.cpu().numpy().astype(np.float64).reshape(96, 96)
    err, asym = float(np.linalg.norm(D - M)), float(np.linalg.norm(D - D.T))
    low = np.linalg.eigvalsh(0.5 * (D + D.T))[0]
    print("mobility of 32 spheres: e_far %.3e, near gate %.3e = max(4 x %.3e, %.3e), bound %.3e; |device - algorithm| %.3e, "
          "|M - M^T| %.3e, smallest eigenvalue %.6f against %.6f" % (e_far, gate, term, COMMITTED[0], bound, err, asym, low, lowest))
    assert err <= bound and asym <= bound
    assert abs(low - lowest) <= math.sqrt(96.0) * bound and low > 0.0


def test_second_derivative_refusals_and_empty_input():
    import torch_nfft_amd as tn
    s, f, _, batch = _whole_sources()
    sp = _splitting("cube")
    fd, xd, bd = _cuda(f).requires_grad_(True), _cuda(s).requires_grad_(True), _cuda(batch)
    u, G = tn.nfft_ewald_rpy(fd, xd, bd, splitting=sp, radius=RADIUS, gradient=True)
    assert u.requires_grad and not G.requires_grad
    df, dx = torch.autograd.grad(u.square().sum(), (fd, xd), create_graph=True)
    with pytest.raises(RuntimeError, match="differentiate twice|once_differentiable"):
        dx.square().sum().backward()
    tn.ops.check_status()
    with pytest.raises(AssertionError, match="batch"):
        tn.nfft_ewald_rpy(fd, xd, torch.zeros(343, device="cuda", requires_grad=True), splitting=sp, radius=RADIUS)
    with pytest.raises(TypeError, match="EwaldSplitting"):
        tn.nfft_ewald_rpy(fd, xd, bd, splitting=tn.DispersionSplitting(8.0, 0.3, 32), radius=RADIUS)
    with pytest.raises(ValueError, match="complex"):
        tn.nfft_ewald_rpy(fd.detach().to(torch.complex64), xd, bd, splitting=sp, radius=RADIUS)
    with pytest.raises(ValueError, match="fractional"):
        tn.nfft_ewald_rpy(fd, xd, bd, splitting=sp, radius=RADIUS, fractional=True)
    for bad in (None, 0.0, -0.05, 0.16):
        with pytest.raises(ValueError, match="radius"):
            tn.nfft_ewald_rpy(fd, xd, bd, splitting=sp, radius=bad)
    fs, xs = fd.detach(), xd.detach()
    for bad in (0.0, -0.05, float("nan"), float("inf"), 0.151):  # the radius refusals of the operator
        with pytest.raises(RuntimeError, match="Input mismatch"):
            tn.ops.nfft_ewald_rpy_near(xs, fs, bd, (), 5.0, 0.3, bad, 2)
    with pytest.raises(RuntimeError, match="Input mismatch"):
        tn.ops.nfft_ewald_rpy_near(xs, fs, bd, _box6(O), 5.0, 0.25, 0.126, 1)
    with pytest.raises(RuntimeError, match="Input mismatch"):
        tn.ops.nfft_ewald_rpy_near(xs, fs, bd, (), 5.0, 0.34, 0.05, 2)
    with pytest.raises(RuntimeError, match="Input mismatch"):
        tn.ops.nfft_ewald_rpy_near(xs, fs, bd, (), 5.0, 0.3, 0.05, 3)
    with pytest.raises(RuntimeError, match="Input mismatch"):
        tn.ops.nfft_ewald_rpy_near(xs, fs[:, :2].contiguous(), bd, (), 5.0, 0.3, 0.05, 1)
    with pytest.raises(RuntimeError, match="Input mismatch"):
        tn.ops.nfft_ewald_rpy_near(xs, fs, bd, _box6(O), 5.0, 0.3, 0.05, 1)
    tn.ops.check_status()
    assert tn.ops.nfft_ewald_rpy_near(xs, fs, bd, (), 5.0, 0.3, 0.15, 1).shape == (343, 3, 2)  # (2 a = r_cut is allowed)
    # empty input
    f0 = torch.zeros(0, 3, 2, device="cuda", requires_grad=True)
    x0 = torch.zeros(0, 3, device="cuda", requires_grad=True)
    u, G = tn.nfft_ewald_rpy(f0, x0, splitting=sp, radius=RADIUS, gradient=True)
    assert u.shape == (0, 3, 2) and G.shape == (0, 3, 3, 2)
    df0, dx0 = torch.autograd.grad(u.sum(), (f0, x0))
    assert df0.shape == (0, 3, 2) and dx0.shape == (0, 3)
    assert tn.nfft_ewald_rpy_power(f0, x0, splitting=sp, radius=RADIUS).shape == (1, 2)
    out = tn.ops.nfft_ewald_rpy_near(x0.detach(), torch.zeros(0, 3, 2, device="cuda"), None, (), 5.0, 0.3, 0.05, 2)
    assert out.shape == (0, 12, 2)
    tn.ops.check_status()
