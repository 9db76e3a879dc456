"""GPU tests of the Ewald sum in orthorhombic and triclinic boxes: the pair sweep
csrc/ewald_near_box.hip and nfft_ewald / nfft_ewald_energy with EwaldSplitting(box=...) against the float64 restatement
tests/ewald_box_ref.py, evaluated on the same float32 fractional positions.

Tolerances.  As in tests/test_gpu_ewald.py: each is 4x the largest rel_l2 of the first device run (the figure behind each
entry is in its comment); a first-run figure above 1e-4 would have been a defect, not a tolerance.  What these must not
hide is wrong by far more: a near sum that drops the off-diagonal entries of A by 0.26 .. 0.50, one that uses A^T by
0.12 .. 0.49, a missed wrap by 2e-2 and above.  Against the converged sum the bound is the triangle inequality with the
algorithm's own truncation error, no free number.
"""
import math

import numpy as np
import pytest
import torch

import ewald_box_ref as eb
import ewald_ref as er
from conftest import rel_l2

pytestmark = pytest.mark.gpu

NEAR_TOL = {  # 4 x the largest rel_l2 of the first device run (in brackets)
    "value": 2.0e-6,  # (5.01e-7: T at (14, 0.25), one set; 9.7e-8 .. 3.0e-7 on the thirteen other cases of 700 points)
    "field": 1.8e-6,  # (4.40e-7: T at (14, 0.25), ragged; 9.1e-8 .. 3.0e-7 on the others)
    "crowded_value": 6.7e-6,  # (1.67e-6)
    "crowded_field": 8.5e-6,  # (2.14e-6)
}
# The crowded corner loses its digits before the kernel is evaluated, as in the unit cube: the difference of two float32
# fractional positions on either side of a face is rounded at |ds| ~ 1 and then stands for a distance of ~ 0.03.
WHOLE_TOL = {  # the same for nfft_ewald (cutoff = 4) against the float64 algorithm
    "value": 2.1e-6,  # (5.16e-7: dq of the backward; the whole sums 4.68e-7 in T and 4.69e-7 in O, Cartesian input 4.56e-7)
    "field": 8.3e-7,  # (2.07e-7 in T; 1.98e-7 in O, Cartesian input 1.74e-7)
    # one or two values each, the difference of terms many times their size (2 alpha / sqrt(pi) = 18 and 24 against 2.8
    # and 3.5) whose far part carries the transform's error at cutoff = 4
    "fixed_point": 8.2e-6,  # (2.05e-6: primitive rock salt; one charge in S 1.11e-6 and 1.60e-6)
}
CARTESIAN_TOL = {  # the same for Cartesian input against fractional input: the float32 x = s A has lost the last bits of s
    "value": 1.3e-6,  # (3.31e-7)
    "field": 4.6e-6,  # (1.15e-6)
}

BOXES = {"T": eb.T, "O": eb.O, "S": eb.S}


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _six(A):
    return [A[0, 0], A[1, 0], A[1, 1], A[2, 0], A[2, 1], A[2, 2]]


def _splitting(A, alpha, r_c, N=32):
    import torch_nfft_amd as tn
    return tn.EwaldSplitting(alpha, r_c, N, box=A)


def _ragged_batch(rng, n):
    """three point sets, the middle one empty"""
    b = np.sort(rng.integers(0, 2, n)) * 2
    b[0], b[-1] = 0, 2
    return b.astype(np.int64)


def _values(rng, n, cols, complex_x):
    x = rng.standard_normal((n,) + cols)
    if complex_x:
        return (x + 1j * rng.standard_normal((n,) + cols)).astype(np.complex64)
    return x.astype(np.float32)


def _box_points(rng, n):
    """n float32 FRACTIONAL points uniform in the box and, among the first hundred (one point set of the ragged cases),
    every edge case of the wrap (those of tests/test_gpu_ewald.py)"""
    x = (rng.random((n, 3)) - 0.5).astype(np.float32)
    x[40:60] = x[0:20]                                    # exact duplicates: r = 0
    below = np.nextafter(np.float32(0.5), np.float32(0))  # the largest float32 below 1/2
    for a in range(3):
        x[60 + a, a] = -0.5                               # exactly on the lower face
        x[63 + a, a] = below
        x[66 + a] = x[60 + a] + np.float32(0.01) * rng.random(3).astype(np.float32)  # ... each with a close neighbour
        x[69 + a] = x[63 + a] - np.float32(0.01) * rng.random(3).astype(np.float32)
    # (one in the box's upper corner and none in the lower one: the two would be images 5e-8 apart, a distance that
    # float32 positions cannot hold across the wrap)
    x[63, :] = below
    x[72:80] += np.float32(0.7)                           # given outside the box: must act as their images
    x[80:88] -= np.float32(1.2)
    for a in range(3):                                    # a pair straddling each face
        y = (rng.random(3) - 0.5).astype(np.float32)
        x[88 + 2 * a] = y
        x[89 + 2 * a] = y + np.float32(0.003)
        x[88 + 2 * a, a] = 0.49
        x[89 + 2 * a, a] = -0.49
    return x


# box, alpha, r_c, the cells, ragged, cols, complex, field
CASES = [
    ("O", 14.0, 0.25, (4, 5, 3), False, (), False, True),   # (all three counts differ: swapped counts show)
    ("O", 14.0, 0.25, (4, 5, 3), True, (3,), False, False),
    ("O", 14.0, 0.25, (4, 5, 3), True, (2,), True, True),
    ("T", 12.0, 0.3, (3, 3, 3), False, (2,), True, True),
    ("T", 12.0, 0.3, (3, 3, 3), True, (), False, True),
    ("T", 14.0, 0.25, (3, 4, 3), True, (3,), False, True),
    ("T", 14.0, 0.25, (3, 4, 3), False, (), False, False),
    ("T", 30.0, 0.12, (7, 8, 7), True, (2,), True, False),
    ("T", 30.0, 0.12, (7, 8, 7), False, (3,), False, True),
    ("S", 16.0, 0.22, (3, 4, 4), False, (), False, True),    # (a tilt of a full box length)
    ("S", 16.0, 0.22, (3, 4, 4), True, (3,), False, True),
    ("S", 16.0, 0.22, (3, 4, 4), True, (2,), True, True),
]


@pytest.mark.parametrize("name,alpha,r_c,cells,ragged,cols,complex_x,field", CASES)
def test_near_sweep_against_brute_force(name, alpha, r_c, cells, ragged, cols, complex_x, field):
    import torch_nfft_amd as tn
    A = BOXES[name]
    assert _splitting(A, alpha, r_c, 4).cells == cells
    rng = np.random.default_rng(int(alpha) * 100 + len(cols) + 10 * ragged + ord(name))
    n = 700
    s = _box_points(rng, n)
    q = _values(rng, n, cols, complex_x)
    batch = _ragged_batch(rng, n) if ragged else None
    if batch is not None:
        assert (batch[:100] == 0).all()  # the edge cases share a point set
    z, f = tn.ops.nfft_ewald_near_box(_cuda(s), _cuda(q), _cuda(batch), _six(A), alpha, r_c, field)
    tn.ops.check_status()
    dtype = torch.complex64 if complex_x else torch.float32
    assert z.shape == q.shape and z.dtype == dtype
    ref = eb.near_sum(q, s, A, batch, alpha, r_c)
    err = rel_l2(z.cpu().numpy(), ref)
    print("ewald near, box %s (%g, %g) ragged=%d cols=%s complex=%d: value rel_l2 %.3e (|ref| %.3e)"
          % (name, alpha, r_c, ragged, cols, complex_x, err, np.linalg.norm(ref)))
    assert np.linalg.norm(ref) > 0
    assert err <= NEAR_TOL["value"]
    if field:
        assert f.shape == (n, 3) + cols and f.dtype == dtype
        fref = eb.near_field(q, s, A, batch, alpha, r_c)
        ferr = rel_l2(f.cpu().numpy(), fref)
        print("ewald near, box %s (%g, %g) ragged=%d cols=%s complex=%d: field rel_l2 %.3e (|ref| %.3e)"
              % (name, alpha, r_c, ragged, cols, complex_x, ferr, np.linalg.norm(fref)))
        assert np.linalg.norm(fref) > 0
        assert ferr <= NEAR_TOL["field"]
    else:
        assert f.numel() == 0


@pytest.mark.parametrize("alpha,r_c", [(12.0, 0.3), (30.0, 0.12)])
def test_identity_box(alpha, r_c):
    """box = (1, 1, 1): the brute-force sums of the unit cube, and the unit-cube kernel on the same points"""
    import torch_nfft_amd as tn
    rng = np.random.default_rng(5)
    n = 700
    s = _box_points(rng, n)
    q = _values(rng, n, (3,), False)
    batch = _ragged_batch(rng, n)
    z, f = tn.ops.nfft_ewald_near_box(_cuda(s), _cuda(q), _cuda(batch), [1, 0, 1, 0, 0, 1], alpha, r_c, True)
    zc, fc = tn.ops.nfft_ewald_near(_cuda(s), _cuda(q), _cuda(batch), alpha, r_c, True)
    tn.ops.check_status()
    ref, fref = er.near_sum(q, s, batch, alpha, r_c), er.near_field(q, s, batch, alpha, r_c)
    errs = (rel_l2(z.cpu().numpy(), ref), rel_l2(f.cpu().numpy(), fref),
            rel_l2(z.cpu().numpy(), zc.cpu().numpy()), rel_l2(f.cpu().numpy(), fc.cpu().numpy()))
    print("identity box (%g, %g): value %.3e field %.3e vs float64; value %.3e field %.3e vs the unit-cube kernel"
          % ((alpha, r_c) + errs))
    assert np.linalg.norm(ref) > 0 and np.linalg.norm(fref) > 0
    assert errs[0] <= NEAR_TOL["value"] and errs[1] <= NEAR_TOL["field"]
    assert errs[2] <= NEAR_TOL["value"] and errs[3] <= NEAR_TOL["field"]


@pytest.fixture(scope="module")
def crowded():
    """3000 points in a fractional cube of edge 0.06 centred on the corner (1/2, 1/2, 1/2) of the box T: after wrapping
    they fill the eight corner cells of the 3^3 grid (~375 each: three items and two LDS tiles per cell), every pair is
    closer than r_c and most of them through a wrap"""
    rng = np.random.default_rng(7)
    s = (0.5 + (rng.random((3000, 3)) - 0.5) * 0.06).astype(np.float32)
    q = rng.standard_normal(3000).astype(np.float32)
    return s, q


def test_crowded_corner(crowded):
    import torch_nfft_amd as tn
    s, q = crowded
    assert (s > 0.5).any(0).all() and (s < 0.5).any(0).all()
    z, f = tn.ops.nfft_ewald_near_box(_cuda(s), _cuda(q), None, _six(eb.T), 12.0, 0.3, True)
    tn.ops.check_status()
    ref, fref = eb.near_sum(q, s, eb.T, None, 12.0, 0.3), eb.near_field(q, s, eb.T, None, 12.0, 0.3)
    err, ferr = rel_l2(z.cpu().numpy(), ref), rel_l2(f.cpu().numpy(), fref)
    print("ewald near, box T, crowded corner: value rel_l2 %.3e, field rel_l2 %.3e" % (err, ferr))
    assert err <= NEAR_TOL["crowded_value"] and ferr <= NEAR_TOL["crowded_field"]


def test_two_calls_are_bitwise_equal(crowded):
    import torch_nfft_amd as tn
    s, q = crowded
    sd, qd = _cuda(s), _cuda(np.stack([q, -q[::-1], q * q], 1))
    z1, f1 = tn.ops.nfft_ewald_near_box(sd, qd, None, _six(eb.T), 12.0, 0.3, True)
    z2, f2 = tn.ops.nfft_ewald_near_box(sd, qd, None, _six(eb.T), 12.0, 0.3, True)
    assert bool(z1.any()) and bool(f1.any())
    assert torch.equal(z1, z2) and torch.equal(f1, f2)
    z3, _ = tn.ops.nfft_ewald_near_box(sd, qd, None, _six(eb.T), 12.0, 0.3, False)  # value only: the same pairs
    assert torch.equal(z1, z3)


def _fixed_point(what, q, s, A, split, constant):
    """phi / q of nfft_ewald(fractional=True) against the lattice constant: the float64 algorithm's own truncation is
    checked against 1e-8 (the splits are chosen for it), the device against the algorithm, then the triangle inequality"""
    import torch_nfft_amd as tn
    alpha, r_c, N = split
    sp = _splitting(A, alpha, r_c, N)
    phi, E = tn.nfft_ewald(_cuda(q), _cuda(s), splitting=sp, cutoff=4, field=True, fractional=True)
    tn.ops.check_status()
    alg = eb.exact_algorithm(q, s, A, None, alpha, r_c, N)
    own = np.abs(alg / q - constant).max() / abs(constant)
    phi = phi.cpu().numpy()
    e_alg, e_const = rel_l2(phi, alg), np.abs(phi / q - constant).max() / abs(constant)
    print("%s: phi / q = %s (%.7f), relative error %.3e, vs the float64 algorithm %.3e (its own %.1e)"
          % (what, phi / q, constant, e_const, e_alg, own))
    assert own <= 1e-8
    assert e_alg <= WHOLE_TOL["fixed_point"] and e_const <= WHOLE_TOL["fixed_point"] + own
    return sp, E.cpu().numpy()


@pytest.mark.parametrize("pos", [(0.0, 0.0, 0.0), (0.31, -0.47, 0.123)])
def test_one_charge_in_the_sheared_cell(pos):
    """the cell S spans the cubic lattice: phi = -2.8373 q wherever the charge sits, and no field"""
    q, s = np.array([1.5], dtype=np.float32), np.array([pos], dtype=np.float32)
    sp, E = _fixed_point("one charge in S at %s" % (pos,), q, s, eb.S, (16.0, 0.22, 64), er.CUBIC_LATTICE)
    # The field of a lattice of one charge vanishes by symmetry: what the device returns is the error of the far transform,
    # which adds |q| sum_k |2 pi kappa_a b_k| in magnitudes on every axis to arrive at zero (as in tests/test_gpu_ewald.py).
    scale = float(sp.field_coeffs()[..., 1:].abs().sum((0, 1, 2)).max())
    print("one charge in S: |E| / |q| = %.3e, scale %.3e" % (np.abs(E).max() / 1.5, scale))
    assert np.abs(E).max() <= WHOLE_TOL["field"] * 1.5 * scale


def test_primitive_rock_salt():
    """two ions in the primitive fcc cell, brought to lower-triangular form by QR: phi_i = -2 M q_i"""
    A, _ = eb.lower_triangular(eb.ROCK_SALT_PRIMITIVE)
    q = np.array([1.0, -1.0], dtype=np.float32)
    s = np.array([[0.0, 0.0, 0.0], [-0.5, -0.5, -0.5]], dtype=np.float32)
    _fixed_point("primitive rock salt", q, s, A, (21.0, 0.19, 48), -2.0 * er.MADELUNG_NACL)


WHOLE = {"T": (12.0, 0.3, 32), "O": (14.0, 0.25, 48)}


@pytest.fixture(scope="module")
def whole():
    """800 charges in two point sets, neither neutral, fractional float32 positions; per box the float64 algorithm and
    the converged sum (one shell of images around the wrapped difference: the next is at 1.5 w_a >= 1.2, where
    erfc(6 r) / r is below 1e-23)"""
    rng = np.random.default_rng(3)
    n = 800
    s = (rng.random((n, 3)) - 0.5).astype(np.float32)
    q = rng.standard_normal(n).astype(np.float32)
    batch = (np.arange(n) >= 370).astype(np.int64)
    done = {}

    def get(name):
        if name not in done:
            alpha, r_c, N = WHOLE[name]
            done[name] = (eb.exact_algorithm(q, s, BOXES[name], batch, alpha, r_c, N, field=True),
                          eb.converged(q, s, BOXES[name], batch, nimg=1, field=True))
        return done[name]

    return s, q, batch, get


@pytest.mark.parametrize("name", ["T", "O"])
def test_whole_sum_and_field(whole, name):
    import torch_nfft_amd as tn
    s, q, batch, get = whole
    alg, conv = get(name)
    alpha, r_c, N = WHOLE[name]
    sp = _splitting(BOXES[name], alpha, r_c, N)
    phi, E = tn.nfft_ewald(_cuda(q), _cuda(s), _cuda(batch), splitting=sp, cutoff=4, field=True, fractional=True)
    only = tn.nfft_ewald(_cuda(q), _cuda(s), _cuda(batch), splitting=sp, cutoff=4, fractional=True)
    tn.ops.check_status()
    assert phi.shape == (800,) and E.shape == (800, 3) and phi.dtype == E.dtype == torch.float32
    for what, got, k in (("value", phi, 0), ("value", only, 0), ("field", E, 1)):
        got = got.cpu().numpy()
        e_alg, e_own, e_conv = rel_l2(got, alg[k]), rel_l2(alg[k], conv[k]), rel_l2(got, conv[k])
        print("nfft_ewald, box %s, %s: rel_l2 vs the float64 algorithm %.3e, vs the converged sum %.3e (the algorithm's "
              "own %.3e)" % (name, what, e_alg, e_conv, e_own))
        assert e_alg <= WHOLE_TOL[what]
        assert e_conv <= e_alg + 1.1 * e_own
    U = tn.nfft_ewald_energy(_cuda(q), _cuda(s), _cuda(batch), splitting=sp, cutoff=4, fractional=True).cpu().numpy()
    want = np.array([0.5 * (q[batch == b] * alg[0][batch == b]).sum() for b in (0, 1)])
    assert U.shape == (2,)
    # (a sum of 400 products, each good to WHOLE_TOL of |q| |phi|: Cauchy-Schwarz)
    for b in (0, 1):
        sel = batch == b
        print("energy of set %d: %.7g (%.7g)" % (b, U[b], want[b]))
        assert abs(U[b] - want[b]) <= WHOLE_TOL["value"] * 0.5 * np.linalg.norm(q[sel]) * np.linalg.norm(alg[0][sel])


@pytest.fixture(scope="module")
def small():
    """300 charges in two point sets in the box T, two real columns, a weight for phi: float32 fractional positions s0,
    their float32 CARTESIAN positions x = s0 A (float64 product, rounded once), the float32 fractional positions s that x
    converts back to (the same way: s0 with its last bits changed) and the float64 algorithm's fields of both on s"""
    rng = np.random.default_rng(4)
    n = 300
    s0 = (rng.random((n, 3)) - 0.5).astype(np.float32)
    x = (s0.astype(np.float64) @ eb.T).astype(np.float32)
    s = (x.astype(np.float64) @ np.linalg.inv(eb.T)).astype(np.float32)
    q = rng.standard_normal((n, 2)).astype(np.float32)
    g = rng.standard_normal((n, 2)).astype(np.float32)
    batch = (np.arange(n) >= 140).astype(np.int64)
    aq = eb.exact_algorithm(q, s, eb.T, batch, 12.0, 0.3, 32, field=True)
    ag = eb.exact_algorithm(g, s, eb.T, batch, 12.0, 0.3, 32, field=True)
    return x, s, q, g, batch, aq, ag, s0


def test_cartesian_input(small):
    """nfft_ewald(q, s0 A) against fractional=True on s0.  The two differ by what the float32 Cartesian positions lose:
    the s that they convert back to is s0 with its last bits changed"""
    import torch_nfft_amd as tn
    x, s, q, g, batch, aq, ag, s0 = small
    assert 0 < np.abs(s - s0).max() <= 2.0 ** -22
    sp = _splitting(eb.T, 12.0, 0.3)
    phi_x, E_x = tn.nfft_ewald(_cuda(q), _cuda(x), _cuda(batch), splitting=sp, field=True)
    phi_s, E_s = tn.nfft_ewald(_cuda(q), _cuda(s0), _cuda(batch), splitting=sp, field=True, fractional=True)
    tn.ops.check_status()
    e_phi, e_E = rel_l2(phi_x.cpu().numpy(), phi_s.cpu().numpy()), rel_l2(E_x.cpu().numpy(), E_s.cpu().numpy())
    e_alg, e_algE = rel_l2(phi_x.cpu().numpy(), aq[0]), rel_l2(E_x.cpu().numpy(), aq[1])
    print("Cartesian input: value %.3e field %.3e vs fractional input; value %.3e field %.3e vs float64"
          % (e_phi, e_E, e_alg, e_algE))
    assert np.linalg.norm(aq[0]) > 0
    assert e_phi <= CARTESIAN_TOL["value"] and e_E <= CARTESIAN_TOL["field"]
    assert e_alg <= WHOLE_TOL["value"] and e_algE <= WHOLE_TOL["field"]
    # positions a lattice vector away are the same charges: the float64 algorithm on what they convert to (float32
    # positions of magnitude 2 have lost a bit or two, so these are not quite the fractional positions above)
    shift = (x.astype(np.float64) + 2.0 * eb.T[1] - eb.T[2]).astype(np.float32)
    s_m = (shift.astype(np.float64) @ np.linalg.inv(eb.T)).astype(np.float32)
    assert np.abs(s_m).max() > 1.5
    phi_m = tn.nfft_ewald(_cuda(q), _cuda(shift), _cuda(batch), splitting=sp)
    e_m = rel_l2(phi_m.cpu().numpy(), eb.exact_algorithm(q, s_m, eb.T, batch, 12.0, 0.3, 32))
    print("Cartesian input moved by 2 a_2 - a_3: value %.3e vs float64" % e_m)
    assert e_m <= WHOLE_TOL["value"]


def test_autograd(small):
    import torch_nfft_amd as tn
    x, s, q, g, batch, aq, ag, _ = small
    sp = _splitting(eb.T, 12.0, 0.3)
    qd, xd, gd, bd = _cuda(q).requires_grad_(True), _cuda(x).requires_grad_(True), _cuda(g), _cuda(batch)
    phi = tn.nfft_ewald(qd, xd, bd, splitting=sp)
    dq, dx = torch.autograd.grad((phi * gd).sum(), (qd, xd))
    tn.ops.check_status()
    # dq: the operator applied to g -- the device's own (two evaluations, each within WHOLE_TOL) and the float64 one
    own = tn.nfft_ewald(gd, xd.detach(), bd, splitting=sp)
    e_own, e_ref = rel_l2(dq.cpu().numpy(), own.cpu().numpy()), rel_l2(dq.cpu().numpy(), ag[0])
    print("nfft_ewald in T, dq: rel_l2 vs the operator on g %.3e, vs float64 %.3e" % (e_own, e_ref))
    assert e_own <= 2 * WHOLE_TOL["value"] and e_ref <= WHOLE_TOL["value"]
    # Cartesian dpos_i = -sum_c (g_ic E[q_c]_i + q_ic E[g_c]_i); each field is good to WHOLE_TOL["field"] in l2 and is
    # weighted by at most max |g| or max |q|
    want = -(g[:, None, :] * aq[1] + q[:, None, :] * ag[1]).sum(2)
    bound = WHOLE_TOL["field"] * (np.abs(g).max() * np.linalg.norm(aq[1]) + np.abs(q).max() * np.linalg.norm(ag[1]))
    err = np.linalg.norm(dx.cpu().numpy() - want)
    print("nfft_ewald in T, dpos: |error| %.3e, bound %.3e, rel_l2 %.3e" % (err, bound, rel_l2(dx.cpu().numpy(), want)))
    assert dx.shape == (300, 3) and err <= bound
    # only one of the two asked for
    dq1, = torch.autograd.grad((tn.nfft_ewald(qd, xd.detach(), bd, splitting=sp) * gd).sum(), qd)
    assert rel_l2(dq1.cpu().numpy(), ag[0]) <= WHOLE_TOL["value"]
    dx1, = torch.autograd.grad((tn.nfft_ewald(qd.detach(), xd, bd, splitting=sp) * gd).sum(), xd)
    assert np.linalg.norm(dx1.cpu().numpy() - want) <= bound
    # fractional positions: dL/ds = (dL/dx) A^T, the bound stretched by at most |A|_2
    sd = _cuda(s).requires_grad_(True)
    ds, = torch.autograd.grad((tn.nfft_ewald(qd.detach(), sd, bd, splitting=sp, fractional=True) * gd).sum(), sd)
    err_s = np.linalg.norm(ds.cpu().numpy() - want @ eb.T.T)
    print("nfft_ewald in T, ds: |error| %.3e, bound %.3e" % (err_s, bound * np.linalg.norm(eb.T, 2)))
    assert ds.shape == (300, 3) and err_s <= bound * np.linalg.norm(eb.T, 2)


def test_forces_of_the_energy(small):
    """-dU/dx_i = sum_c q_ic E_ic, Cartesian"""
    import torch_nfft_amd as tn
    x, s, q, g, batch, aq, ag, _ = small
    sp = _splitting(eb.T, 12.0, 0.3)
    qd, xd, bd = _cuda(q), _cuda(x).requires_grad_(True), _cuda(batch)
    U = tn.nfft_ewald_energy(qd, xd, bd, splitting=sp)
    assert U.shape == (2, 2)
    dx, = torch.autograd.grad(U.sum(), xd)
    _, E = tn.nfft_ewald(qd, xd.detach(), bd, splitting=sp, field=True)
    assert not E.requires_grad
    force = (qd.unsqueeze(1) * E).sum(2).cpu().numpy()
    want = (q[:, None, :] * aq[1]).sum(2)
    bound = WHOLE_TOL["field"] * np.abs(q).max() * np.linalg.norm(aq[1])
    e_dev, e_ref = np.linalg.norm(-dx.cpu().numpy() - force), np.linalg.norm(-dx.cpu().numpy() - want)
    print("forces in T: |autograd - q E| %.3e, |autograd - float64| %.3e, bound %.3e" % (e_dev, e_ref, bound))
    assert e_ref <= bound and e_dev <= 2 * bound


def test_second_derivative_and_refusals(small):
    import torch_nfft_amd as tn
    x, s, q, g, batch, _, _, _ = small
    sp = _splitting(eb.T, 12.0, 0.3)
    qd, xd, bd = _cuda(q).requires_grad_(True), _cuda(x).requires_grad_(True), _cuda(batch)
    phi, E = tn.nfft_ewald(qd, xd, bd, splitting=sp, field=True)
    assert phi.requires_grad and not E.requires_grad
    dq, dx = torch.autograd.grad(phi.square().sum(), (qd, xd), create_graph=True)
    with pytest.raises(RuntimeError, match="differentiate twice|once_differentiable"):
        dx.square().sum().backward()
    wmin = eb.widths(eb.T).min()
    upper, zero = eb.T.copy(), eb.T.copy()
    upper[1, 2] = 0.01
    zero[0, 0] = 0.0
    for kw in (dict(r_cut=wmin / 3 * (1 + 1e-6)), dict(box=upper), dict(box=zero)):
        args = dict(alpha=12.0, r_cut=0.3, bandwidth=16, box=eb.T)
        args.update(kw)
        with pytest.raises(ValueError):
            tn.EwaldSplitting(**args)
    with pytest.raises(ValueError, match="fractional"):
        tn.nfft_ewald(qd, xd, bd, splitting=tn.EwaldSplitting(12.0, 0.3, 16), fractional=True)
    with pytest.raises(AssertionError, match="box requires grad"):
        tn.EwaldSplitting(12.0, 0.3, 16, box=torch.tensor(eb.T, device="cuda", requires_grad=True))
    with pytest.raises(AssertionError, match="batch"):
        tn.nfft_ewald(qd, xd, torch.zeros(300, device="cuda", requires_grad=True), splitting=sp)
    pd, qq = xd.detach(), qd.detach()
    with pytest.raises(RuntimeError, match="Input mismatch"):
        tn.ops.nfft_ewald_near_box(pd, qq, bd, _six(eb.T), 12.0, wmin / 3 * (1 + 1e-6), False)
    with pytest.raises(RuntimeError, match="Input mismatch"):
        tn.ops.nfft_ewald_near_box(pd, qq, bd, _six(zero), 12.0, 0.2, False)
    with pytest.raises(RuntimeError, match="Input mismatch"):
        tn.ops.nfft_ewald_near_box(pd, qq, bd, [1.0, 1.0, 1.0], 12.0, 0.3, False)
    with pytest.raises(RuntimeError, match="Input mismatch"):
        tn.ops.nfft_ewald_near_box(pd[:, :2].contiguous(), qq, bd, _six(eb.T), 12.0, 0.3, False)


def test_empty_input_and_box_none():
    import torch_nfft_amd as tn
    sp = _splitting(eb.T, 12.0, 0.3, 16)
    q = torch.zeros(0, 2, device="cuda", requires_grad=True)
    x = torch.zeros(0, 3, device="cuda", requires_grad=True)
    for fractional in (False, True):
        phi, E = tn.nfft_ewald(q, x, splitting=sp, field=True, fractional=fractional)
        assert phi.shape == (0, 2) and E.shape == (0, 3, 2)
        dq, dx = torch.autograd.grad(phi.sum(), (q, x))
        assert dq.shape == (0, 2) and dx.shape == (0, 3)
    z, f = tn.ops.nfft_ewald_near_box(x.detach(), q.detach(), None, _six(eb.T), 12.0, 0.3, True)
    assert z.shape == (0, 2) and f.shape == (0, 3, 2) and z.dtype == torch.float32
    z, f = tn.ops.nfft_ewald_near_box(x.detach(), torch.zeros(0, device="cuda", dtype=torch.complex64), None, _six(eb.T),
                                      12.0, 0.3, False)
    assert z.shape == (0,) and z.dtype == torch.complex64 and f.numel() == 0
    assert tn.nfft_ewald_energy(q.detach(), x.detach(), splitting=sp).shape == (1, 2)
    # box=None is the splitting as it was: the coefficients restated the old way, bit for bit
    N, alpha = 32, 12.0
    k = torch.arange(-(N // 2), N // 2, dtype=torch.float64)
    k2 = (k * k).reshape(N, 1, 1) + (k * k).reshape(1, N, 1) + (k * k).reshape(1, 1, N)
    b = torch.exp(-(math.pi / alpha) ** 2 * k2) / (math.pi * k2.clamp(min=1.0))
    b[N // 2, N // 2, N // 2] = 0.0
    b[0, :, :] = 0.0
    b[:, 0, :] = 0.0
    b[:, :, 0] = 0.0
    old = tn.EwaldSplitting(alpha, 0.3, N)
    assert old.box is None and torch.equal(old.coeffs, b.to(torch.float32).cuda())
