"""GPU tests of the Ewald sum for the periodic 1/r: the wrapped pair sweep csrc/ewald_near.hip and
nfft_ewald / nfft_ewald_energy against the float64 restatement tests/ewald_ref.py.

Tolerances.  The device evaluates erfc(alpha r) / r and its slope in float32, the restatement in float64 on the same float32
positions.  NEAR_TOL and WHOLE_TOL are 4x the largest rel_l2 of the first device run (the figure behind each entry is in its
comment), the project's convention (tests/test_gpu_nearfield.py); a first-run figure above 1e-4 would have been a defect,
not a tolerance.  A near sum that misses the wrap on one side of one axis is wrong by 2e-2 .. 3e-2 on uniform points, with no
wrap at all by 0.23: neither hides under these.  Against the converged sum the bound is the triangle inequality with the
algorithm's own truncation error, no free number.
"""
import numpy as np
import pytest
import torch

import ewald_ref as er
from conftest import rel_l2

pytestmark = pytest.mark.gpu

NEAR_TOL = {  # 4 x the largest rel_l2 of the first device run (in brackets)
    "value": 6.4e-6,  # (1.61e-6: the crowded corner; 1.1e-7 .. 6.2e-7 on the nine uniform cases)
    "field": 8.9e-6,  # (2.23e-6: the crowded corner; 1.9e-7 .. 4.9e-7 on the uniform cases)
}
# The crowded corner loses its digits before the kernel is evaluated: the difference of two float32 positions on either
# side of a face is rounded at |d| ~ 1 (3e-8 absolute) and then stands for a distance of ~ 0.03 (1e-6 relative).
WHOLE_TOL = {  # the same for nfft_ewald (cutoff = 4) against the float64 algorithm
    "value": 1.9e-6,  # (4.67e-7; dq of the backward 4.85e-7; the fixed points: NaCl 7.1e-7, one charge 1.2e-6 and 8e-8)
    "field": 9.4e-7,  # (2.35e-7)
}


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _splitting(alpha, r_c, N=32):
    import torch_nfft_amd as tn
    return tn.EwaldSplitting(alpha, r_c, N)


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
    """n float32 points uniform in the box and, among the first hundred (one point set of the ragged cases), every edge case
    of the wrap"""
    x = (rng.random((n, 3)) - 0.5).astype(np.float32)
    x[40:60] = x[0:20]                                    # exact duplicates: r = 0
    below = np.nextafter(np.float32(0.5), np.float32(0))  # the largest float32 below 1/2
    for a in range(3):
        x[60 + a, a] = -0.5                               # exactly on the lower face
        x[63 + a, a] = below
        x[66 + a] = x[60 + a] + np.float32(0.01) * rng.random(3).astype(np.float32)  # ... each with a close neighbour
        x[69 + a] = x[63 + a] - np.float32(0.01) * rng.random(3).astype(np.float32)
    # (and one in the box's upper corner.  Not one in the lower corner as well: the two would be images 5e-8 apart, a
    # distance that float32 positions cannot hold across the wrap, with a weight 1 / r that drowns every other pair)
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


# alpha, r_c (G = floor(1 / r_c): 3, 4, 8), ragged, cols, complex, field
CASES = [
    (12.0, 0.3, False, (), False, True),
    (12.0, 0.3, True, (3,), False, False),
    (12.0, 0.3, False, (2,), True, True),
    (14.0, 0.25, True, (), False, True),
    (14.0, 0.25, False, (3,), False, True),
    (14.0, 0.25, True, (2,), True, False),
    (30.0, 0.12, False, (), False, False),
    (30.0, 0.12, True, (3,), False, True),
    (30.0, 0.12, True, (2,), True, True),
]


@pytest.mark.parametrize("alpha,r_c,ragged,cols,complex_x,field", CASES)
def test_near_sweep_against_brute_force(alpha, r_c, ragged, cols, complex_x, field):
    import torch_nfft_amd as tn
    rng = np.random.default_rng(int(alpha) * 100 + len(cols) + 10 * ragged)
    n = 700
    x = _box_points(rng, n)
    q = _values(rng, n, cols, complex_x)
    batch = _ragged_batch(rng, n) if ragged else None
    if batch is not None:
        assert (batch[:100] == 0).all()  # the edge cases share a point set
    z, f = tn.ops.nfft_ewald_near(_cuda(x), _cuda(q), _cuda(batch), alpha, r_c, field)
    tn.ops.check_status()
    dtype = torch.complex64 if complex_x else torch.float32
    assert z.shape == q.shape and z.dtype == dtype
    ref = er.near_sum(q, x, batch, alpha, r_c)
    err = rel_l2(z.cpu().numpy(), ref)
    print("ewald near (%g, %g) ragged=%d cols=%s complex=%d: value rel_l2 %.3e (|ref| %.3e)"
          % (alpha, r_c, ragged, cols, complex_x, err, np.linalg.norm(ref)))
    assert np.linalg.norm(ref) > 0
    assert err <= NEAR_TOL["value"]
    if field:
        assert f.shape == (n, 3) + cols and f.dtype == dtype
        fref = er.near_field(q, x, batch, alpha, r_c)
        ferr = rel_l2(f.cpu().numpy(), fref)
        print("ewald near (%g, %g) ragged=%d cols=%s complex=%d: field rel_l2 %.3e (|ref| %.3e)"
              % (alpha, r_c, ragged, cols, complex_x, ferr, np.linalg.norm(fref)))
        assert ferr <= NEAR_TOL["field"]
    else:
        assert f.numel() == 0


@pytest.fixture(scope="module")
def crowded():
    """3000 points in a cube of edge 0.06 centred on the box corner (1/2, 1/2, 1/2): after wrapping they fill the eight
    corner cells of the 3^3 grid (~375 each: three items and two LDS tiles per cell), every pair is closer than r_c and
    most of them through a wrap"""
    rng = np.random.default_rng(7)
    x = (0.5 + (rng.random((3000, 3)) - 0.5) * 0.06).astype(np.float32)
    q = rng.standard_normal(3000).astype(np.float32)
    return x, q


def test_crowded_corner(crowded):
    import torch_nfft_amd as tn
    x, q = crowded
    assert (x > 0.5).any(0).all() and (x < 0.5).any(0).all()
    z, f = tn.ops.nfft_ewald_near(_cuda(x), _cuda(q), None, 12.0, 0.3, True)
    tn.ops.check_status()
    ref, fref = er.near_sum(q, x, None, 12.0, 0.3), er.near_field(q, x, None, 12.0, 0.3)
    err, ferr = rel_l2(z.cpu().numpy(), ref), rel_l2(f.cpu().numpy(), fref)
    print("ewald near, crowded corner: value rel_l2 %.3e, field rel_l2 %.3e" % (err, ferr))
    assert err <= NEAR_TOL["value"] and ferr <= NEAR_TOL["field"]


def test_two_calls_are_bitwise_equal(crowded):
    import torch_nfft_amd as tn
    x, q = crowded
    xd, qd = _cuda(x), _cuda(np.stack([q, -q[::-1], q * q], 1))
    z1, f1 = tn.ops.nfft_ewald_near(xd, qd, None, 12.0, 0.3, True)
    z2, f2 = tn.ops.nfft_ewald_near(xd, qd, None, 12.0, 0.3, True)
    assert torch.equal(z1, z2) and torch.equal(f1, f2)
    z3, _ = tn.ops.nfft_ewald_near(xd, qd, None, 12.0, 0.3, False)  # the value-only instantiation adds the same pairs
    assert torch.equal(z1, z3)


def test_isolated_charge():
    """a point set of one charge: the pair sum is exactly zero and phi = -2.8373 q wherever the charge sits"""
    import torch_nfft_amd as tn
    rng = np.random.default_rng(11)
    x = (rng.random((61, 3)) - 0.5).astype(np.float32)
    x[0] = (0.31, -0.47, 0.123)
    x[60] = (-0.5, 0.2, 0.4999)
    q = rng.standard_normal(61).astype(np.float32)
    batch = np.concatenate([[0], np.ones(59, dtype=np.int64), [2]]).astype(np.int64)
    z, f = tn.ops.nfft_ewald_near(_cuda(x), _cuda(q), _cuda(batch), 12.0, 0.3, True)
    assert float(z[0]) == 0.0 and float(z[60]) == 0.0 and not bool(f[0].any()) and not bool(f[60].any())
    assert bool(z[1:60].any())
    phi, E = tn.nfft_ewald(_cuda(q), _cuda(x), _cuda(batch), splitting=_splitting(12.0, 0.3), cutoff=4, field=True)
    tn.ops.check_status()
    phi = phi.cpu().numpy()
    for i in (0, 60):
        err = abs(phi[i] / q[i] - er.CUBIC_LATTICE) / abs(er.CUBIC_LATTICE)
        print("isolated charge %d: phi / q = %.7f (%.7f), relative error %.3e" % (i, phi[i] / q[i], er.CUBIC_LATTICE, err))
        assert err <= WHOLE_TOL["value"]
    # The field of a lattice of one charge vanishes by symmetry: what the device returns is the error of the far transform,
    # which adds |q| sum_k |2 pi k_a b_k| in magnitudes on every axis (~ 4 alpha^2 / pi in all) to arrive at zero.
    sp = _splitting(12.0, 0.3)
    scale = float(sp.field_coeffs()[..., 1:].abs().sum((0, 1, 2)).max())
    E = E.cpu().numpy()
    for i in (0, 60):
        print("isolated charge %d: |E| / |q| = %.3e, scale %.3e" % (i, np.abs(E[i]).max() / abs(q[i]), scale))
        assert np.abs(E[i]).max() <= WHOLE_TOL["field"] * abs(q[i]) * scale


def test_nacl_madelung():
    import torch_nfft_amd as tn
    x, q = er.nacl()
    phi = tn.nfft_ewald(_cuda(q.astype(np.float32)), _cuda(x.astype(np.float32)), splitting=_splitting(12.0, 0.3),
                        cutoff=4)
    tn.ops.check_status()
    err = rel_l2(phi.cpu().numpy(), -2.0 * er.MADELUNG_NACL * q)
    print("NaCl: phi / q =", phi.cpu().numpy() / q, "rel_l2 %.3e" % err)
    assert err <= WHOLE_TOL["value"]


@pytest.fixture(scope="module")
def whole():
    """800 charges in two point sets, neither neutral, with the float64 algorithm at (12, 0.3, 32) and the converged sum"""
    rng = np.random.default_rng(3)
    n = 800
    x = (rng.random((n, 3)) - 0.5).astype(np.float32)
    q = rng.standard_normal(n).astype(np.float32)
    batch = (np.arange(n) >= 370).astype(np.int64)
    alg = er.exact_algorithm(q, x, batch, 12.0, 0.3, 32, field=True)
    conv = er.converged(q, x, batch, field=True)
    return x, q, batch, alg, conv


def test_whole_sum_and_field(whole):
    import torch_nfft_amd as tn
    x, q, batch, alg, conv = whole
    sp = _splitting(12.0, 0.3)
    phi, E = tn.nfft_ewald(_cuda(q), _cuda(x), _cuda(batch), splitting=sp, cutoff=4, field=True)
    only = tn.nfft_ewald(_cuda(q), _cuda(x), _cuda(batch), splitting=sp, cutoff=4)
    tn.ops.check_status()
    assert phi.shape == (800,) and E.shape == (800, 3) and phi.dtype == E.dtype == torch.float32
    for what, got, k in (("value", phi, 0), ("value", only, 0), ("field", E, 1)):
        got = got.cpu().numpy()
        e_alg, e_own, e_conv = rel_l2(got, alg[k]), rel_l2(alg[k], conv[k]), rel_l2(got, conv[k])
        print("nfft_ewald %s: rel_l2 vs the float64 algorithm %.3e, vs the converged sum %.3e (the algorithm's own %.3e)"
              % (what, e_alg, e_conv, e_own))
        assert e_alg <= WHOLE_TOL[what]
        assert e_conv <= e_alg + 1.1 * e_own
    U = tn.nfft_ewald_energy(_cuda(q), _cuda(x), _cuda(batch), splitting=sp, cutoff=4).cpu().numpy()
    want = np.array([0.5 * (q[batch == b] * alg[0][batch == b]).sum() for b in (0, 1)])
    assert U.shape == (2,)
    # (a sum of 400 products, each good to WHOLE_TOL of |q| |phi|: Cauchy-Schwarz)
    for b in (0, 1):
        s = batch == b
        assert abs(U[b] - want[b]) <= WHOLE_TOL["value"] * 0.5 * np.linalg.norm(q[s]) * np.linalg.norm(alg[0][s])


@pytest.fixture(scope="module")
def small():
    """300 charges in two point sets, two real columns, a weight for phi, and the float64 algorithm's fields of both"""
    rng = np.random.default_rng(4)
    n = 300
    x = (rng.random((n, 3)) - 0.5).astype(np.float32)
    q = rng.standard_normal((n, 2)).astype(np.float32)
    g = rng.standard_normal((n, 2)).astype(np.float32)
    batch = (np.arange(n) >= 140).astype(np.int64)
    aq = er.exact_algorithm(q, x, batch, 12.0, 0.3, 32, field=True)
    ag = er.exact_algorithm(g, x, batch, 12.0, 0.3, 32, field=True)
    return x, q, g, batch, aq, ag


def test_autograd(small):
    import torch_nfft_amd as tn
    x, q, g, batch, aq, ag = small
    sp = _splitting(12.0, 0.3)
    qd, xd, gd, bd = _cuda(q).requires_grad_(True), _cuda(x).requires_grad_(True), _cuda(g), _cuda(batch)
    phi = tn.nfft_ewald(qd, xd, bd, splitting=sp)
    dq, dx = torch.autograd.grad((phi * gd).sum(), (qd, xd))
    tn.ops.check_status()
    # dq: the operator applied to g -- the device's own (two evaluations, each within WHOLE_TOL) and the float64 one
    own = tn.nfft_ewald(gd, xd.detach(), bd, splitting=sp)
    e_own, e_ref = rel_l2(dq.cpu().numpy(), own.cpu().numpy()), rel_l2(dq.cpu().numpy(), ag[0])
    print("nfft_ewald dq: rel_l2 vs the operator on g %.3e, vs float64 %.3e" % (e_own, e_ref))
    assert e_own <= 2 * WHOLE_TOL["value"] and e_ref <= WHOLE_TOL["value"]
    # dpos_i = -sum_c (g_ic E[q_c]_i + q_ic E[g_c]_i); each field is good to WHOLE_TOL["field"] in l2 and is weighted by at
    # most max |g| or max |q|
    want = -(g[:, None, :] * aq[1] + q[:, None, :] * ag[1]).sum(2)
    bound = WHOLE_TOL["field"] * (np.abs(g).max() * np.linalg.norm(aq[1]) + np.abs(q).max() * np.linalg.norm(ag[1]))
    err = np.linalg.norm(dx.cpu().numpy() - want)
    print("nfft_ewald dpos: |error| %.3e, bound %.3e, rel_l2 %.3e" % (err, bound, rel_l2(dx.cpu().numpy(), want)))
    assert dx.shape == (300, 3) and err <= bound
    # only one of the two asked for
    dq1, = torch.autograd.grad((tn.nfft_ewald(qd, xd.detach(), bd, splitting=sp) * gd).sum(), qd)
    assert rel_l2(dq1.cpu().numpy(), ag[0]) <= WHOLE_TOL["value"]
    dx1, = torch.autograd.grad((tn.nfft_ewald(qd.detach(), xd, bd, splitting=sp) * gd).sum(), xd)
    assert np.linalg.norm(dx1.cpu().numpy() - want) <= bound


def test_forces_of_the_energy(small):
    """-dU/dx_i = sum_c q_ic E_ic"""
    import torch_nfft_amd as tn
    x, q, g, batch, aq, ag = small
    sp = _splitting(12.0, 0.3)
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
    print("forces: |autograd - q E| %.3e, |autograd - float64| %.3e, bound %.3e" % (e_dev, e_ref, bound))
    assert e_ref <= bound and e_dev <= 2 * bound


def test_second_derivative_and_refusals(small):
    import torch_nfft_amd as tn
    x, q, g, batch, _, _ = small
    sp = _splitting(12.0, 0.3)
    qd, xd, bd = _cuda(q).requires_grad_(True), _cuda(x).requires_grad_(True), _cuda(batch)
    phi, E = tn.nfft_ewald(qd, xd, bd, splitting=sp, field=True)
    assert phi.requires_grad and not E.requires_grad
    dq, dx = torch.autograd.grad(phi.square().sum(), (qd, xd), create_graph=True)
    with pytest.raises(RuntimeError, match="differentiate twice|once_differentiable"):
        dx.square().sum().backward()
    with pytest.raises(AssertionError, match="batch"):
        tn.nfft_ewald(qd, xd, torch.zeros(300, device="cuda", requires_grad=True), splitting=sp)
    with pytest.raises(ValueError, match="three-dimensional"):
        tn.nfft_ewald(qd, xd[:, :2], bd, splitting=sp)
    with pytest.raises(RuntimeError, match="Input mismatch"):
        tn.ops.nfft_ewald_near(xd.detach(), qd.detach(), bd, 12.0, 0.34, False)
    with pytest.raises(RuntimeError, match="Input mismatch"):
        tn.ops.nfft_ewald_near(xd.detach()[:, :2].contiguous(), qd.detach(), bd, 12.0, 0.3, False)


def test_empty_input():
    import torch_nfft_amd as tn
    sp = _splitting(12.0, 0.3, 16)
    q = torch.zeros(0, 2, device="cuda", requires_grad=True)
    x = torch.zeros(0, 3, device="cuda", requires_grad=True)
    phi, E = tn.nfft_ewald(q, x, splitting=sp, field=True)
    assert phi.shape == (0, 2) and E.shape == (0, 3, 2)
    dq, dx = torch.autograd.grad(phi.sum(), (q, x))
    assert dq.shape == (0, 2) and dx.shape == (0, 3)
    z, f = tn.ops.nfft_ewald_near(x.detach(), q.detach(), None, 12.0, 0.3, True)
    assert z.shape == (0, 2) and f.shape == (0, 3, 2)
    assert tn.nfft_ewald_energy(q.detach(), x.detach(), splitting=sp).shape == (1, 2)
