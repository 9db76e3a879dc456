"""GPU tests of the screened Coulomb (Yukawa) Ewald sum: the wrapped pair sweep and the pair reduction
of csrc/ewald_yukawa.hip on the unit torus and in a box, and nfft_ewald_yukawa / _energy / _virial with their gradients, against
the float64 restatement tests/yukawa_ref.py on the same float32 positions, and against the brute-force lattice sum.

All cases run on the 512 points of yukawa_ref.near_points(): the 8^3 jittered lattice with the edge cases of the wrap.

Tolerances.  NEAR_TOL, WHOLE_TOL and VIRIAL_TOL are 4x the largest rel_l2 of the first device run against the float64
reference (the figure behind each entry is in its comment), the project's convention (tests/test_gpu_ewald.py); a first-run
figure above 1e-4 would have been a defect, not a tolerance.  tests/test_yukawa_ref.py shows that every mistake of the pair
weight or of the sweep moves the sums at lambda = 10, (6, 0.25) by 1e-2 at least.  Against the lattice sum the bound is the
triangle inequality with the algorithm's own truncation error, no free number.
"""
import functools

import numpy as np
import pytest
import torch

import yukawa_ref as yr
from conftest import rel_l2
from ewald_box_ref import O, T

pytestmark = pytest.mark.gpu

NEAR_TOL = {  # 4 x the largest rel_l2 of the first device run (in brackets)
    "value": 3.6e-6,  # (9.029e-7: cube at (12, 0.12), lambda = 40, one set; 2.2e-7 .. 8.5e-7 on the fourteen other cases)
    "field": 4.0e-6,  # (1.007e-6: cube at (6, 0.25), lambda = 40, three columns; 2.7e-7 .. 8.1e-7 on the others)
}
# (charges of mixed sign: single points whose sum nearly cancels stand up to 9.8e-4 from their own value, the l2 norms do not
# see them; at lambda = 0 the sweep stood 6.9e-8 (value) and 3.7e-8 (field) from the Coulomb sweep)
WHOLE_TOL = {  # the same for nfft_ewald_yukawa ((14, 0.25, 32), cutoff = 4) against the float64 algorithm
    "value": 4.5e-6,  # (1.113e-6: dL/dq in T, Cartesian input, lambda = 10; 1.111e-6 for complex q in O; the values themselves
                      # 4.8e-7 .. 1.02e-6)
    "field": 2.0e-6,  # (5.106e-7 in O, lambda = 10; 4.6e-7 .. 5.1e-7 on the others)
}
VIRIAL_TOL = {  # the same for nfft_ewald_yukawa_virial
    "U": 4.2e-5,  # (1.042e-5: cube, lambda = 10, three columns, ragged, background; 4.4e-7 .. 8.2e-6 on the others -- charges of
                  # mixed sign: U is what is left of pair terms of both signs)
    "W": 3.6e-6,  # (9.052e-7 in O, lambda = 10, three columns; 2.7e-7 .. 8.8e-7 on the others)
}

BOXES = {"cube": None, "T": T, "O": O}
RAGGED = np.concatenate([np.zeros(230, np.int64), np.full(282, 2, np.int64)])  # three point sets, the middle one empty
WHOLE = (14.0, 0.25, 32)  # alpha, r_c, N: erfc(alpha r_c) = 7e-7, e^(-pi^2 16^2 / alpha^2) = 3e-6 on the plane k_a = 16


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _box6(A):
    return () if A is None else (A[0, 0], A[1, 0], A[1, 1], A[2, 0], A[2, 1], A[2, 2])


def _charges(rng, n, cols, complex_x=False):
    """charges of mixed sign"""
    x = rng.standard_normal((n,) + cols)
    if complex_x:
        return (x + 1j * rng.standard_normal((n,) + cols)).astype(np.complex64)
    return x.astype(np.float32)


def _max_pointwise(got, ref):
    """the largest relative error of one point (all its columns and components together)"""
    d = np.abs(got - ref).reshape(ref.shape[0], -1).max(1)
    scale = np.abs(ref).reshape(ref.shape[0], -1).max(1)
    return float((d[scale > 0] / scale[scale > 0]).max())


@functools.lru_cache(maxsize=None)
def _points():
    return yr.near_points()  # (shared and left unchanged)


# box, alpha, r_c (cube: G = 3, 4, 8), lambda, ragged, cols, complex, field
CASES = [
    ("cube", 5.0, 0.3, 2.0, False, (), False, True),
    ("cube", 5.0, 0.3, 10.0, True, (3,), False, False),
    ("cube", 5.0, 0.3, 40.0, False, (2,), True, True),
    ("cube", 6.0, 0.25, 10.0, True, (), False, True),
    ("cube", 6.0, 0.25, 40.0, False, (3,), False, True),
    ("cube", 6.0, 0.25, 2.0, True, (2,), True, False),
    ("cube", 12.0, 0.12, 40.0, False, (), False, False),
    ("cube", 12.0, 0.12, 2.0, True, (3,), False, True),
    ("cube", 12.0, 0.12, 10.0, True, (2,), True, True),
    ("T", 5.0, 0.3, 10.0, True, (), False, True),
    ("T", 6.0, 0.25, 2.0, False, (3,), False, True),
    ("T", 12.0, 0.12, 40.0, True, (2,), True, True),
    ("O", 6.0, 0.25, 40.0, True, (), False, False),
    ("O", 6.0, 0.25, 10.0, False, (2,), True, True),
    ("O", 12.0, 0.12, 2.0, True, (3,), False, True),
]


def _sweep(box, x, q, batch, alpha, r_c, lam, field):
    import torch_nfft_amd as tn
    out = tn.ops.nfft_ewald_yukawa_near(_cuda(x), _cuda(q), _cuda(batch), _box6(BOXES[box]), alpha, r_c, lam, field)
    tn.ops.check_status()
    return out


@pytest.mark.parametrize("box,alpha,r_c,lam,ragged,cols,complex_x,field", CASES)
def test_near_sweep_against_brute_force(box, alpha, r_c, lam, ragged, cols, complex_x, field):
    x = _points()
    n = x.shape[0]
    A = BOXES[box]
    rng = np.random.default_rng(int(alpha) * 100 + len(cols) + 10 * ragged + int(lam))
    q = _charges(rng, n, cols, complex_x)
    batch = RAGGED if ragged else None
    z, f = _sweep(box, x, q, batch, alpha, r_c, lam, field)
    dtype = torch.complex64 if complex_x else torch.float32
    assert z.shape == q.shape and z.dtype == dtype
    ref = yr.near_sum(q, x, A, batch, alpha, lam, r_c)
    err = rel_l2(z.cpu().numpy(), ref)
    print("yukawa near %s (%g, %g) lambda=%g ragged=%d cols=%s complex=%d: value rel_l2 %.3e, worst point %.3e (|ref| %.3e)"
          % (box, alpha, r_c, lam, ragged, cols, complex_x, err, _max_pointwise(z.cpu().numpy(), ref), np.linalg.norm(ref)))
    assert np.linalg.norm(ref) > 0
    assert err <= NEAR_TOL["value"]
    if field:
        assert f.shape == (n, 3) + cols and f.dtype == dtype
        fref = yr.near_field(q, x, A, batch, alpha, lam, r_c)
        ferr = rel_l2(f.cpu().numpy(), fref)
        print("yukawa near %s (%g, %g) lambda=%g ragged=%d cols=%s complex=%d: field rel_l2 %.3e, worst point %.3e (|ref| %.3e)"
              % (box, alpha, r_c, lam, ragged, cols, complex_x, ferr, _max_pointwise(f.cpu().numpy(), fref), np.linalg.norm(fref)))
        assert ferr <= NEAR_TOL["field"]
    else:
        assert f.numel() == 0


@pytest.mark.parametrize("box", ["cube", "T"])
def test_zero_screening_is_the_coulomb_sweep(box):
    """screening = 0 is legal for the operator and gives the Coulomb weights: the Coulomb sweep of the same pairs on the same
    inputs, within the near tolerance (the first device run stood 6.9e-8 in the value and 3.7e-8 in the field from it)"""
    import torch_nfft_amd as tn
    x = _points()
    q = _charges(np.random.default_rng(21), 512, (2,))
    z, f = _sweep(box, x, q, RAGGED, 6.0, 0.25, 0.0, True)
    if BOXES[box] is None:
        zc, fc = tn.ops.nfft_ewald_near(_cuda(x), _cuda(q), _cuda(RAGGED), 6.0, 0.25, True)
    else:
        zc, fc = tn.ops.nfft_ewald_near_box(_cuda(x), _cuda(q), _cuda(RAGGED), _box6(BOXES[box]), 6.0, 0.25, True)
    tn.ops.check_status()
    ev, ef = rel_l2(z.cpu().numpy(), zc.cpu().numpy()), rel_l2(f.cpu().numpy(), fc.cpu().numpy())
    print("yukawa near at lambda = 0 against the Coulomb sweep in %s: value rel_l2 %.3e, field rel_l2 %.3e" % (box, ev, ef))
    assert ev <= NEAR_TOL["value"] and ef <= NEAR_TOL["field"]


def test_two_calls_give_the_same_bits():
    import torch_nfft_amd as tn
    x = _points()
    q = _charges(np.random.default_rng(22), 512, (3,))
    z, f = _sweep("T", x, q, RAGGED, 6.0, 0.25, 10.0, True)
    z2, f2 = _sweep("T", x, q, RAGGED, 6.0, 0.25, 10.0, True)
    z3, _ = _sweep("T", x, q, RAGGED, 6.0, 0.25, 10.0, False)  # (the value-only instantiation adds the same pairs)
    assert torch.equal(z, z2) and torch.equal(f, f2) and torch.equal(z, z3)
    seven = [tn.ops.nfft_ewald_yukawa_virial_near(_cuda(x), _cuda(q), _cuda(RAGGED), _box6(T), 6.0, 0.25, 10.0) for _ in range(2)]
    tn.ops.check_status()
    assert seven[0].shape == (3, 7, 3) and seven[0].dtype == torch.float64 and torch.equal(seven[0], seven[1])
    assert not seven[0][1].any()  # (the empty set)


def _splitting(box, lam, background, params=WHOLE):
    import torch_nfft_amd as tn
    A = BOXES[box]
    return tn.YukawaSplitting(params[0], params[1], params[2], lam, box=None if A is None else torch.from_numpy(A),
                              background=background)


@functools.lru_cache(maxsize=None)
def _whole_inputs():
    rng = np.random.default_rng(3)
    return _charges(rng, 512, ()) + np.float32(0.1), _charges(rng, 512, ())  # (q is not neutral), g


def _positions(box, fractional):
    """(what is passed, the fractional float32 positions that it stands for)"""
    s, A = _points(), BOXES[box]
    if A is None or fractional:
        return s, s
    pos = (s.astype(np.float64) @ A).astype(np.float32)
    return pos, (pos.astype(np.float64) @ np.linalg.inv(A)).astype(np.float32)


# box, fractional, lambda, background, the split (None: WHOLE; a number: from_tolerance(1e-5, 0.25, that))
WHOLE_CASES = [
    ("cube", False, 2.0, False, None),
    ("cube", False, 10.0, True, None),
    ("T", True, 2.0, True, None),
    ("T", False, 10.0, False, None),
    ("O", True, 10.0, False, None),
    ("O", False, 2.0, True, None),
    ("T", True, 5.0, False, 5.0),
]


@pytest.mark.parametrize("box,fractional,lam,background,from_tol", WHOLE_CASES)
def test_whole_sum_field_and_gradients(box, fractional, lam, background, from_tol):
    import torch_nfft_amd as tn
    A = BOXES[box]
    q, g = _whole_inputs()
    pos, sf = _positions(box, fractional)
    if from_tol is None:
        sp = _splitting(box, lam, background)
    else:
        sp = tn.YukawaSplitting.from_tolerance(1e-5, 0.25, from_tol, box=torch.from_numpy(A), background=background)
        assert sp.bandwidth % 2 == 0 and sp.screening == from_tol
    phi_ref, E_ref = yr.yukawa(np.stack([q, g], 1), sf, A, RAGGED, sp.alpha, lam, sp.r_cut, sp.bandwidth, background=background)
    kw = dict(splitting=sp, cutoff=4, fractional=fractional)
    qd, xd, gd, bd = _cuda(q).requires_grad_(True), _cuda(pos).requires_grad_(True), _cuda(g), _cuda(RAGGED)
    phi, E = tn.nfft_ewald_yukawa(qd, xd, bd, field=True, **kw)
    only = tn.nfft_ewald_yukawa(qd.detach(), xd.detach(), bd, **kw)
    tn.ops.check_status()
    assert phi.shape == (512,) and E.shape == (512, 3) and phi.dtype == E.dtype == torch.float32 and not E.requires_grad
    tag = "nfft_ewald_yukawa in %s (fractional=%d, lambda=%g, background=%d, N=%d)" % (box, fractional, lam, background, sp.bandwidth)
    for what, got, want in (("value", phi, phi_ref[:, 0]), ("value", only, phi_ref[:, 0]), ("field", E, E_ref[:, :, 0])):
        got = got.detach().cpu().numpy()
        err = rel_l2(got, want)
        print("%s %s: rel_l2 vs the float64 algorithm %.3e, worst point %.3e" % (tag, what, err, _max_pointwise(got, want)))
        assert err <= WHOLE_TOL[what]
    # L = sum g phi: dL/dq is the operator applied to g
    dq, dx = torch.autograd.grad((phi * gd).sum(), (qd, xd))
    tn.ops.check_status()
    err = rel_l2(dq.cpu().numpy(), phi_ref[:, 1])
    print("%s dL/dq: rel_l2 vs the float64 algorithm %.3e" % (tag, err))
    assert err <= WHOLE_TOL["value"]
    # dL/dpos_i = -(g_i E[q]_i + q_i E[g]_i) (Cartesian), times A^T for fractional input; each field is good to
    # WHOLE_TOL["field"] in l2 and is weighted by at most max |g| or max |q|
    want = -(g[:, None] * E_ref[:, :, 0] + q[:, None] * E_ref[:, :, 1])
    bound = WHOLE_TOL["field"] * (np.abs(g).max() * np.linalg.norm(E_ref[:, :, 0]) + np.abs(q).max() * np.linalg.norm(E_ref[:, :, 1]))
    if fractional:
        want = want @ A.T
        bound *= np.linalg.norm(A, 2)
    err = np.linalg.norm(dx.cpu().numpy() - want)
    print("%s dL/dpos: |error| %.3e, bound %.3e, rel_l2 %.3e" % (tag, err, bound, rel_l2(dx.cpu().numpy(), want)))
    assert dx.shape == pos.shape and err <= bound
    # the energy: dU/dpos_i = -q_i E[q]_i
    xe = _cuda(pos).requires_grad_(True)
    U = tn.nfft_ewald_yukawa_energy(_cuda(q), xe, bd, **kw)
    de, = torch.autograd.grad(U.sum(), xe)
    tn.ops.check_status()
    U = U.detach()
    assert U.shape == (3,) and float(U[1]) == 0.0
    want = -(q[:, None] * E_ref[:, :, 0])
    bound = WHOLE_TOL["field"] * np.abs(q).max() * np.linalg.norm(E_ref[:, :, 0])
    if fractional:
        want = want @ A.T
        bound *= np.linalg.norm(A, 2)
    err = np.linalg.norm(de.cpu().numpy() - want)
    print("%s energy dU/dpos: |error| %.3e, bound %.3e" % (tag, err, bound))
    assert err <= bound
    for b in (0, 2):  # (a sum of products, each good to WHOLE_TOL of |q| |phi|: Cauchy-Schwarz)
        sel = RAGGED == b
        want = 0.5 * (q[sel].astype(np.float64) * phi_ref[sel, 0]).sum()
        assert abs(float(U[b]) - want) <= WHOLE_TOL["value"] * 0.5 * np.linalg.norm(q[sel]) * np.linalg.norm(phi_ref[sel, 0])


def test_complex_charges_and_columns():
    """complex q in two columns through the whole sum: the real and the imaginary part are two real problems"""
    import torch_nfft_amd as tn
    rng = np.random.default_rng(8)
    q = _charges(rng, 512, (2,), True)
    sp = _splitting("O", 10.0, True)
    phi, E = tn.nfft_ewald_yukawa(_cuda(q), _cuda(_points()), _cuda(RAGGED), splitting=sp, field=True, fractional=True)
    tn.ops.check_status()
    assert phi.shape == (512, 2) and E.shape == (512, 3, 2) and phi.dtype == E.dtype == torch.complex64
    ref, eref = yr.yukawa(q, _points(), O, RAGGED, WHOLE[0], 10.0, WHOLE[1], WHOLE[2], background=True)
    ev, ef = rel_l2(phi.cpu().numpy(), ref), rel_l2(E.cpu().numpy(), eref)
    print("nfft_ewald_yukawa in O, complex q, two columns: value rel_l2 %.3e, field rel_l2 %.3e" % (ev, ef))
    assert ev <= WHOLE_TOL["value"] and ef <= WHOLE_TOL["field"]


@pytest.mark.parametrize("box", ["cube", "T"])
def test_converged_sum(box):
    """216 points against the brute-force lattice sum (lambda = 8, images |n|_inf <= 6: e^(-8 * 0.9 * 6) = 2e-19 is left out):
    |device - lattice| <= |device - algorithm| + |algorithm - lattice|, the first within WHOLE_TOL of |algorithm| <=
    (1 + e_own) |lattice|, the second e_own |lattice| computed here in float64"""
    import torch_nfft_amd as tn
    import dispersion_ref as dr
    A = BOXES[box]
    rng = np.random.default_rng(9)
    s = dr.jittered_lattice(rng, 6, 1.0 / 6, 0.03).reshape(-1, 3)
    q = _charges(rng, 216, ())
    lam = 8.0
    alpha, r_c, N = WHOLE
    lat = yr.lattice_sum(q, s, A, lam, 6, reach=4.6)  # (the images skipped carry e^(-8 * 4.6) / 4.6 = 2e-17 per pair)
    alg = yr.yukawa(q, s, A, None, alpha, lam, r_c, N)
    sp = _splitting(box, lam, False)
    frac = dict(fractional=True) if A is not None else {}
    got = tn.nfft_ewald_yukawa(_cuda(q), _cuda(s), splitting=sp, cutoff=4, field=True, **frac)
    tn.ops.check_status()
    for what, k in (("value", 0), ("field", 1)):
        e_own, e_conv = rel_l2(alg[k], lat[k]), rel_l2(got[k].cpu().numpy(), lat[k])
        print("nfft_ewald_yukawa %s in %s: rel_l2 vs the lattice sum %.3e (the algorithm's own %.3e, vs the algorithm %.3e)"
              % (what, box, e_conv, e_own, rel_l2(got[k].cpu().numpy(), alg[k])))
        assert e_conv <= WHOLE_TOL[what] * (1 + e_own) + e_own


# box, lambda, cols, ragged, background
VIRIAL_CASES = [
    ("cube", 2.0, (), False, False),
    ("cube", 10.0, (3,), True, True),
    ("T", 10.0, (), True, False),
    ("T", 2.0, (3,), False, True),
    ("O", 2.0, (), False, True),
    ("O", 10.0, (3,), True, False),
]


@pytest.mark.parametrize("box,lam,cols,ragged,background", VIRIAL_CASES)
def test_virial(box, lam, cols, ragged, background):
    import torch_nfft_amd as tn
    A = BOXES[box]
    s = _points()
    q = _charges(np.random.default_rng(31 + len(cols)), 512, cols) + np.float32(0.1)
    batch = RAGGED if ragged else None
    alpha, r_c, N = WHOLE
    sp = _splitting(box, lam, background)
    frac = dict(fractional=True) if A is not None else {}
    U, W = tn.nfft_ewald_yukawa_virial(_cuda(q), _cuda(s), _cuda(batch), splitting=sp, cutoff=4, **frac)
    tn.ops.check_status()
    B = 3 if ragged else 1
    assert U.shape == (B,) + cols and W.shape == (B, 3, 3) + cols and U.dtype == W.dtype == torch.float32
    assert not U.requires_grad and torch.equal(W, W.transpose(1, 2))
    Uref, Wref = yr.virial(q, s, A, batch, alpha, lam, r_c, N, background=background)
    eu, ew = rel_l2(U.cpu().numpy(), Uref), rel_l2(W.cpu().numpy(), Wref)
    print("nfft_ewald_yukawa_virial in %s lambda=%g cols=%s ragged=%d background=%d: U rel_l2 %.3e, W rel_l2 %.3e"
          % (box, lam, cols, ragged, background, eu, ew))
    assert eu <= VIRIAL_TOL["U"] and ew <= VIRIAL_TOL["W"]
    # U is the energy of nfft_ewald_yukawa_energy: each within its tolerance of the float64 value
    Ue = tn.nfft_ewald_yukawa_energy(_cuda(q), _cuda(s), _cuda(batch), splitting=sp, cutoff=4, **frac)
    tn.ops.check_status()
    phi_ref = yr.yukawa(q, s, A, batch, alpha, lam, r_c, N, background=background)[0]
    for b in range(B):
        sel = slice(None) if batch is None else batch == b
        scale = 0.5 * np.linalg.norm(q[sel], axis=0) * np.linalg.norm(phi_ref[sel], axis=0)
        gap = np.abs(U[b].cpu().numpy().astype(np.float64) - Ue[b].cpu().numpy())
        assert (gap <= WHOLE_TOL["value"] * scale + VIRIAL_TOL["U"] * np.abs(Uref[b])).all()
    # the box gradient goes through unchanged
    g = tn.virial_to_box_gradient(W, sp.box).cpu().numpy().reshape(B, 3, 3, -1)
    inv = np.eye(3) if A is None else np.linalg.inv(A)
    want = np.tril(np.ones((3, 3)))[None, :, :, None] * -np.einsum("ki,bkjc->bijc", inv, W.cpu().numpy().reshape(B, 3, 3, -1))
    assert np.abs(g - want).max() <= 1e-5 * np.abs(want).max()


def test_refusals_on_the_device():
    import torch_nfft_amd as tn
    q, _ = _whole_inputs()
    sp = _splitting("cube", 2.0, False)
    qd, xd, bd = _cuda(q).requires_grad_(True), _cuda(_points()).requires_grad_(True), _cuda(RAGGED)
    phi, E = tn.nfft_ewald_yukawa(qd, xd, bd, splitting=sp, field=True)
    assert phi.requires_grad and not E.requires_grad
    dq, dx = torch.autograd.grad(phi.square().sum(), (qd, xd), create_graph=True)
    with pytest.raises(RuntimeError, match="differentiate twice|once_differentiable"):
        dx.square().sum().backward()
    for fn in (tn.nfft_ewald_yukawa, tn.nfft_ewald_yukawa_energy, tn.nfft_ewald_yukawa_virial):
        with pytest.raises(AssertionError, match="batch"):
            fn(qd, xd, torch.zeros(512, device="cuda", requires_grad=True), splitting=sp)
    with pytest.raises(ValueError, match="real"):
        tn.nfft_ewald_yukawa_virial(_cuda(q).to(torch.complex64), xd, bd, splitting=sp)
    with pytest.raises(TypeError, match="YukawaSplitting"):
        tn.nfft_ewald_yukawa(qd, xd, bd, splitting=tn.EwaldSplitting(14.0, 0.25, 32))
    for lam in (-1.0, float("nan"), 50.0001 / 0.25):
        with pytest.raises(RuntimeError, match="Input mismatch.*screening"):
            tn.ops.nfft_ewald_yukawa_near(xd.detach(), qd.detach(), bd, (), 6.0, 0.25, lam, False)
        with pytest.raises(RuntimeError, match="Input mismatch.*screening"):
            tn.ops.nfft_ewald_yukawa_virial_near(xd.detach(), qd.detach(), bd, _box6(T), 6.0, 0.25, lam)
    with pytest.raises(RuntimeError, match="Input mismatch"):
        tn.ops.nfft_ewald_yukawa_near(xd.detach(), qd.detach(), bd, (), 5.0, 0.34, 2.0, False)
    tn.ops.check_status()
    # empty input
    q0 = torch.zeros(0, 2, device="cuda", requires_grad=True)
    x0 = torch.zeros(0, 3, device="cuda", requires_grad=True)
    phi, E = tn.nfft_ewald_yukawa(q0, x0, splitting=sp, field=True)
    assert phi.shape == (0, 2) and E.shape == (0, 3, 2)
    dq, dx0 = torch.autograd.grad(phi.sum(), (q0, x0))
    assert dq.shape == (0, 2) and dx0.shape == (0, 3)
    tn.ops.check_status()
