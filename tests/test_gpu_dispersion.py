"""GPU tests of the dispersion Ewald sum, the periodic 1/r^6: the wrapped pair sweep
csrc/ewald_disp.hip on the unit torus and in a box, and nfft_ewald_dispersion / nfft_ewald_dispersion_energy with their
gradients, against the float64 restatement tests/dispersion_ref.py on the same float32 positions.

Tolerances.  The device evaluates e^(-a^2) (1 + a^2 + a^4/2) / r^6 and its slope in float32.  NEAR_TOL and WHOLE_TOL are 4x the
largest rel_l2 of the first device run (the figure behind each entry is in its comment), the project's convention
(tests/test_gpu_ewald.py); a first-run figure above 1e-4 would have been a defect, not a tolerance.  The near tests run at
alpha r_c ~ 1.5, where tests/test_dispersion_ref.py shows that a missing wrap, a cut at 0.95 r_c or a dropped polynomial term
each move the sums by 5e-4 at least.  1/r^6 lets a few close pairs dominate an l2 norm, so every case also prints its
largest per-point relative error (not gated; recorded in section 7j).  Against the converged lattice sum the bound is the
triangle inequality with the algorithm's own truncation error, no free number.
"""
import numpy as np
import pytest
import torch

import dispersion_ref as dr
from conftest import rel_l2
from ewald_box_ref import O, T

pytestmark = pytest.mark.gpu

NEAR_TOL = {  # 4 x the largest rel_l2 of the first device run (in brackets)
    "value": 6.6e-6,  # (1.649e-6: cube at (5, 0.3), one set; 2.2e-7 .. 1.4e-6 on the fourteen other cases)
    "field": 7.4e-6,  # (1.857e-6: the same case; 1.3e-7 .. 1.5e-6 on the others)
    "crowded_value": 2.6e-5,  # (6.415e-6; 6.34e-6 and 6.36e-6 with two and five columns)
    "crowded_field": 2.0e-5,  # (5.101e-6; 5.09e-6 and 5.06e-6)
}
# What these figures are made of: the difference of two float32 positions on either side of a face is rounded at |d| ~ 1
# (3e-8 absolute) and then stands for a distance r, a relative error of 3e-8 / r that 1/r^6 multiplies by six (by eight in
# the field).  The pairs 0.04 apart through a face carry 4.5e-6 each (the worst point of every case above is 3.7e-6 ..
# 3.9e-6 in the value, 4.4e-6 .. 7.0e-6 in the field), the crowded corner's wrapped neighbours at 0.01 .. 0.02 carry 1e-5.
WHOLE_TOL = {  # the same for nfft_ewald_dispersion ((14, 0.25, 32), cutoff = 4) against the float64 algorithm
    "value": 9.4e-6,  # (2.360e-6: dc of the backward in T; the whole sums 1.320e-6 in the cube, 1.586e-6 in T, 1.301e-6 in O)
    "field": 3.0e-6,  # (7.476e-7 in O; 4.94e-7 in the cube, 4.67e-7 in T)
}
# (the self term alpha^6 / 6 = 1.25e6 per unit of c stands against a far sum of the same size: psi is what is left of them,
# here about half, and its relative error doubles the transform's)

BOXES = {"cube": None, "T": T, "O": O}


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _box6(A):
    return (A[0, 0], A[1, 0], A[1, 1], A[2, 0], A[2, 1], A[2, 2])


def _values(rng, n, cols, complex_x):
    """coefficients in [0.5, 1.5): dispersion coefficients are positive, and a sum without cancellation is the stricter
    yardstick for a relative error"""
    x = rng.random((n,) + cols) + 0.5
    if complex_x:
        return (x + 1j * (rng.random((n,) + cols) + 0.5)).astype(np.complex64)
    return x.astype(np.float32)


def _max_pointwise(got, ref):
    """the largest relative error of one point (all its columns and components together)"""
    d = np.abs(got - ref).reshape(ref.shape[0], -1).max(1)
    scale = np.abs(ref).reshape(ref.shape[0], -1).max(1)
    assert (d[scale == 0] == 0).all()  # (a point without a neighbour inside r_c: exactly zero on both sides)
    return float((d[scale > 0] / scale[scale > 0]).max())


def _near_points():
    """The 8^3 jittered lattice (spacing 1/8, jitter 0.03; the points of the sensitivity test of tests/test_dispersion_ref.py)
    with the edge cases of the wrap written over 29 of its nodes, those first: float32 [512, 3]"""
    rng = np.random.default_rng(0)
    x = dr.jittered_lattice(rng, 8, 1.0 / 8, 0.03)
    below = np.nextafter(np.float32(0.5), np.float32(0))  # the largest float32 below 1/2
    special = []

    def node(i, j, k):
        special.append((i, j, k))
        return (i, j, k)

    for a, idx in enumerate(((0, 2, 3), (3, 0, 2), (2, 3, 0))):      # exactly on the lower faces
        x[node(*idx)][a] = -0.5
    for a, idx in enumerate(((7, 5, 4), (4, 7, 5), (5, 4, 7))):      # just below the upper faces
        x[node(*idx)][a] = below
    x[node(7, 7, 7)][:] = below                                      # ... and in the upper corner
    for idx in ((1, 1, 1), (6, 1, 2), (2, 6, 1), (1, 2, 6)):         # given outside the box: must act as their images
        x[node(*idx)] += np.float32(0.7)
    for idx in ((5, 5, 1), (1, 5, 5), (5, 1, 5), (6, 6, 2)):
        x[node(*idx)] -= np.float32(1.2)
    for dst, src in (((3, 3, 3), (3, 3, 4)), ((4, 4, 4), (4, 4, 3)), ((3, 4, 3), (3, 4, 4)), ((4, 3, 4), (4, 3, 3))):
        x[node(*dst)] = x[node(*src)]                                # exact duplicates: r = 0
    for a, (p, q) in enumerate((((0, 6, 5), (7, 6, 5)), ((6, 0, 6), (6, 7, 6)), ((2, 5, 0), (2, 5, 7)))):
        x[node(*q)] = x[node(*p)] + np.float32(0.01)                 # a pair 0.04 apart through each face
        x[p][a], x[q][a] = -0.48, 0.48
    flat = [(i * 8 + j) * 8 + k for i, j, k in special]
    rest = np.setdiff1d(np.arange(512), flat)
    return x.reshape(-1, 3)[np.concatenate([flat, rng.permutation(rest)])]


RAGGED = np.concatenate([np.zeros(230, np.int64), np.full(282, 2, np.int64)])  # three point sets, the middle one empty

# box, alpha, r_c (cube: G = 3, 4, 8), ragged, cols, complex, field
CASES = [
    ("cube", 5.0, 0.3, False, (), False, True),
    ("cube", 5.0, 0.3, True, (3,), False, False),
    ("cube", 5.0, 0.3, False, (2,), True, True),
    ("cube", 6.0, 0.25, True, (), False, True),
    ("cube", 6.0, 0.25, False, (3,), False, True),
    ("cube", 6.0, 0.25, True, (2,), True, False),
    ("cube", 12.0, 0.12, False, (), False, False),
    ("cube", 12.0, 0.12, True, (3,), False, True),
    ("cube", 12.0, 0.12, True, (2,), True, True),
    ("T", 5.0, 0.3, True, (), False, True),
    ("T", 6.0, 0.25, False, (3,), False, True),
    ("T", 12.0, 0.12, True, (2,), True, True),
    ("O", 6.0, 0.25, True, (), False, False),
    ("O", 6.0, 0.25, False, (2,), True, True),
    ("O", 12.0, 0.12, True, (3,), False, True),
]


def _sweep(box, x, c, batch, alpha, r_c, field):
    import torch_nfft_amd as tn
    if BOXES[box] is None:
        out = tn.ops.nfft_ewald_dispersion_near(_cuda(x), _cuda(c), _cuda(batch), alpha, r_c, field)
    else:
        out = tn.ops.nfft_ewald_dispersion_near_box(_cuda(x), _cuda(c), _cuda(batch), _box6(BOXES[box]), alpha, r_c, field)
    tn.ops.check_status()
    return out


@pytest.mark.parametrize("box,alpha,r_c,ragged,cols,complex_x,field", CASES)
def test_near_sweep_against_brute_force(box, alpha, r_c, ragged, cols, complex_x, field):
    x = _near_points()
    n = x.shape[0]
    A = BOXES[box]
    assert dr.min_separation(x, A) >= 0.03 * (1.0 if A is None else 0.8)  # (no pair close enough to drown the others)
    rng = np.random.default_rng(int(alpha) * 100 + len(cols) + 10 * ragged)
    c = _values(rng, n, cols, complex_x)
    batch = RAGGED if ragged else None
    z, f = _sweep(box, x, c, batch, alpha, r_c, field)
    dtype = torch.complex64 if complex_x else torch.float32
    assert z.shape == c.shape and z.dtype == dtype
    ref = dr.near_sum(c, x, A, batch, alpha, r_c)
    err = rel_l2(z.cpu().numpy(), ref)
    print("dispersion near %s (%g, %g) ragged=%d cols=%s complex=%d: value rel_l2 %.3e, worst point %.3e (|ref| %.3e)"
          % (box, alpha, r_c, ragged, cols, complex_x, err, _max_pointwise(z.cpu().numpy(), ref), np.linalg.norm(ref)))
    assert np.linalg.norm(ref) > 0
    assert err <= NEAR_TOL["value"]
    if field:
        assert f.shape == (n, 3) + cols and f.dtype == dtype
        fref = dr.near_field(c, x, A, batch, alpha, r_c)
        ferr = rel_l2(f.cpu().numpy(), fref)
        print("dispersion near %s (%g, %g) ragged=%d cols=%s complex=%d: field rel_l2 %.3e, worst point %.3e (|ref| %.3e)"
              % (box, alpha, r_c, ragged, cols, complex_x, ferr, _max_pointwise(f.cpu().numpy(), fref), np.linalg.norm(fref)))
        assert ferr <= NEAR_TOL["field"]
    else:
        assert f.numel() == 0


@pytest.fixture(scope="module")
def crowded():
    """14^3 points on a jittered lattice of spacing 0.017 (jitter 20 %: no two closer than 0.01) in a cube of edge 0.24 centred
    on the box corner (1/2, 1/2, 1/2): after wrapping ~343 in each of the eight corner cells of the 3^3 grid -- several LDS
    tiles and work items per cell -- and most pairs through a wrap.  Five columns and their float64 sums at (5, 0.3)."""
    rng = np.random.default_rng(7)
    x = dr.jittered_lattice(rng, 14, 0.017, 0.2 * 0.017, centre=0.5).reshape(-1, 3)
    c = _values(rng, x.shape[0], (5,), False)
    return x, c, dr.near_sum(c, x, None, None, 5.0, 0.3), dr.near_field(c, x, None, None, 5.0, 0.3)


@pytest.mark.parametrize("columns", [1, 2, 5])
def test_crowded_corner(crowded, columns):
    x, c, ref, fref = crowded
    assert x.shape == (2744, 3) and (x > 0.5).any(0).all() and (x < 0.5).any(0).all()
    assert dr.min_separation(x) >= 0.01
    c, ref, fref = c[:, :columns], ref[:, :columns], fref[:, :, :columns]
    z, f = _sweep("cube", x, c, None, 5.0, 0.3, True)
    z, f = z.cpu().numpy(), f.cpu().numpy()
    err, ferr = rel_l2(z, ref), rel_l2(f, fref)
    print("dispersion near, crowded corner, %d columns: value rel_l2 %.3e (worst point %.3e), field rel_l2 %.3e (worst point "
          "%.3e)" % (columns, err, _max_pointwise(z, ref), ferr, _max_pointwise(f, fref)))
    assert err <= NEAR_TOL["crowded_value"] and ferr <= NEAR_TOL["crowded_field"]
    # no atomics: the same bits again, and the value-only instantiation adds the same pairs
    z2, f2 = _sweep("cube", x, c, None, 5.0, 0.3, True)
    z3, _ = _sweep("cube", x, c, None, 5.0, 0.3, False)
    assert np.array_equal(z2.cpu().numpy(), z) and np.array_equal(f2.cpu().numpy(), f) and np.array_equal(z3.cpu().numpy(), z)


WHOLE = (14.0, 0.25, 32)  # alpha, r_c, N: the pair factor at r_c is 4e-4, f(b) on the plane k_a = 16 is 3e-7 (1e-4 in O)


@pytest.fixture(scope="module")
def whole():
    """7^3 points on a jittered lattice (spacing 1/7, jitter 0.03) in two point sets, two columns c and a weight g; per box
    the float64 algorithm's (psi, G) of both on the fractional float32 positions"""
    rng = np.random.default_rng(3)
    s = rng.permutation(dr.jittered_lattice(rng, 7, 1.0 / 7, 0.03).reshape(-1, 3))
    n = s.shape[0]
    c, g = _values(rng, n, (2,), False), rng.standard_normal((n, 2)).astype(np.float32)
    batch = (np.arange(n) >= 160).astype(np.int64)
    alpha, r_c, N = WHOLE
    ref = {}
    for box, A in BOXES.items():
        ref[box] = (dr.dispersion(c, s, A, batch, alpha, r_c, N), dr.dispersion(g, s, A, batch, alpha, r_c, N))
    return s, c, g, batch, ref


def _splitting(box):
    import torch_nfft_amd as tn
    A = BOXES[box]
    return tn.DispersionSplitting(WHOLE[0], WHOLE[1], WHOLE[2], box=None if A is None else torch.from_numpy(A))


@pytest.mark.parametrize("box", ["cube", "T", "O"])
def test_whole_sum_and_field(whole, box):
    import torch_nfft_amd as tn
    s, c, g, batch, ref = whole
    (psi_ref, G_ref), _ = ref[box]
    sp = _splitting(box)
    frac = dict(fractional=True) if BOXES[box] is not None else {}
    psi, G = tn.nfft_ewald_dispersion(_cuda(c), _cuda(s), _cuda(batch), splitting=sp, cutoff=4, field=True, **frac)
    only = tn.nfft_ewald_dispersion(_cuda(c), _cuda(s), _cuda(batch), splitting=sp, cutoff=4, **frac)
    tn.ops.check_status()
    assert psi.shape == c.shape and G.shape == (c.shape[0], 3, 2) and psi.dtype == G.dtype == torch.float32
    assert not G.requires_grad
    for what, got, want in (("value", psi, psi_ref), ("value", only, psi_ref), ("field", G, G_ref)):
        got = got.cpu().numpy()
        err = rel_l2(got, want)
        print("nfft_ewald_dispersion %s in %s: rel_l2 vs the float64 algorithm %.3e, worst point %.3e"
              % (what, box, err, _max_pointwise(got, want)))
        assert err <= WHOLE_TOL[what]
    if BOXES[box] is not None:  # Cartesian input: x = s A in float32 has lost the last bits of s; the sums move by that much
        xc = (s.astype(np.float64) @ BOXES[box]).astype(np.float32)
        sc = xc.astype(np.float64) @ np.linalg.inv(BOXES[box])
        psi_c, G_c = tn.nfft_ewald_dispersion(_cuda(c), _cuda(xc), _cuda(batch), splitting=sp, cutoff=4, field=True)
        tn.ops.check_status()
        alpha, r_c, N = WHOLE
        want_c = dr.dispersion(c, sc.astype(np.float32), BOXES[box], batch, alpha, r_c, N)
        ev, ef = rel_l2(psi_c.cpu().numpy(), want_c[0]), rel_l2(G_c.cpu().numpy(), want_c[1])
        print("nfft_ewald_dispersion in %s, Cartesian input: value rel_l2 %.3e, field rel_l2 %.3e" % (box, ev, ef))
        assert ev <= WHOLE_TOL["value"] and ef <= WHOLE_TOL["field"]
    U = tn.nfft_ewald_dispersion_energy(_cuda(c), _cuda(s), _cuda(batch), splitting=sp, cutoff=4, **frac).cpu().numpy()
    assert U.shape == (2, 2)
    for b in (0, 1):  # (a sum of products, each good to WHOLE_TOL of |c| |psi|: Cauchy-Schwarz, per column)
        sel = batch == b
        want = 0.5 * (c[sel].astype(np.float64) * psi_ref[sel]).sum(0)
        bound = WHOLE_TOL["value"] * 0.5 * np.linalg.norm(c[sel], axis=0) * np.linalg.norm(psi_ref[sel], axis=0)
        assert (np.abs(U[b] - want) <= bound).all()


@pytest.mark.parametrize("box,fractional", [("cube", False), ("T", True), ("T", False), ("O", True)])
def test_autograd(whole, box, fractional):
    import torch_nfft_amd as tn
    s, c, g, batch, ref = whole
    (psi_c, G_c), (psi_g, G_g) = ref[box]
    A = BOXES[box]
    sp = _splitting(box)
    kw = dict(splitting=sp, cutoff=4, fractional=fractional)
    pos = s if (A is None or fractional) else (s.astype(np.float64) @ A).astype(np.float32)
    if A is not None and not fractional:  # the reference on the fractional positions that the float32 Cartesian ones stand for
        sf = (pos.astype(np.float64) @ np.linalg.inv(A)).astype(np.float32)
        alpha, r_c, N = WHOLE
        (psi_c, G_c), (psi_g, G_g) = dr.dispersion(c, sf, A, batch, alpha, r_c, N), dr.dispersion(g, sf, A, batch, alpha, r_c, N)
    cd, xd, gd, bd = _cuda(c).requires_grad_(True), _cuda(pos).requires_grad_(True), _cuda(g), _cuda(batch)
    psi = tn.nfft_ewald_dispersion(cd, xd, bd, **kw)
    dc, dx = torch.autograd.grad((psi * gd).sum(), (cd, xd))
    tn.ops.check_status()
    # dc: the operator applied to g
    own = tn.nfft_ewald_dispersion(gd, xd.detach(), bd, **kw)
    e_own, e_ref = rel_l2(dc.cpu().numpy(), own.cpu().numpy()), rel_l2(dc.cpu().numpy(), psi_g)
    print("nfft_ewald_dispersion dc in %s: rel_l2 vs the operator on g %.3e, vs float64 %.3e" % (box, e_own, e_ref))
    assert e_own <= 2 * WHOLE_TOL["value"] and e_ref <= WHOLE_TOL["value"]
    # dpos_i = -sum_c (g_ic G[c]_i + c_ic G[g]_i) (Cartesian), times A^T for fractional input; each field is good to
    # WHOLE_TOL["field"] in l2 and is weighted by at most max |g| or max |c|
    want = -(g[:, None, :] * G_c + c[:, None, :] * G_g).sum(2)
    bound = WHOLE_TOL["field"] * (np.abs(g).max() * np.linalg.norm(G_c) + np.abs(c).max() * np.linalg.norm(G_g))
    if fractional:
        want = want @ A.T
        bound *= np.linalg.norm(A, 2)
    err = np.linalg.norm(dx.cpu().numpy() - want)
    print("nfft_ewald_dispersion dpos in %s: |error| %.3e, bound %.3e, rel_l2 %.3e" % (box, err, bound, rel_l2(dx.cpu().numpy(), want)))
    assert dx.shape == pos.shape and err <= bound
    # the energy: dU/dpos_i = -sum_c c_ic G[c]_i
    xe = _cuda(pos).requires_grad_(True)
    U = tn.nfft_ewald_dispersion_energy(_cuda(c), xe, bd, **kw)
    de, = torch.autograd.grad(U.sum(), xe)
    tn.ops.check_status()
    want = -(c[:, None, :] * G_c).sum(2)
    bound = WHOLE_TOL["field"] * np.abs(c).max() * np.linalg.norm(G_c)
    if fractional:
        want = want @ A.T
        bound *= np.linalg.norm(A, 2)
    err = np.linalg.norm(de.cpu().numpy() - want)
    print("nfft_ewald_dispersion_energy dpos in %s: |error| %.3e, bound %.3e" % (box, err, bound))
    assert err <= bound


def test_second_derivative_and_refusals(whole):
    import torch_nfft_amd as tn
    s, c, g, batch, _ = whole
    sp = _splitting("cube")
    cd, xd, bd = _cuda(c).requires_grad_(True), _cuda(s).requires_grad_(True), _cuda(batch)
    psi, G = tn.nfft_ewald_dispersion(cd, xd, bd, splitting=sp, field=True)
    assert psi.requires_grad and not G.requires_grad
    dc, dx = torch.autograd.grad(psi.square().sum(), (cd, xd), create_graph=True)
    with pytest.raises(RuntimeError, match="differentiate twice|once_differentiable"):
        dx.square().sum().backward()
    with pytest.raises(AssertionError, match="batch"):
        tn.nfft_ewald_dispersion(cd, xd, torch.zeros(343, device="cuda", requires_grad=True), splitting=sp)
    with pytest.raises(TypeError, match="DispersionSplitting"):
        tn.nfft_ewald_dispersion(cd, xd, bd, splitting=tn.EwaldSplitting(14.0, 0.25, 32))
    with pytest.raises(RuntimeError, match="Input mismatch"):
        tn.ops.nfft_ewald_dispersion_near(xd.detach(), cd.detach(), bd, 5.0, 0.34, False)
    with pytest.raises(RuntimeError, match="Input mismatch"):
        tn.ops.nfft_ewald_dispersion_near_box(xd.detach(), cd.detach(), bd, _box6(O), 5.0, 0.3, False)
    # empty input
    q0 = torch.zeros(0, 2, device="cuda", requires_grad=True)
    x0 = torch.zeros(0, 3, device="cuda", requires_grad=True)
    psi, G = tn.nfft_ewald_dispersion(q0, x0, splitting=sp, field=True)
    assert psi.shape == (0, 2) and G.shape == (0, 3, 2)
    dq, dx0 = torch.autograd.grad(psi.sum(), (q0, x0))
    assert dq.shape == (0, 2) and dx0.shape == (0, 3)
    z, f = tn.ops.nfft_ewald_dispersion_near(x0.detach(), q0.detach(), None, 5.0, 0.3, True)
    assert z.shape == (0, 2) and f.shape == (0, 3, 2)


@pytest.mark.parametrize("box", ["cube", "T"])
def test_converged_sum(box):
    """One small set against the brute-force lattice sum: |device - lattice| <= |device - algorithm| + |algorithm - lattice|,
    the first within WHOLE_TOL of |algorithm| <= (1 + e_own) |lattice|, the second e_own |lattice| computed here in float64.
    The set is a cluster across the box corner (4^3 points, spacing 0.1): its psi (1.5e6 and more per unit of c) is larger than the self term.
    A sparse set is no yardstick for WHOLE_TOL: at spacing 0.25 psi is a fiftieth of the self term alpha^6 / 6 that the far sum
    has to cancel, and the first device run stood 2.2e-5 (cube) and 2.9e-5 (T) from the algorithm there."""
    import torch_nfft_amd as tn
    A = BOXES[box]
    rng = np.random.default_rng(9)
    s = dr.jittered_lattice(rng, 4, 0.1, 0.02, centre=0.45).reshape(-1, 3)
    assert (s > 0.5).any(0).all() and dr.min_separation(s, A) >= 0.04
    c = _values(rng, 64, (), False)
    alpha, r_c, N = WHOLE
    lat = dr.lattice_sum(c, s, A, 8.0)
    alg = dr.dispersion(c, s, A, None, alpha, r_c, N)
    sp = _splitting(box)
    frac = dict(fractional=True) if A is not None else {}
    got = tn.nfft_ewald_dispersion(_cuda(c), _cuda(s), splitting=sp, cutoff=4, field=True, **frac)
    tn.ops.check_status()
    for what, k in (("value", 0), ("field", 1)):
        e_own, e_conv = rel_l2(alg[k], lat[k]), rel_l2(got[k].cpu().numpy(), lat[k])
        print("nfft_ewald_dispersion %s in %s: rel_l2 vs the lattice sum %.3e (the algorithm's own %.3e, vs the algorithm %.3e)"
              % (what, box, e_conv, e_own, rel_l2(got[k].cpu().numpy(), alg[k])))
        assert e_conv <= WHOLE_TOL[what] * (1 + e_own) + e_own
