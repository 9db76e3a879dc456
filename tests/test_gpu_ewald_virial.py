"""GPU tests of the Ewald virial tensor: the pair reduction and the spectral reduction of
csrc/ewald_virial.hip on their own, then nfft_ewald_virial as a whole, against the float64 restatement
tests/ewald_virial_ref.py evaluated on the same float32 fractional positions.  Everything is compared in the relative
Frobenius / l2 norm.

Tolerances.  As in tests/test_gpu_ewald_box.py: each is 4x the largest figure of the first device run (the figure behind
each entry is in its comment and in section 7i); a first-run figure above 1e-4 would have been a defect, not a tolerance.
What these must not hide is wrong by far more (tests/test_ewald_virial_ref.py::test_mutants_are_far_off): the fractional
difference in place of d 0.15, A^T in place of A 0.16, k in place of kappa 2.7, the term pi^2 / alpha^2 left out 2.5, the
background left out 0.036.  Against the converged sum the bound is the triangle inequality with the algorithm's own
truncation error, no free number.
"""
import math

import numpy as np
import pytest
import torch

import ewald_box_ref as eb
import ewald_ref as er
import ewald_virial_ref as ev

pytestmark = pytest.mark.gpu

NEAR_TOL = {  # 4 x the largest figure of the first device run (in brackets)
    # (2.04e-6: T at (30, 0.12), three sets, one column, where |ref| is 54 against 300 .. 2300 elsewhere; 1.28e-6 and
    # 8.7e-7 next, 8.2e-8 .. 5.2e-7 on the thirty-seven other cases of 700 points)
    "seven": 8.2e-6,
    "crowded": 2.6e-6,  # (6.45e-7)
}
# float64 against float64 on the same float32 coefficients: what is left is the order of the additions, numpy's included
# (with three columns its einsum adds 5e5 cells one after the other: 1.7e-14 .. 9.3e-14 there, 3e-16 .. 3e-15 with one)
FAR_TOL = 3.8e-13  # (9.28e-14: N = 80 in T, three columns; 6.39e-14 at N = 72, 2.36e-14 at N = 32)
WHOLE_TOL = {  # nfft_ewald_virial (cutoff = 4) against the float64 algorithm
    "W": 3.2e-6,  # (7.95e-7 in O; 5.99e-7 in T, 4.06e-7 and 3.55e-7 on 300 charges)
    # U = 130 and 14.5 (T), 140 and 43.9 (O) are what is left of a self term of 2700 .. 3200 and a far sum of that size
    # which carries the transform's error at cutoff = 4; nfft_ewald_energy, made from the same transform, has the same
    "U": 5.5e-5,  # (1.36e-5 in O; 1.32e-5 in T, 1.09e-6 and 1.08e-6 on 300 charges)
    "energy": 3.8e-6,  # U against nfft_ewald_energy of the same call (9.33e-7 in T, 6.30e-7 in O)
    # one or two charges: U and W are differences of terms many times their size, as in 7h
    "fixed_point": 2.0e-5,  # (4.83e-6: primitive rock salt; one charge in the unit cube 1.48e-6, in S 2.15e-6)
    "cartesian": 2.6e-6,  # Cartesian against fractional input (W 6.37e-7, U 1.45e-7)
}
# Two calls of nfft_ewald_virial need not give the same bits: the two reductions do, the adjoint transform before them
# spreads with float atomics.  Where two calls are compared, each is within WHOLE_TOL of the float64 algorithm, so they
# differ by at most twice that.

BOXES = {"T": eb.T, "O": eb.O, "S": eb.S, "I": np.eye(3)}


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _six(A):
    return [A[0, 0], A[1, 0], A[1, 1], A[2, 0], A[2, 1], A[2, 2]]


def _seven(U, W):
    """(U, W) of the restatement in the layout of the two operators: [B, 7, *cols], energy, xx, yy, zz, yz, xz, xy"""
    return np.stack([U, W[:, 0, 0], W[:, 1, 1], W[:, 2, 2], W[:, 1, 2], W[:, 0, 2], W[:, 0, 1]], 1)


def _ragged_batch(rng, n):
    """three point sets, the middle one empty"""
    b = np.sort(rng.integers(0, 2, n)) * 2
    b[0], b[-1] = 0, 2
    return b.astype(np.int64)


def _box_points(rng, n):
    """n float32 FRACTIONAL points uniform in the box and, among the first hundred (one point set of the ragged cases),
    every edge case of the wrap (those of tests/test_gpu_ewald_box.py, restated)"""
    x = (rng.random((n, 3)) - 0.5).astype(np.float32)
    x[40:60] = x[0:20]                                    # exact duplicates: r = 0
    below = np.nextafter(np.float32(0.5), np.float32(0))  # the largest float32 below 1/2
    for a in range(3):
        x[60 + a, a] = -0.5                               # exactly on the lower face
        x[63 + a, a] = below
        x[66 + a] = x[60 + a] + np.float32(0.01) * rng.random(3).astype(np.float32)  # ... each with a close neighbour
        x[69 + a] = x[63 + a] - np.float32(0.01) * rng.random(3).astype(np.float32)
    x[63, :] = below                                      # (the upper corner; none in the lower one, see there)
    x[72:80] += np.float32(0.7)                           # given outside the box: must act as their images
    x[80:88] -= np.float32(1.2)
    for a in range(3):                                    # a pair straddling each face
        y = (rng.random(3) - 0.5).astype(np.float32)
        x[88 + 2 * a] = y
        x[89 + 2 * a] = y + np.float32(0.003)
        x[88 + 2 * a, a] = 0.49
        x[89 + 2 * a, a] = -0.49
    return x


# box, alpha, r_c, the cells
NEAR_SPLITS = [("O", 14.0, 0.25, (4, 5, 3)), ("T", 12.0, 0.3, (3, 3, 3)), ("T", 30.0, 0.12, (7, 8, 7)),
               ("S", 16.0, 0.22, (3, 4, 4)), ("I", 12.0, 0.3, (3, 3, 3))]


@pytest.mark.parametrize("cols", [(), (2,), (3,), (5,)])  # (five columns: the CC = 4 pass twice, the tail masked)
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("name,alpha,r_c,cells", NEAR_SPLITS)
def test_near_reduction_against_brute_force(name, alpha, r_c, cells, ragged, cols):
    import torch_nfft_amd as tn
    A = BOXES[name]
    assert tn.EwaldSplitting(alpha, r_c, 4, box=A).cells == cells
    rng = np.random.default_rng(int(alpha) * 100 + len(cols) + 10 * ragged + ord(name))
    n = 700
    s = _box_points(rng, n)
    q = rng.standard_normal((n,) + cols).astype(np.float32)
    batch = _ragged_batch(rng, n) if ragged else None
    if batch is not None:
        assert (batch[:100] == 0).all()  # the edge cases share a point set
    out = tn.ops.nfft_ewald_virial_near(_cuda(s), _cuda(q), _cuda(batch), _six(A), alpha, r_c)
    tn.ops.check_status()
    B = 3 if ragged else 1
    assert out.shape == (B, 7) + cols and out.dtype == torch.float64
    out = out.cpu().numpy()
    ref = _seven(*ev.near_virial(q, s, A, batch, alpha, r_c))
    err = ev.rel_fro(out, ref)
    print("virial near, box %s (%g, %g) ragged=%d cols=%s: rel %.3e (|ref| %.3e)" % (name, alpha, r_c, ragged, cols, err,
                                                                                     np.linalg.norm(ref)))
    assert np.linalg.norm(ref[:, 0]) > 0 and np.linalg.norm(ref[:, 4:]) > 0
    assert err <= NEAR_TOL["seven"]
    if ragged:
        assert not out[1].any()  # the empty point set: exactly zero
        assert out[0].all() and out[2].all()


@pytest.fixture(scope="module")
def crowded():
    """3000 points in a fractional cube of edge 0.06 centred on the corner (1/2, 1/2, 1/2) of the box T (that of
    tests/test_gpu_ewald_box.py): ~375 in each of the eight corner cells -- three items per cell, the last with 119
    targets, so both waves of a workgroup live with idle lanes in the second, and two LDS tiles per cell"""
    rng = np.random.default_rng(7)
    s = (0.5 + (rng.random((3000, 3)) - 0.5) * 0.06).astype(np.float32)
    q = rng.standard_normal(3000).astype(np.float32)
    return s, q


def test_crowded_corner(crowded):
    import torch_nfft_amd as tn
    s, q = crowded
    out = tn.ops.nfft_ewald_virial_near(_cuda(s), _cuda(q), None, _six(eb.T), 12.0, 0.3)
    tn.ops.check_status()
    ref = _seven(*ev.near_virial(q, s, eb.T, None, 12.0, 0.3))
    err = ev.rel_fro(out.cpu().numpy(), ref)
    print("virial near, box T, crowded corner: rel %.3e" % err)
    assert err <= NEAR_TOL["crowded"]


def test_two_calls_are_bitwise_equal(crowded):
    import torch_nfft_amd as tn
    s, q = crowded
    sd, qd = _cuda(s), _cuda(np.stack([q, -q[::-1], q * q], 1))
    a = tn.ops.nfft_ewald_virial_near(sd, qd, None, _six(eb.T), 12.0, 0.3)
    b = tn.ops.nfft_ewald_virial_near(sd, qd, None, _six(eb.T), 12.0, 0.3)
    assert a.shape == (1, 7, 3) and bool(a.all()) and torch.equal(a, b)
    band = torch.randn(2, 12, 12, 12, 3, dtype=torch.complex64, device="cuda")
    sp = tn.EwaldSplitting(12.0, 0.3, 12, box=eb.T)
    a = tn.ops.nfft_ewald_virial_far(band, sp.coeffs, sp.box6, 12.0)
    b = tn.ops.nfft_ewald_virial_far(band, sp.coeffs, sp.box6, 12.0)
    assert a.shape == (2, 7, 3) and bool(a.all()) and torch.equal(a, b)


@pytest.mark.parametrize("cols", [(2,), (4,)])
def test_far_reduction_of_a_band_that_is_not_16_byte_aligned(cols):
    """a contiguous view one complex64 into its storage: the cells are read with 8-byte loads, the sums are the same"""
    import torch_nfft_amd as tn
    sp = tn.EwaldSplitting(6.0, 0.25, 8, box=eb.T)
    shape = (2, 8, 8, 8) + cols
    buf = torch.randn(1 + math.prod(shape), dtype=torch.complex64, device="cuda")
    band = buf[1:].view(shape)
    assert band.is_contiguous() and band.data_ptr() % 16 == 8
    aligned = band.clone()
    assert aligned.data_ptr() % 16 == 0
    a = tn.ops.nfft_ewald_virial_far(band, sp.coeffs, sp.box6, 6.0)
    b = tn.ops.nfft_ewald_virial_far(aligned, sp.coeffs, sp.box6, 6.0)
    tn.ops.check_status()
    assert bool(a.all()) and torch.equal(a, b)


def test_no_points():
    import torch_nfft_amd as tn
    pos = torch.zeros(0, 3, device="cuda")
    out = tn.ops.nfft_ewald_virial_near(pos, torch.zeros(0, 2, device="cuda"), None, _six(eb.T), 12.0, 0.3)
    assert out.shape == (1, 7, 2) and out.dtype == torch.float64 and not bool(out.any())
    out = tn.ops.nfft_ewald_virial_near(pos, torch.zeros(0, device="cuda"), None, _six(eb.T), 12.0, 0.3)
    assert out.shape == (1, 7) and not bool(out.any())
    sp = tn.EwaldSplitting(12.0, 0.3, 16, box=eb.T)
    U, W = tn.nfft_ewald_virial(torch.zeros(0, 2, device="cuda"), pos, splitting=sp)
    assert U.shape == (1, 2) and W.shape == (1, 3, 3, 2) and U.dtype == W.dtype == torch.float32
    assert not bool(U.any()) and not bool(W.any())
    with pytest.raises(RuntimeError, match="Input mismatch"):
        tn.ops.nfft_ewald_virial_near(torch.zeros(4, 3, device="cuda"), torch.zeros(4, dtype=torch.complex64, device="cuda"),
                                      None, _six(eb.T), 12.0, 0.3)
    with pytest.raises(RuntimeError, match="Input mismatch"):
        tn.ops.nfft_ewald_virial_near(torch.zeros(4, 3, device="cuda"), torch.zeros(4, device="cuda"), None, _six(eb.T), 12.0, 0.31)


# N = 6: 216 cells, not a multiple of any block size, one workgroup with idle lanes; 32: 128 workgroups per point set;
# 64: 1024 workgroups of 256, one cell per thread exactly.  72 and 80: more cells than the 262144 threads of a point set,
# so 42 % and 95 % of the threads take a second cell and the index is advanced by the stride, whose three digits in base N
# are all non-zero there (50, 40, 64 and 40, 76, 64): both carries happen.  alpha = 40 from N = 64 on, so that the
# coefficients of those later cells count (their Gaussian factor is above 0.02 out to |kappa| = 24).  Columns: one, two and four take whole
# cells in one or two loads, three has a masked tail, five runs the four-column pass twice.
FAR_CASES = [(N, name, cols) for N in (6, 8, 12, 32) for name in ("T", "O") for cols in ((), (3,))] + \
            [(8, "T", (2,)), (8, "T", (4,)), (8, "O", (5,)), (64, "T", ()),
             (72, "T", ()), (72, "O", (3,)), (80, "O", ()), (80, "T", (3,))]


@pytest.mark.parametrize("N,name,cols", FAR_CASES)
def test_far_reduction_against_dense_sum(N, name, cols):
    import torch_nfft_amd as tn
    A = BOXES[name]
    alpha = 40.0 if N >= 64 else (12.0 if N >= 12 else 6.0)  # (so that the coefficients count out to the grid's edge)
    sp = tn.EwaldSplitting(alpha, 0.25, N, box=A)
    rng = np.random.default_rng(N + len(cols) + ord(name))
    shape = (2, N, N, N) + cols
    band = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)
    out = tn.ops.nfft_ewald_virial_far(_cuda(band), sp.coeffs, sp.box6, alpha)
    tn.ops.check_status()
    assert out.shape == (2, 7) + cols and out.dtype == torch.float64
    ref = _seven(*ev.far_virial(band, sp.coeffs.cpu().numpy(), A, alpha))  # (the splitting's own float32 coefficients)
    err = ev.rel_fro(out.cpu().numpy(), ref)
    print("virial far, N %d box %s cols %s: rel %.3e (|ref| %.3e)" % (N, name, cols, err, np.linalg.norm(ref)))
    assert np.linalg.norm(ref[:, 4:]) > 0
    assert err <= FAR_TOL


WHOLE = {"T": (12.0, 0.3, 32), "O": (14.0, 0.25, 48)}


@pytest.fixture(scope="module")
def whole():
    """800 charges in two point sets, neither neutral, fractional float32 positions (those of
    tests/test_gpu_ewald_box.py); per box the float64 algorithm and the converged sum (one shell of images, as there)"""
    rng = np.random.default_rng(3)
    n = 800
    s = (rng.random((n, 3)) - 0.5).astype(np.float32)
    q = rng.standard_normal(n).astype(np.float32)
    batch = (np.arange(n) >= 370).astype(np.int64)
    done = {}

    def get(name):
        if name not in done:
            alpha, r_c, N = WHOLE[name]
            done[name] = (ev.exact_algorithm_virial(q, s, BOXES[name], batch, alpha, r_c, N),
                          ev.converged_virial(q, s, BOXES[name], batch, nimg=1))
        return done[name]

    return s, q, batch, get


@pytest.mark.parametrize("name", ["T", "O"])
def test_whole_virial(whole, name):
    import torch_nfft_amd as tn
    s, q, batch, get = whole
    (Ua, Wa), (Uc, Wc) = get(name)
    alpha, r_c, N = WHOLE[name]
    sp = tn.EwaldSplitting(alpha, r_c, N, box=BOXES[name])
    qd, sd, bd = _cuda(q), _cuda(s), _cuda(batch)
    U, W = tn.nfft_ewald_virial(qd, sd, bd, splitting=sp, cutoff=4, fractional=True)
    energy = tn.nfft_ewald_energy(qd, sd, bd, splitting=sp, cutoff=4, fractional=True)
    tn.ops.check_status()
    assert U.shape == (2,) and W.shape == (2, 3, 3) and U.dtype == W.dtype == torch.float32
    assert torch.equal(W, W.transpose(1, 2))
    U, W, energy = U.cpu().numpy(), W.cpu().numpy(), energy.cpu().numpy()
    for what, got, alg, conv in (("W", W, Wa, Wc), ("U", U, Ua, Uc)):
        e_alg, e_own, e_conv = ev.rel_fro(got, alg), ev.rel_fro(alg, conv), ev.rel_fro(got, conv)
        print("nfft_ewald_virial, box %s, %s: rel vs the float64 algorithm %.3e, vs the converged sum %.3e (the algorithm's "
              "own %.3e)" % (name, what, e_alg, e_conv, e_own))
        assert e_alg <= WHOLE_TOL[what]
        # the triangle inequality |got - conv| <= |got - alg| + |alg - conv| with the tolerance in place of the first term
        assert np.linalg.norm(got - conv) <= WHOLE_TOL[what] * np.linalg.norm(alg) + np.linalg.norm(alg - conv)
    e_energy = ev.rel_fro(U, energy)
    print("nfft_ewald_virial, box %s: U vs nfft_ewald_energy %.3e (%s, %s)" % (name, e_energy, U, energy))
    assert e_energy <= WHOLE_TOL["energy"]
    # tr W = U for the converged sum: the device's two differ by no more than their two measured errors against it
    # (|tr E| <= sqrt(3) |E|_F)
    for b in (0, 1):
        bound = math.sqrt(3.0) * np.linalg.norm(W[b] - Wc[b]) + abs(U[b] - Uc[b]) + 4e-9
        print("set %d: tr W - U = %.3e, bound %.3e (U = %.7g)" % (b, np.trace(W[b]) - U[b], bound, U[b]))
        assert abs(np.trace(W[b].astype(np.float64)) - U[b]) <= bound


def _fixed_point(what, q, s, A, split, want):
    """U and W = (U / 3) I of nfft_ewald_virial against the lattice constant: the device against the float64 algorithm,
    then the triangle inequality with the algorithm's own truncation"""
    import torch_nfft_amd as tn
    alpha, r_c, N = split
    sp = tn.EwaldSplitting(alpha, r_c, N, box=A)
    U, W = tn.nfft_ewald_virial(_cuda(q), _cuda(s), splitting=sp, cutoff=4, fractional=A is not None)
    tn.ops.check_status()
    U, W = U.cpu().numpy(), W.cpu().numpy()
    Ua, Wa = ev.exact_algorithm_virial(q, s, np.eye(3) if A is None else A, None, alpha, r_c, N)
    ideal = want / 3.0 * np.eye(3)
    own = max(abs(Ua[0] - want) / abs(want), np.abs(Wa[0] - ideal).max() / abs(want / 3.0))
    e_alg = max(ev.rel_fro(U, Ua), ev.rel_fro(W, Wa))
    e_const = max(abs(U[0] - want) / abs(want), np.abs(W[0] - ideal).max() / abs(want / 3.0))
    print("%s: U = %.7f (%.7f), diag W = %s, relative error %.3e, vs the float64 algorithm %.3e (its own %.1e)"
          % (what, U[0], want, np.diag(W[0]), e_const, e_alg, own))
    assert own <= 1e-8
    assert e_alg <= WHOLE_TOL["fixed_point"]
    assert e_const <= math.sqrt(3.0) * WHOLE_TOL["fixed_point"] + own  # (the largest entry against the Frobenius norm)


def test_fixed_points():
    """cubic symmetry: W = (U / 3) I, U / q^2 at the lattice constants"""
    q1 = np.array([1.5], dtype=np.float32)
    _fixed_point("one charge in the unit cube", q1, np.array([[0.2, -0.4, 0.1]], dtype=np.float32), None, (16.0, 0.3, 64),
                 0.5 * er.CUBIC_LATTICE * 2.25)
    _fixed_point("one charge in S", q1, np.array([[0.31, -0.47, 0.123]], dtype=np.float32), eb.S, (16.0, 0.22, 64),
                 0.5 * er.CUBIC_LATTICE * 2.25)
    A, _ = eb.lower_triangular(eb.ROCK_SALT_PRIMITIVE)
    _fixed_point("primitive rock salt", np.array([1.0, -1.0], dtype=np.float32),
                 np.array([[0.0, 0.0, 0.0], [-0.5, -0.5, -0.5]], dtype=np.float32), A, (21.0, 0.19, 48), -2.0 * er.MADELUNG_NACL)


@pytest.fixture(scope="module")
def small():
    """300 charges in two point sets in the box T, two columns: float32 fractional positions s0 and their float32
    Cartesian positions x = s0 A (float64 product, rounded once)"""
    rng = np.random.default_rng(4)
    n = 300
    s0 = (rng.random((n, 3)) - 0.5).astype(np.float32)
    x = (s0.astype(np.float64) @ eb.T).astype(np.float32)
    q = rng.standard_normal((n, 2)).astype(np.float32)
    batch = (np.arange(n) >= 140).astype(np.int64)
    return x, s0, q, batch


def test_cartesian_input_and_columns(small):
    import torch_nfft_amd as tn
    x, s0, q, batch = small
    sp = tn.EwaldSplitting(12.0, 0.3, 32, box=eb.T)
    Ux, Wx = tn.nfft_ewald_virial(_cuda(q), _cuda(x), _cuda(batch), splitting=sp)
    Us, Ws = tn.nfft_ewald_virial(_cuda(q), _cuda(s0), _cuda(batch), splitting=sp, fractional=True)
    tn.ops.check_status()
    assert Ux.shape == (2, 2) and Wx.shape == (2, 3, 3, 2)
    Ua, Wa = ev.exact_algorithm_virial(q, s0, eb.T, batch, 12.0, 0.3, 32)
    e_U, e_W = ev.rel_fro(Ux.cpu().numpy(), Us.cpu().numpy()), ev.rel_fro(Wx.cpu().numpy(), Ws.cpu().numpy())
    a_U, a_W = ev.rel_fro(Us.cpu().numpy(), Ua), ev.rel_fro(Ws.cpu().numpy(), Wa)
    print("Cartesian input: U %.3e W %.3e vs fractional input; fractional vs float64: U %.3e W %.3e" % (e_U, e_W, a_U, a_W))
    assert max(e_U, e_W) <= WHOLE_TOL["cartesian"]
    assert a_U <= WHOLE_TOL["U"] and a_W <= WHOLE_TOL["W"]
    # the gradient in the box entries, through the public helper on the device
    G = tn.virial_to_box_gradient(Ws, sp.box)
    want = -np.einsum("ki,bkjc->bijc", np.linalg.inv(eb.T), Wa) * np.tril(np.ones((3, 3)))[None, :, :, None]
    assert G.shape == (2, 3, 3, 2) and G.is_cuda
    # |tril(A^-T E)|_F <= |A^-1|_2 |E|_F for the error E of W, plus the float32 rounding of the product itself
    scale = np.linalg.norm(np.linalg.inv(eb.T), 2) * np.linalg.norm(Wa)
    assert np.linalg.norm(G.cpu().numpy() - want) <= (WHOLE_TOL["W"] + 4 * 2.0 ** -24) * scale


def test_box_none_is_the_identity_box(small):
    import torch_nfft_amd as tn
    _, s0, q, batch = small
    cube = tn.EwaldSplitting(12.0, 0.3, 32)
    ident = tn.EwaldSplitting(12.0, 0.3, 32, box=(1, 1, 1))
    Uc, Wc = tn.nfft_ewald_virial(_cuda(q), _cuda(s0), _cuda(batch), splitting=cube)
    Ui, Wi = tn.nfft_ewald_virial(_cuda(q), _cuda(s0), _cuda(batch), splitting=ident, fractional=True)
    tn.ops.check_status()
    Ua, Wa = ev.exact_algorithm_virial(q, s0, np.eye(3), batch, 12.0, 0.3, 32)
    e_U, e_W = ev.rel_fro(Uc.cpu().numpy(), Ui.cpu().numpy()), ev.rel_fro(Wc.cpu().numpy(), Wi.cpu().numpy())
    a_U, a_W = ev.rel_fro(Uc.cpu().numpy(), Ua), ev.rel_fro(Wc.cpu().numpy(), Wa)
    print("box=None vs the identity box: U %.3e W %.3e; box=None vs float64: U %.3e W %.3e" % (e_U, e_W, a_U, a_W))
    assert e_U <= 2 * WHOLE_TOL["U"] and e_W <= 2 * WHOLE_TOL["W"]  # (equal bits on the first run)
    assert a_U <= WHOLE_TOL["U"] and a_W <= WHOLE_TOL["W"]


def test_refusals_and_autograd(small):
    import torch_nfft_amd as tn
    x, s0, q, batch = small
    sp = tn.EwaldSplitting(12.0, 0.3, 16, box=eb.T)
    qd, xd, bd = _cuda(q), _cuda(x), _cuda(batch)
    with pytest.raises(ValueError, match="real"):
        tn.nfft_ewald_virial(qd.to(torch.complex64), xd, bd, splitting=sp)
    with pytest.raises(AssertionError, match="batch"):
        tn.nfft_ewald_virial(qd, xd, torch.zeros(300, device="cuda", requires_grad=True), splitting=sp)
    with pytest.raises(ValueError, match="fractional"):
        tn.nfft_ewald_virial(qd, xd, bd, splitting=tn.EwaldSplitting(12.0, 0.3, 16), fractional=True)
    # inputs that require grad are accepted; the outputs are constants to autograd
    U, W = tn.nfft_ewald_virial(qd.clone().requires_grad_(True), xd.clone().requires_grad_(True), bd, splitting=sp)
    assert not U.requires_grad and not W.requires_grad and U.grad_fn is None and W.grad_fn is None
    U0, W0 = tn.nfft_ewald_virial(qd, xd, bd, splitting=sp)
    assert ev.rel_fro(U.cpu().numpy(), U0.cpu().numpy()) <= 2 * WHOLE_TOL["U"]
    assert ev.rel_fro(W.cpu().numpy(), W0.cpu().numpy()) <= 2 * WHOLE_TOL["W"]
