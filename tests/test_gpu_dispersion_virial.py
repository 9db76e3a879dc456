"""GPU tests of the virial tensor of the dispersion Ewald sum: the pair reduction and the spectral
reduction of csrc/ewald_disp_virial.hip on their own, then nfft_ewald_dispersion_virial as a whole, against the float64
restatement tests/dispersion_virial_ref.py evaluated on the same float32 fractional positions.  Everything is compared in
the relative Frobenius / l2 norm.

Tolerances.  As in tests/test_gpu_ewald_virial.py and tests/test_gpu_dispersion.py: each is 4x the largest figure of the
first device run (the figure behind each entry is in its comment and in section 7k); a first-run figure above 1e-4 would
have been a defect, not a tolerance.  What these must not hide is wrong by far more
(tests/test_dispersion_virial_ref.py::test_mutants_are_far_off, on the inputs used here): the fractional difference in
place of d 0.37, A^T in place of A 0.23, a^6 dropped from mg 1.2e-3, k in place of kappa 0.08, t_k left out 0.19, the k = 0
term left out 0.61.  The near tests run at alpha r_c = 1.5 for that reason, as those of tests/test_gpu_dispersion.py do.
Against the converged sum the bound is the triangle inequality with the algorithm's own truncation error, no free number.
"""
import math

import numpy as np
import pytest
import torch

import dispersion_ref as dr
import dispersion_virial_ref as dv
import ewald_box_ref as eb

pytestmark = pytest.mark.gpu

NEAR_TOL = {  # 4 x the largest figure of the first device run (in brackets)
    # (1.98e-7: the identity box at (5, 0.3), one set, one column; 1.72e-7 and 1.53e-7 next, 4.7e-8 .. 1.4e-7 on the
    # thirty-seven other cases of 700 points)
    "seven": 7.9e-7,
    # (4.88e-6: every pair is 0.0024 .. 0.1 apart and most go through a wrap, where the float32 difference of two
    # positions is rounded at |ds| ~ 1, 3e-8 absolute, 1e-5 of the closest distances, eight times that in 1 / r^8)
    "crowded": 2.0e-5,
}
# float64 against float64 on the same float32 coefficients: what is left is the order of the additions, numpy's included
FAR_TOL = 2.3e-13  # (5.78e-14: N = 80 in T, three columns; 4.48e-14 at N = 72, 1.18e-14 at N = 32, 1.4e-16 .. 2.7e-15 at N <= 12)
WHOLE_TOL = {  # nfft_ewald_dispersion_virial ((14, 0.25, 32), cutoff = 4) against the float64 algorithm
    "W": 1.2e-6,  # (3.04e-7 in T; 2.46e-7 in O, 2.81e-7 and 2.73e-7 with two columns in T and in the cube)
    # U = 5.2e7 and 6.4e7 (T), 8.5e7 and 8.2e7 (O) are what is left of a self term of 1.0e8 .. 1.3e8 per set and a far sum
    # of that size which carries the transform's error at cutoff = 4; nfft_ewald_dispersion_energy, made from the same
    # transform, has the same
    "U": 4.3e-6,  # (1.08e-6 in T; 8.04e-7 in O, 9.82e-7 and 9.60e-7 with two columns)
    "energy": 6.1e-7,  # U against nfft_ewald_dispersion_energy of the same call (1.51e-7 in O, 1.09e-7 in T)
    "cartesian": 5.4e-7,  # Cartesian against fractional input (U 1.36e-7, W 9.82e-8)
}
# Two calls of nfft_ewald_dispersion_virial need not give the same bits: the two reductions do, the adjoint transform before
# them spreads with float atomics.  Where two calls are compared, each is within WHOLE_TOL of the float64 algorithm, so they
# differ by at most twice that.

BOXES = {"T": eb.T, "O": eb.O, "S": eb.S, "I": np.eye(3)}


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _six(A):
    return [A[0, 0], A[1, 0], A[1, 1], A[2, 0], A[2, 1], A[2, 2]]


def _seven(U, W):
    """(U, W) of the restatement in the layout of the two operators: [B, 7, *cols], energy, xx, yy, zz, yz, xz, xy"""
    return np.stack([U, W[:, 0, 0], W[:, 1, 1], W[:, 2, 2], W[:, 1, 2], W[:, 0, 2], W[:, 0, 1]], 1)


def _splitting(alpha, r_c, N, A):
    import torch_nfft_amd as tn
    return tn.DispersionSplitting(alpha, r_c, N, box=None if A is None else torch.from_numpy(np.ascontiguousarray(A)))


# box, alpha, r_c (alpha r_c = 1.5), the cells
NEAR_SPLITS = [("O", 6.0, 0.25, (4, 5, 3)), ("T", 5.0, 0.3, (3, 3, 3)), ("T", 12.5, 0.12, (7, 8, 7)),
               ("S", 7.0, 0.22, (3, 4, 4)), ("I", 5.0, 0.3, (3, 3, 3))]


@pytest.mark.parametrize("cols", [(), (2,), (3,), (5,)])  # (five columns: the CC = 4 pass twice, the tail masked)
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("name,alpha,r_c,cells", NEAR_SPLITS)
def test_near_reduction_against_brute_force(name, alpha, r_c, cells, ragged, cols):
    import torch_nfft_amd as tn
    A = BOXES[name]
    assert _splitting(alpha, r_c, 4, A).cells == cells
    s = dv.near_points()
    n = s.shape[0]
    assert dr.min_separation(s, A) >= 0.018  # (no pair close enough to be the whole sum; the exact duplicates are skipped)
    rng = np.random.default_rng(int(alpha) * 100 + len(cols) + 10 * ragged + ord(name))
    c = dv.values(rng, n, cols)
    batch = dv.ragged_batch(n) if ragged else None
    out = tn.ops.nfft_ewald_dispersion_virial_near(_cuda(s), _cuda(c), _cuda(batch), _six(A), alpha, r_c)
    tn.ops.check_status()
    B = 3 if ragged else 1
    assert out.shape == (B, 7) + cols and out.dtype == torch.float64
    out = out.cpu().numpy()
    ref = _seven(*dv.near_virial(c, s, A, batch, alpha, r_c))
    err = dv.rel_fro(out, ref)
    print("dispersion virial near, box %s (%g, %g) ragged=%d cols=%s: rel %.3e (|ref| %.3e)" % (name, alpha, r_c, ragged, cols,
                                                                                               err, np.linalg.norm(ref)))
    assert np.linalg.norm(ref[:, 0]) > 0 and np.linalg.norm(ref[:, 4:]) > 0
    assert err <= NEAR_TOL["seven"]
    if ragged:
        assert not out[1].any()  # the empty point set: exactly zero
        assert out[0].all() and out[2].all()


@pytest.fixture(scope="module")
def crowded():
    s = dv.crowded_points()
    c = dv.values(np.random.default_rng(8), s.shape[0], ())
    return s, c


def test_crowded_corner(crowded):
    import torch_nfft_amd as tn
    s, c = crowded
    assert s.shape == (3000, 3) and (s > 0.5).any(0).all() and (s < 0.5).any(0).all()
    assert dr.min_separation(s, eb.T) >= 0.002
    out = tn.ops.nfft_ewald_dispersion_virial_near(_cuda(s), _cuda(c), None, _six(eb.T), 5.0, 0.3)
    tn.ops.check_status()
    ref = _seven(*dv.near_virial(c, s, eb.T, None, 5.0, 0.3))
    err = dv.rel_fro(out.cpu().numpy(), ref)
    print("dispersion virial near, box T, crowded corner: rel %.3e (|ref| %.3e)" % (err, np.linalg.norm(ref)))
    assert err <= NEAR_TOL["crowded"]


def test_two_calls_are_bitwise_equal(crowded):
    import torch_nfft_amd as tn
    s, c = crowded
    sd, cd = _cuda(s), _cuda(np.stack([c, c[::-1], c * c], 1))
    a = tn.ops.nfft_ewald_dispersion_virial_near(sd, cd, None, _six(eb.T), 5.0, 0.3)
    b = tn.ops.nfft_ewald_dispersion_virial_near(sd, cd, None, _six(eb.T), 5.0, 0.3)
    assert a.shape == (1, 7, 3) and bool(a.all()) and torch.equal(a, b)
    band = torch.randn(2, 12, 12, 12, 3, dtype=torch.complex64, device="cuda")
    sp = _splitting(dv.far_alpha(12), 0.25, 12, eb.T)
    a = tn.ops.nfft_ewald_dispersion_virial_far(band, sp.coeffs, sp.strain_coeffs(), sp.box6)
    b = tn.ops.nfft_ewald_dispersion_virial_far(band, sp.coeffs, sp.strain_coeffs(), sp.box6)
    assert a.shape == (2, 7, 3) and bool(a.all()) and torch.equal(a, b)


@pytest.mark.parametrize("cols", [(2,), (4,)])
def test_far_reduction_of_a_band_that_is_not_16_byte_aligned(cols):
    """a contiguous view one complex64 into its storage: the cells are read with 8-byte loads, the sums are the same"""
    import torch_nfft_amd as tn
    sp = _splitting(dv.far_alpha(8), 0.25, 8, eb.T)
    shape = (2, 8, 8, 8) + cols
    buf = torch.randn(1 + math.prod(shape), dtype=torch.complex64, device="cuda")
    band = buf[1:].view(shape)
    assert band.is_contiguous() and band.data_ptr() % 16 == 8
    aligned = band.clone()
    assert aligned.data_ptr() % 16 == 0
    a = tn.ops.nfft_ewald_dispersion_virial_far(band, sp.coeffs, sp.strain_coeffs(), sp.box6)
    b = tn.ops.nfft_ewald_dispersion_virial_far(aligned, sp.coeffs, sp.strain_coeffs(), sp.box6)
    tn.ops.check_status()
    assert bool(a.all()) and torch.equal(a, b)


def test_no_points_and_refusals():
    import torch_nfft_amd as tn
    pos = torch.zeros(0, 3, device="cuda")
    out = tn.ops.nfft_ewald_dispersion_virial_near(pos, torch.zeros(0, 2, device="cuda"), None, _six(eb.T), 5.0, 0.3)
    assert out.shape == (1, 7, 2) and out.dtype == torch.float64 and not bool(out.any())
    out = tn.ops.nfft_ewald_dispersion_virial_near(pos, torch.zeros(0, device="cuda"), None, _six(eb.T), 5.0, 0.3)
    assert out.shape == (1, 7) and not bool(out.any())
    sp = _splitting(6.0, 0.25, 16, eb.T)
    U, W = tn.nfft_ewald_dispersion_virial(torch.zeros(0, 2, device="cuda"), pos, splitting=sp)
    assert U.shape == (1, 2) and W.shape == (1, 3, 3, 2) and U.dtype == W.dtype == torch.float32
    assert not bool(U.any()) and not bool(W.any())
    with pytest.raises(RuntimeError, match="Input mismatch"):
        tn.ops.nfft_ewald_dispersion_virial_near(torch.zeros(4, 3, device="cuda"), torch.zeros(4, dtype=torch.complex64, device="cuda"),
                                                 None, _six(eb.T), 5.0, 0.3)
    with pytest.raises(RuntimeError, match="Input mismatch"):
        tn.ops.nfft_ewald_dispersion_virial_near(torch.zeros(4, 3, device="cuda"), torch.zeros(4, device="cuda"), None, _six(eb.T),
                                                 5.0, 0.31)
    band = torch.zeros(1, 16, 16, 16, dtype=torch.complex64, device="cuda")
    with pytest.raises(RuntimeError, match="Input mismatch"):
        tn.ops.nfft_ewald_dispersion_virial_far(band, sp.coeffs, sp.strain_coeffs()[:8], sp.box6)
    with pytest.raises(RuntimeError, match="Input mismatch"):
        tn.ops.nfft_ewald_dispersion_virial_far(band, sp.coeffs, sp.strain_coeffs().double(), sp.box6)


# The cases of tests/test_gpu_ewald_virial.py.  N = 6: 216 cells, not a multiple of any block size, one workgroup with idle
# lanes; 32: 128 workgroups per point set; 64: 1024 workgroups of 256, one cell per thread exactly.  72 and 80: more cells
# than the 262144 threads of a point set, so 42 % and 95 % of the threads take a second cell and the index is advanced by
# the stride, whose three digits in base N are all non-zero there (50, 40, 64 and 40, 76, 64): both carries happen.
# alpha = 0.8 N throughout (dv.far_alpha), so that b_k and t_k count out to the grid's edge.  Columns: one, two and four take
# whole cells in one or two loads, three has a masked tail, five runs the four-column pass twice.
FAR_CASES = [(N, name, cols) for N in (6, 8, 12, 32) for name in ("T", "O") for cols in ((), (3,))] + \
            [(8, "T", (2,)), (8, "T", (4,)), (8, "O", (5,)), (64, "T", ()),
             (72, "T", ()), (72, "O", (3,)), (80, "O", ()), (80, "T", (3,))]


@pytest.mark.parametrize("N,name,cols", FAR_CASES)
def test_far_reduction_against_dense_sum(N, name, cols):
    import torch_nfft_amd as tn
    A = BOXES[name]
    sp = _splitting(dv.far_alpha(N), 0.25, N, A)
    band = dv.far_band(N, name, cols)
    out = tn.ops.nfft_ewald_dispersion_virial_far(_cuda(band), sp.coeffs, sp.strain_coeffs(), sp.box6)
    tn.ops.check_status()
    assert out.shape == (2, 7) + cols and out.dtype == torch.float64
    # (the splitting's own float32 coefficients)
    ref = _seven(*dv.far_virial(band, sp.coeffs.cpu().numpy(), sp.strain_coeffs().cpu().numpy(), A))
    err = dv.rel_fro(out.cpu().numpy(), ref)
    print("dispersion virial far, N %d box %s cols %s: rel %.3e (|ref| %.3e)" % (N, name, cols, err, np.linalg.norm(ref)))
    assert np.linalg.norm(ref[:, 4:]) > 0
    assert err <= FAR_TOL


@pytest.fixture(scope="module")
def whole():
    """the 343 points of dv.whole_points in two point sets (a dense set: tests/test_gpu_dispersion.py::test_converged_sum says
    why a sparse one is no yardstick for the cancellation of the self term); per box the float64 algorithm and the
    converged sum"""
    s, c, batch = dv.whole_points()
    alpha, r_c, N = dv.WHOLE
    done = {}

    def get(name):
        if name not in done:
            done[name] = (dv.exact_algorithm_virial(c, s, BOXES[name], batch, alpha, r_c, N),
                          dv.converged_virial(c, s, BOXES[name], batch))
        return done[name]

    return s, c, batch, get


@pytest.mark.parametrize("name", ["T", "O"])
def test_whole_virial(whole, name):
    import torch_nfft_amd as tn
    s, c, batch, get = whole
    (Ua, Wa), (Uc, Wc) = get(name)
    alpha, r_c, N = dv.WHOLE
    sp = _splitting(alpha, r_c, N, BOXES[name])
    cd, sd, bd = _cuda(c), _cuda(s), _cuda(batch)
    U, W = tn.nfft_ewald_dispersion_virial(cd, sd, bd, splitting=sp, cutoff=4, fractional=True)
    energy = tn.nfft_ewald_dispersion_energy(cd, sd, bd, splitting=sp, cutoff=4, fractional=True)
    tn.ops.check_status()
    assert U.shape == (2,) and W.shape == (2, 3, 3) and U.dtype == W.dtype == torch.float32
    assert torch.equal(W, W.transpose(1, 2))
    U, W, energy = U.cpu().numpy(), W.cpu().numpy(), energy.cpu().numpy()
    for what, got, alg, conv in (("W", W, Wa, Wc), ("U", U, Ua, Uc)):
        e_alg, e_own, e_conv = dv.rel_fro(got, alg), dv.rel_fro(alg, conv), dv.rel_fro(got, conv)
        print("nfft_ewald_dispersion_virial, box %s, %s: rel vs the float64 algorithm %.3e, vs the converged sum %.3e (the "
              "algorithm's own %.3e)" % (name, what, e_alg, e_conv, e_own))
        assert e_alg <= WHOLE_TOL[what]
        # the triangle inequality |got - conv| <= |got - alg| + |alg - conv| with the tolerance in place of the first term
        assert np.linalg.norm(got - conv) <= WHOLE_TOL[what] * np.linalg.norm(alg) + np.linalg.norm(alg - conv)
    e_energy = dv.rel_fro(U, energy)
    print("nfft_ewald_dispersion_virial, box %s: U vs nfft_ewald_dispersion_energy %.3e (%s, %s)" % (name, e_energy, U, energy))
    assert e_energy <= WHOLE_TOL["energy"]
    # tr W = 6 U for the converged sum (to 1e-13 of U there): the device's two differ by no more than their two measured
    # errors against it (|tr E| <= sqrt(3) |E|_F)
    for b in (0, 1):
        assert abs(np.trace(Wc[b]) - 6.0 * Uc[b]) <= 1e-12 * abs(Uc[b])
        bound = math.sqrt(3.0) * np.linalg.norm(W[b] - Wc[b]) + 6.0 * abs(U[b] - Uc[b]) + 1e-12 * abs(Uc[b])
        print("set %d: tr W - 6 U = %.3e, bound %.3e (U = %.7g)" % (b, np.trace(W[b].astype(np.float64)) - 6.0 * U[b], bound, U[b]))
        assert abs(np.trace(W[b].astype(np.float64)) - 6.0 * U[b]) <= bound


@pytest.fixture(scope="module")
def small():
    """the same 343 points in the box T with two columns: float32 fractional positions s0, their float32 Cartesian positions
    x = s0 A (float64 product, rounded once), the fractional positions sx that those stand for, and the float64 algorithm on
    s0 in T and in the unit cube"""
    s0, c, batch = dv.whole_points()
    c2 = np.stack([c, c[::-1] * c], 1)
    x = (s0.astype(np.float64) @ eb.T).astype(np.float32)
    alpha, r_c, N = dv.WHOLE
    return x, s0, c2, batch, dv.exact_algorithm_virial(c2, s0, eb.T, batch, alpha, r_c, N), \
        dv.exact_algorithm_virial(c2, s0, np.eye(3), batch, alpha, r_c, N)


def test_cartesian_input_columns_and_box_gradient(small):
    import torch_nfft_amd as tn
    x, s0, c, batch, (Ua, Wa), _ = small
    alpha, r_c, N = dv.WHOLE
    sp = _splitting(alpha, r_c, N, eb.T)
    Ux, Wx = tn.nfft_ewald_dispersion_virial(_cuda(c), _cuda(x), _cuda(batch), splitting=sp)
    Us, Ws = tn.nfft_ewald_dispersion_virial(_cuda(c), _cuda(s0), _cuda(batch), splitting=sp, fractional=True)
    tn.ops.check_status()
    assert Ux.shape == (2, 2) and Wx.shape == (2, 3, 3, 2)
    assert torch.equal(Ws, Ws.transpose(1, 2))
    e_U, e_W = dv.rel_fro(Ux.cpu().numpy(), Us.cpu().numpy()), dv.rel_fro(Wx.cpu().numpy(), Ws.cpu().numpy())
    a_U, a_W = dv.rel_fro(Us.cpu().numpy(), Ua), dv.rel_fro(Ws.cpu().numpy(), Wa)
    print("Cartesian input: U %.3e W %.3e vs fractional input; fractional vs float64: U %.3e W %.3e" % (e_U, e_W, a_U, a_W))
    assert max(e_U, e_W) <= WHOLE_TOL["cartesian"]
    assert a_U <= WHOLE_TOL["U"] and a_W <= WHOLE_TOL["W"]
    # the gradient in the box entries, through the public helper on the device, unchanged
    G = tn.virial_to_box_gradient(Ws, sp.box)
    want = -np.einsum("ki,bkjc->bijc", np.linalg.inv(eb.T), Wa) * np.tril(np.ones((3, 3)))[None, :, :, None]
    assert G.shape == (2, 3, 3, 2) and G.is_cuda
    # |tril(A^-T E)|_F <= |A^-1|_2 |E|_F for the error E of W, plus the float32 rounding of the product itself
    scale = np.linalg.norm(np.linalg.inv(eb.T), 2) * np.linalg.norm(Wa)
    assert np.linalg.norm(G.cpu().numpy() - want) <= (WHOLE_TOL["W"] + 4 * 2.0 ** -24) * scale


def test_box_none_is_the_identity_box(small):
    import torch_nfft_amd as tn
    _, s0, c, batch, _, (Ua, Wa) = small
    alpha, r_c, N = dv.WHOLE
    cube, ident = _splitting(alpha, r_c, N, None), _splitting(alpha, r_c, N, np.eye(3))
    Uc, Wc = tn.nfft_ewald_dispersion_virial(_cuda(c), _cuda(s0), _cuda(batch), splitting=cube)
    Ui, Wi = tn.nfft_ewald_dispersion_virial(_cuda(c), _cuda(s0), _cuda(batch), splitting=ident, fractional=True)
    tn.ops.check_status()
    e_U, e_W = dv.rel_fro(Uc.cpu().numpy(), Ui.cpu().numpy()), dv.rel_fro(Wc.cpu().numpy(), Wi.cpu().numpy())
    a_U, a_W = dv.rel_fro(Uc.cpu().numpy(), Ua), dv.rel_fro(Wc.cpu().numpy(), Wa)
    print("box=None vs the identity box: U %.3e W %.3e; box=None vs float64: U %.3e W %.3e" % (e_U, e_W, a_U, a_W))
    assert e_U <= 2 * WHOLE_TOL["U"] and e_W <= 2 * WHOLE_TOL["W"]
    assert a_U <= WHOLE_TOL["U"] and a_W <= WHOLE_TOL["W"]


def test_refusals_and_autograd(small):
    import torch_nfft_amd as tn
    x, s0, c, batch, _, _ = small
    sp = _splitting(*dv.WHOLE, eb.T)
    cd, xd, bd = _cuda(c), _cuda(x), _cuda(batch)
    with pytest.raises(ValueError, match="real"):
        tn.nfft_ewald_dispersion_virial(cd.to(torch.complex64), xd, bd, splitting=sp)
    with pytest.raises(AssertionError, match="batch"):
        tn.nfft_ewald_dispersion_virial(cd, xd, torch.zeros(343, device="cuda", requires_grad=True), splitting=sp)
    with pytest.raises(ValueError, match="fractional"):
        tn.nfft_ewald_dispersion_virial(cd, xd, bd, splitting=_splitting(6.0, 0.25, 16, None), fractional=True)
    with pytest.raises(TypeError, match="DispersionSplitting"):
        tn.nfft_ewald_dispersion_virial(cd, xd, bd, splitting=tn.EwaldSplitting(6.0, 0.25, 16, box=eb.T))
    # inputs that require grad are accepted; the outputs are constants to autograd
    U, W = tn.nfft_ewald_dispersion_virial(cd.clone().requires_grad_(True), xd.clone().requires_grad_(True), bd, splitting=sp)
    assert not U.requires_grad and not W.requires_grad and U.grad_fn is None and W.grad_fn is None
    U0, W0 = tn.nfft_ewald_dispersion_virial(cd, xd, bd, splitting=sp)
    assert dv.rel_fro(U.cpu().numpy(), U0.cpu().numpy()) <= 2 * WHOLE_TOL["U"]
    assert dv.rel_fro(W.cpu().numpy(), W0.cpu().numpy()) <= 2 * WHOLE_TOL["W"]
