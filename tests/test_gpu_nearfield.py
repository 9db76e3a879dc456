"""GPU tests of the near-field pair sum (csrc/nearfield.hip) and of nfft_fastsum_nearfield against the float64
restatement tests/nearfield_ref.py.

Tolerances.  The device evaluates K - T_I in float32, the restatement in float64 with the same a_k.
NEAR_TOL is 4x the largest rel_l2 seen per kernel on the first device run (the figure behind each entry is in its comment);
kernels that T_I approximates well (K - T_I small against K) lose more digits to the subtraction than the singular ones.  A
missed neighbour cell shows as an error of 1e-2 .. 1 on these shapes; a missed pair at r ~ eps_I is invisible and harmless,
K - T_I vanishes there to order p.  WHOLE_TOL is the same for the whole sum against the float64 algorithm.
"""
import numpy as np
import pytest
import torch

import nearfield_ref as nr
from conftest import rel_l2

pytestmark = pytest.mark.gpu

NEAR_TOL = {  # 4 x the largest rel_l2 of the first device run (in brackets)
    "one_over_modulus": 3.9e-6,      # (9.65e-7: the crowded cell; 4.5e-8 .. 2.6e-7 elsewhere)
    "one_over_square": 5.4e-7,       # (1.34e-7)
    "logarithm": 1.5e-6,             # (3.75e-7)
    "thinplate_spline": 3.2e-5,      # (8.03e-6: T_I follows r^2 log r closely, the difference is 1e-2 of its terms)
    "multiquadric": 1.9e-6,          # (4.86e-7)
    "inverse_multiquadric": 1.0e-6,  # (2.61e-7)
    "gaussian": 8.5e-7,              # (2.12e-7)
    "laplacian_rbf": 1.7e-6,         # (4.29e-7)
}
WHOLE_TOL = 2.2e-6  # (5.41e-7: the 1/r sum; 2.5e-7 .. 4.3e-7 for the other sums and the gradients, coefficients 1.0e-7)

def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _kernel(name, c, dim, N, p, eps_I, device="cpu"):
    import torch_nfft_amd as tn
    return tn.RegularizedKernel(name, c=c, dim=dim, bandwidth=N, p=p, eps_I=eps_I, device=device)


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


def _near(kern, x, s, t=None, sb=None, tb=None):
    import torch_nfft_amd as tn
    z = tn.nfft_nearfield(_cuda(x), kern, _cuda(s), _cuda(t), _cuda(sb), _cuda(tb))
    tn.ops.check_status()
    return z


def _near_ref(kern, x, s, t=None, sb=None, tb=None):
    return nr.near_sum(kern.name, kern.c, kern.near_poly.numpy(), kern.eps_I, x, s, t, sb, tb)


# dim, N, kernel, c, p, eps_I (cells per axis = floor(1 / (2 eps_I)), never a divisor of anything), shared, ragged, cols, complex
CASES = [
    (1, 16, "one_over_modulus", 1.0, 4, 0.07, False, False, (), False),
    (2, 16, "logarithm", 1.0, 4, 0.07, True, True, (3,), False),
    (3, 16, "one_over_square", 1.0, 2, 0.07, False, True, (2,), True),
    (3, 32, "one_over_modulus", 1.0, 4, 0.045, True, False, (), False),
    (2, 32, "thinplate_spline", 1.0, 6, 0.045, False, False, (3,), True),
    (3, 32, "multiquadric", 0.01, 4, 0.045, True, True, (3,), False),
    (1, 32, "inverse_multiquadric", 0.01, 8, 0.045, False, True, (2,), True),
    (2, 16, "gaussian", 0.02, 3, 0.07, True, False, (), False),
    (3, 16, "laplacian_rbf", 0.02, 5, 0.07, False, False, (2,), False),
    (3, 16, "logarithm", 1.0, 1, 0.07, False, False, (5,), False),
]


@pytest.mark.parametrize("dim,N,name,c,p,eps_I,shared,ragged,cols,complex_x", CASES)
def test_near_field_against_brute_force(dim, N, name, c, p, eps_I, shared, ragged, cols, complex_x):
    rng = np.random.default_rng(dim * 1000 + N + p)
    kern = _kernel(name, c, dim, N, p, eps_I)
    ns, nt = 700, 500
    s = nr.ball_points(rng, ns, dim, kern.max_radius)
    x = _values(rng, ns, cols, complex_x)
    sb = _ragged_batch(rng, ns) if ragged else None
    if shared:
        s[40:60] = s[0:20]  # exact duplicates: the r = 0 branch (within one point set for the first of them at least)
        if sb is not None:
            sb[40:60] = sb[0:20]
            order = np.argsort(sb, kind="stable")
            s, x, sb = s[order], x[order], sb[order]
        t, tb = None, None
    else:
        t = nr.ball_points(rng, nt, dim, kern.max_radius)
        t[0:25] = s[0:25]
        tb = None
        if ragged:  # the sources' middle set is empty, the targets' is not: those targets meet nothing
            tb = np.sort(rng.integers(0, 3, nt)).astype(np.int64)
            tb[0], tb[-1] = 0, 2
    z = _near(kern, x, s, t, sb, tb)
    ref = _near_ref(kern, x, s, t, sb, tb)
    assert z.shape == ref.shape and z.dtype == (torch.complex64 if complex_x else torch.float32)
    err = rel_l2(z.cpu().numpy(), ref)
    print("near field %s d=%d N=%d p=%d: rel_l2 %.3e (|ref| %.3e)" % (name, dim, N, p, err, np.linalg.norm(ref)))
    assert np.linalg.norm(ref) > 0
    if not shared and ragged:
        assert bool((z[_cuda(tb == 1)] == 0).all()) and (tb == 1).sum() > 50
    assert err <= NEAR_TOL[name]


@pytest.fixture(scope="module")
def crowded():
    """3000 sources and 600 targets inside the centre cell of a 7^3 grid: twelve LDS tiles, five items of that cell"""
    rng = np.random.default_rng(5)
    kern = _kernel("one_over_modulus", 1.0, 3, 16, 4, 0.07)
    s = (rng.random((3000, 3)) * 0.06 - 0.03).astype(np.float32)
    t = (rng.random((600, 3)) * 0.06 - 0.03).astype(np.float32)
    t[:50] = s[:50]
    x = _values(rng, 3000, (), False)
    return kern, x, s, t, _near_ref(kern, x, s, t)


def test_one_crowded_cell(crowded):
    kern, x, s, t, ref = crowded
    z = _near(kern, x, s, t)
    err = rel_l2(z.cpu().numpy(), ref)
    print("near field crowded cell: rel_l2 %.3e" % err)
    assert err <= NEAR_TOL[kern.name]


def test_two_calls_are_bitwise_equal(crowded):
    kern, x, s, t, _ = crowded
    assert torch.equal(_near(kern, x, s, t), _near(kern, x, s, t))
    rng = np.random.default_rng(6)
    kern = _kernel("logarithm", 1.0, 3, 32, 4, 0.045)
    pts = nr.ball_points(rng, 5000, 3, kern.max_radius)
    xc = _values(rng, 5000, (3,), True)
    b = _ragged_batch(rng, 5000)
    assert torch.equal(_near(kern, xc, pts, None, b, None), _near(kern, xc, pts, None, b, None))


def test_points_on_cell_faces_and_on_the_sphere():
    rng = np.random.default_rng(7)
    kern = _kernel("one_over_modulus", 1.0, 2, 16, 4, 0.07)
    G = 7
    faces = (np.arange(G + 1, dtype=np.float64) / (2 * G) - 0.25).astype(np.float32)
    lattice = np.stack(np.meshgrid(faces, faces, indexing="ij"), -1).reshape(-1, 2)
    ang = rng.random(100) * 2 * np.pi
    sphere = (np.stack([np.cos(ang), np.sin(ang)], -1) * kern.max_radius).astype(np.float32)
    near_faces = lattice[rng.integers(0, len(lattice), 200)] + (rng.standard_normal((200, 2)) * 1e-7).astype(np.float32)
    s = np.concatenate([lattice, sphere, near_faces, nr.ball_points(rng, 300, 2, kern.max_radius)]).astype(np.float32)
    t = np.concatenate([lattice, sphere[::-1], near_faces[:100] + np.float32(0.03), nr.ball_points(rng, 200, 2, 0.25)])
    x = _values(rng, len(s), (2,), False)
    z = _near(kern, x, s, t.astype(np.float32))
    ref = _near_ref(kern, x, s, t.astype(np.float32))
    err = rel_l2(z.cpu().numpy(), ref)
    print("near field cell faces: rel_l2 %.3e" % err)
    assert err <= NEAR_TOL[kern.name]


def test_targets_without_a_source_in_range_get_exact_zeros():
    rng = np.random.default_rng(8)
    kern = _kernel("one_over_square", 1.0, 2, 16, 4, 0.07)
    s = (rng.random((400, 2)) * 0.05 - 0.2).astype(np.float32)  # in [-0.2, -0.15]^2
    far = (rng.random((200, 2)) * 0.3 - 0.05).astype(np.float32)  # >= 0.1 away
    ring = s[:200] + (np.float32(0.125) * np.stack([np.cos(np.arange(200.0)), np.sin(np.arange(200.0))], -1)).astype(np.float32)
    ring = ring[np.linalg.norm(ring[:, None].astype(np.float64) - s[None].astype(np.float64), axis=-1).min(1) > 0.0701]
    assert len(ring) > 20  # targets in neighbouring cells of sources, yet farther than eps_I from every one of them
    t = np.concatenate([far, ring]).astype(np.float32)
    z = _near(kern, _values(rng, 400, (3,), False), s, t)
    assert z.shape == (len(t), 3) and bool((z == 0).all())


@pytest.mark.parametrize("ns,nt,cols", [(0, 7, (2,)), (9, 0, (2,)), (9, 7, (0,)), (0, 0, ())])
def test_empty_sides_and_no_columns(ns, nt, cols):
    import torch_nfft_amd as tn
    kern = _kernel("one_over_modulus", 1.0, 3, 16, 4, 0.07)
    rng = np.random.default_rng(9)
    s, t = nr.ball_points(rng, ns, 3, 0.2), nr.ball_points(rng, nt, 3, 0.2)
    for complex_x in (False, True):
        z = tn.nfft_nearfield(_cuda(_values(rng, ns, cols, complex_x)), kern, _cuda(s), _cuda(t))
        assert z.shape == (nt,) + cols and z.dtype == (torch.complex64 if complex_x else torch.float32)
        assert bool((z == 0).all())
        tn.ops.check_status()


def test_device_coefficients_match_the_restatement():
    kern = _kernel("one_over_modulus", 1.0, 3, 32, 4, None, device="cuda")
    ref = nr.Restatement("one_over_modulus", 1.0, 4, kern.eps_I, kern.eps_B)
    assert kern.coeffs.is_cuda and kern.coeffs.dtype == torch.float32 and kern.coeffs.shape == (32, 32, 32)
    err = rel_l2(kern.coeffs.cpu().numpy(), ref.coeffs(32, 3))
    print("device coeffs: rel_l2 %.3e" % err)
    assert err <= WHOLE_TOL


# name, c, dim, separate targets, point sets
WHOLE = [("one_over_modulus", 1.0, 3, False, 1), ("logarithm", 1.0, 3, True, 2), ("multiquadric", 0.05, 2, False, 1)]


@pytest.fixture(scope="module", params=WHOLE, ids=[w[0] for w in WHOLE])
def whole(request):
    """N = 32, p = 4, 800 points: the problem, the float64 algorithm's result and the dense float64 sum"""
    name, c, dim, separate, B = request.param
    rng = np.random.default_rng(21 + dim)
    N, p = 32, 4
    kern = _kernel(name, c, dim, N, p, None, device="cuda")
    ref = nr.Restatement(name, c, p, kern.eps_I, kern.eps_B)
    s = nr.ball_points(rng, 800, dim, kern.max_radius)
    t = nr.ball_points(rng, 600, dim, kern.max_radius) if separate else None
    sb = tb = None
    if B > 1:
        sb = np.sort(rng.integers(0, B, 800)).astype(np.int64)
        sb[0], sb[-1] = 0, B - 1
        tb = np.sort(rng.integers(0, B, 600)).astype(np.int64)
        tb[0], tb[-1] = 0, B - 1
    x = _values(rng, 800, (), False)
    return kern, ref, N, x, s, t, sb, tb, nr.exact_algorithm(ref, N, x, s, t, sb, tb), nr.dense_sum(name, c, x, s, t, sb, tb)


def test_whole_sum(whole):
    import torch_nfft_amd as tn
    kern, ref, N, x, s, t, sb, tb, alg, dense = whole
    y = tn.nfft_fastsum_nearfield(_cuda(x), kern, _cuda(s), _cuda(t), _cuda(sb), _cuda(tb), cutoff=4)
    tn.ops.check_status()
    assert y.dtype == torch.float32 and y.shape == alg.shape
    y = y.cpu().numpy()
    e_alg, e_own, e_dense = rel_l2(y, alg), rel_l2(alg, dense), rel_l2(y, dense)
    print("whole sum %s: vs float64 algorithm %.3e; vs dense %.3e (the algorithm's own error %.3e)" % (kern.name, e_alg, e_dense, e_own))
    assert e_alg <= WHOLE_TOL
    assert e_dense <= 1.1 * e_own


@pytest.mark.parametrize("complex_x", [False, True])
def test_gradient_in_x(complex_x):
    import torch_nfft_amd as tn
    rng = np.random.default_rng(31)
    kern = _kernel("one_over_modulus", 1.0, 3, 32, 4, None, device="cuda")
    ref = nr.Restatement("one_over_modulus", 1.0, 4, kern.eps_I, kern.eps_B)
    s, t = nr.ball_points(rng, 700, 3, kern.max_radius), nr.ball_points(rng, 500, 3, kern.max_radius)
    t[:20] = s[:20]
    x, dy = _values(rng, 700, (2,), complex_x), _values(rng, 500, (2,), complex_x)
    xs, ss, ts, dys = _cuda(x).requires_grad_(True), _cuda(s), _cuda(t), _cuda(dy)
    # the near field alone: its backward IS the swapped call
    gz, = torch.autograd.grad(tn.nfft_nearfield(xs, kern, ss, ts), xs, dys)
    assert torch.equal(gz, tn.nfft_nearfield(dys, kern, ts, ss))
    y = tn.nfft_fastsum_nearfield(xs, kern, ss, ts, cutoff=4)
    g, = torch.autograd.grad(y, xs, dys)
    assert g.dtype == xs.dtype and g.shape == xs.shape
    swapped = tn.nfft_fastsum_nearfield(dys, kern, ts, ss, cutoff=4)
    want = nr.exact_algorithm(ref, 32, dy, t, s)  # the transpose: sources and targets swapped, applied to dy
    e_swap, e_ref = rel_l2(g.cpu().numpy(), swapped.cpu().numpy()), rel_l2(g.cpu().numpy(), want)
    print("gradient in x (complex %s): vs swapped call %.3e, vs float64 %.3e" % (complex_x, e_swap, e_ref))
    assert e_swap <= WHOLE_TOL and e_ref <= WHOLE_TOL
    tn.ops.check_status()


def test_gradient_of_the_gradient_and_refused_arguments():
    import torch_nfft_amd as tn
    rng = np.random.default_rng(32)
    kern = _kernel("logarithm", 1.0, 2, 32, 4, None, device="cuda")
    pts = _cuda(nr.ball_points(rng, 600, 2, kern.max_radius))
    x = _cuda(_values(rng, 600, (), False)).requires_grad_(True)
    dy = _cuda(_values(rng, 600, (), False)).requires_grad_(True)
    v = _cuda(_values(rng, 600, (), False))
    z = tn.nfft_nearfield(x, kern, pts)  # (the far field, nfft_fastsum, differentiates once)
    g, = torch.autograd.grad(z, x, dy, create_graph=True)
    gg, = torch.autograd.grad(g, dy, v)  # d<v, W^T dy>/d dy = W v: the same call on v
    assert torch.equal(gg, tn.nfft_nearfield(v, kern, pts))
    with pytest.raises(AssertionError, match="sources"):
        tn.nfft_fastsum_nearfield(x, kern, pts.clone().requires_grad_(True), cutoff=4)
    with pytest.raises(AssertionError, match="targets"):
        tn.nfft_nearfield(x, kern, pts, pts.clone().requires_grad_(True))
    tn.ops.check_status()
