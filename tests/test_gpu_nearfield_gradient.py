"""GPU tests of the gradient pair kernel (csrc/nearfield_grad.hip), of its transpose and of
nfft_fastsum_nearfield_gradient against the float64 restatement tests/nearfield_gradient_ref.py.

Tolerances.  The device evaluates (K' - T_I') / r in float32, the restatement in float64 with the
same a_k.  GRAD_TOL is 4x the largest rel_l2 seen per kernel on the first device run, over every test that prints one (the
figure behind each entry is in its comment); as for the value sum, r^2 log r, which T_I follows closely, loses the most
digits to the subtraction K'/r - T_I'/r, and no figure is more than 1.2x its value-sum figure in test_gpu_nearfield.py's
NEAR_TOL.  A missed neighbour cell, tile or item shows as an error of 1e-2 .. 1 on these shapes, so no entry may reach
1e-3; a missed pair at r ~ eps_I is invisible and harmless, K' - T_I' vanishes there to order p - 1.  WHOLE_GRAD_TOL is
the same for the whole gradient and its transpose against the float64 algorithm; the stronger check there is
e_dense <= 1.1 e_own.
"""
import numpy as np
import pytest
import torch

import nearfield_gradient_ref as ng
import nearfield_ref as nr
from conftest import rel_l2

pytestmark = pytest.mark.gpu

GRAD_TOL = {  # 4 x the largest rel_l2 of the first device run (in brackets)
    "one_over_modulus": 4.6e-6,      # (1.130e-6: the crowded cell; 1.6e-8 .. 1.4e-7 elsewhere)
    "one_over_square": 5.1e-7,       # (1.260e-7)
    "logarithm": 6.6e-7,             # (1.627e-7)
    "thinplate_spline": 9.3e-6,      # (2.317e-6: T_I' follows K' closely, |K' - T_I'| is 1/19 of |K'| + |T_I'|)
    "multiquadric": 2.3e-6,          # (5.722e-7)
    "inverse_multiquadric": 1.2e-6,  # (2.834e-7)
    "gaussian": 8.8e-7,              # (2.199e-7)
    "laplacian_rbf": 1.2e-6,         # (2.830e-7)
}
WHOLE_GRAD_TOL = 7.9e-6  # (1.952e-6: the multiquadric's gradient in x; 2.3e-7 .. 1.6e-6 for the other whole gradients)


def test_no_tolerance_hides_a_missed_cell():
    assert max(GRAD_TOL.values()) < 1e-3 and WHOLE_GRAD_TOL < 1e-3 and set(GRAD_TOL) == set(nr.NAMES)


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


def _values(rng, shape, complex_x):
    x = rng.standard_normal(shape)
    if complex_x:
        return (x + 1j * rng.standard_normal(shape)).astype(np.complex64)
    return x.astype(np.float32)


def _op(kern, x, s, t, sb, tb, transpose):
    """the operator itself: both modes"""
    import torch_nfft_amd as tn
    s_, sb_ = _cuda(s), _cuda(sb)
    t_, tb_ = (s_, sb_) if t is None else (_cuda(t), _cuda(tb))
    z = tn.ops.nfft_nearfield_gradient(s_, t_, _cuda(x), sb_, tb_, kern.kernel_id, kern.c, kern.eps_I,
                                       kern.near_gradient_poly.tolist(), transpose)
    tn.ops.check_status()
    return z


def _ref(kern, x, s, t, sb, tb, transpose):
    fn = ng.near_gradient_transpose if transpose else ng.near_gradient
    return fn(kern.name, kern.c, kern.near_poly.numpy(), kern.eps_I, x, s, t, sb, tb)


def _check_both_modes(label, kern, rng, x, s, t, sb, tb, complex_x):
    """gradient of x and transpose of a random v against brute force; returns the two device results"""
    nt = len(s) if t is None else len(t)
    v = _values(rng, (nt, s.shape[1]) + x.shape[1:], complex_x)
    out = []
    for transpose, arg in ((False, x), (True, v)):
        z = _op(kern, arg, s, t, sb, tb, transpose)
        ref = _ref(kern, arg, s, t, sb, tb, transpose)
        assert z.shape == ref.shape and z.dtype == (torch.complex64 if complex_x else torch.float32)
        err = rel_l2(z.cpu().numpy(), ref)
        print("near gradient %s %s%s: rel_l2 %.3e (|ref| %.3e)" % (label, kern.name, " transpose" if transpose else "", err,
                                                                   np.linalg.norm(ref)))
        assert np.linalg.norm(ref) > 0
        assert err <= GRAD_TOL[kern.name]
        out.append(z)
    return out


# dim, N, kernel, c, p, eps_I (cells per axis = floor(1 / (2 eps_I)): 7 and 11), shared, ragged, cols, complex.
# Real columns 1, 2, 3, 4 (CC = 1, 2, 4, 4) and 5, 6 (a second column pass); p - 1 <= 4 terms (PT = 4) and 5, 7 (PT = 8).
CASES = [
    (1, 16, "one_over_modulus", 1.0, 4, 0.07, False, False, (), False),
    (2, 16, "logarithm", 1.0, 4, 0.07, True, True, (3,), False),
    (3, 16, "one_over_square", 1.0, 2, 0.07, False, True, (2,), True),
    (3, 32, "one_over_modulus", 1.0, 4, 0.045, True, False, (), False),
    (2, 32, "thinplate_spline", 1.0, 6, 0.045, False, False, (3,), True),
    (3, 32, "multiquadric", 0.01, 5, 0.045, True, True, (5,), False),
    (1, 32, "inverse_multiquadric", 0.01, 8, 0.045, False, True, (2,), True),
    (2, 16, "gaussian", 0.02, 3, 0.07, True, False, (2,), False),
    (3, 16, "laplacian_rbf", 0.02, 5, 0.07, False, False, (2,), False),
]


@pytest.mark.parametrize("dim,N,name,c,p,eps_I,shared,ragged,cols,complex_x", CASES)
def test_near_gradient_against_brute_force(dim, N, name, c, p, eps_I, shared, ragged, cols, complex_x):
    rng = np.random.default_rng(dim * 1000 + N + p)
    kern = _kernel(name, c, dim, N, p, eps_I)
    ns, nt = 700, 500
    s = nr.ball_points(rng, ns, dim, kern.max_radius)
    x = _values(rng, (ns,) + cols, complex_x)
    sb = _ragged_batch(rng, ns) if ragged else None
    if shared:
        s[40:60] = s[0:20]  # exact duplicates: the r = 0 pairs (within one point set for the first of them at least)
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
    G, _ = _check_both_modes("d=%d N=%d p=%d" % (dim, N, p), kern, rng, x, s, t, sb, tb, complex_x)
    assert bool(torch.isfinite(torch.view_as_real(G) if complex_x else G).all())
    if not shared and ragged:
        assert bool((G[_cuda(tb == 1)] == 0).all()) and (tb == 1).sum() > 50


@pytest.fixture(scope="module")
def crowded():
    """3000 sources and 600 targets inside the centre cell of a 7^3 grid: twelve LDS tiles, five items of that cell (and,
    transposed, three tiles and twenty-four items)"""
    rng = np.random.default_rng(5)
    kern = _kernel("one_over_modulus", 1.0, 3, 16, 4, 0.07)
    s = (rng.random((3000, 3)) * 0.06 - 0.03).astype(np.float32)
    t = (rng.random((600, 3)) * 0.06 - 0.03).astype(np.float32)
    t[:50] = s[:50]
    return kern, _values(rng, (3000,), False), s, t


def test_one_crowded_cell(crowded):
    kern, x, s, t = crowded
    _check_both_modes("crowded cell", kern, np.random.default_rng(50), x, s, t, None, None, False)


def test_two_calls_are_bitwise_equal(crowded):
    kern, x, s, t = crowded
    v = _values(np.random.default_rng(51), (600, 3), False)
    assert torch.equal(_op(kern, x, s, t, None, None, False), _op(kern, x, s, t, None, None, False))
    assert torch.equal(_op(kern, v, s, t, None, None, True), _op(kern, v, s, t, None, None, True))
    rng = np.random.default_rng(6)
    kern = _kernel("logarithm", 1.0, 3, 32, 4, 0.045)
    pts = nr.ball_points(rng, 5000, 3, kern.max_radius)
    b = _ragged_batch(rng, 5000)
    xc, vc = _values(rng, (5000, 3), True), _values(rng, (5000, 3, 3), True)
    assert torch.equal(_op(kern, xc, pts, None, b, None, False), _op(kern, xc, pts, None, b, None, False))
    assert torch.equal(_op(kern, vc, pts, None, b, None, True), _op(kern, vc, pts, None, b, None, True))


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
    x = _values(rng, (len(s), 2), False)
    _check_both_modes("cell faces", kern, rng, x, s, t.astype(np.float32), None, None, False)


def test_targets_without_a_source_in_range_get_exact_zeros():
    rng = np.random.default_rng(8)
    kern = _kernel("one_over_square", 1.0, 2, 16, 4, 0.07)
    s = (rng.random((400, 2)) * 0.05 - 0.2).astype(np.float32)  # in [-0.2, -0.15]^2
    far = (rng.random((200, 2)) * 0.3 - 0.05).astype(np.float32)  # >= 0.1 away
    ring = s[:200] + (np.float32(0.125) * np.stack([np.cos(np.arange(200.0)), np.sin(np.arange(200.0))], -1)).astype(np.float32)
    ring = ring[np.linalg.norm(ring[:, None].astype(np.float64) - s[None].astype(np.float64), axis=-1).min(1) > 0.0701]
    assert len(ring) > 20  # targets in neighbouring cells of sources, yet farther than eps_I from every one of them
    t = np.concatenate([far, ring]).astype(np.float32)
    z = _op(kern, _values(rng, (400, 3), False), s, t, None, None, False)
    assert z.shape == (len(t), 2, 3) and bool((z == 0).all())
    zt = _op(kern, _values(rng, (len(t), 2, 3), False), s, t, None, None, True)
    assert zt.shape == (400, 3) and bool((zt == 0).all())


@pytest.mark.parametrize("ns,nt,cols", [(0, 7, (2,)), (9, 0, (2,)), (9, 7, (0,)), (0, 0, ())])
def test_empty_sides_and_no_columns(ns, nt, cols):
    import torch_nfft_amd as tn
    kern = _kernel("one_over_modulus", 1.0, 3, 16, 4, 0.07)
    rng = np.random.default_rng(9)
    s, t = nr.ball_points(rng, ns, 3, 0.2), nr.ball_points(rng, nt, 3, 0.2)
    for complex_x in (False, True):
        dtype = torch.complex64 if complex_x else torch.float32
        z = tn.nfft_nearfield_gradient(_cuda(_values(rng, (ns,) + cols, complex_x)), kern, _cuda(s), _cuda(t))
        assert z.shape == (nt, 3) + cols and z.dtype == dtype and bool((z == 0).all())
        zt = _op(kern, _values(rng, (nt, 3) + cols, complex_x), s, t, None, None, True)
        assert zt.shape == (ns,) + cols and zt.dtype == dtype and bool((zt == 0).all())
        tn.ops.check_status()


@pytest.mark.parametrize("complex_x", [False, True])
def test_transpose_is_the_backward(complex_x):
    import torch_nfft_amd as tn
    rng = np.random.default_rng(31)
    kern = _kernel("one_over_modulus", 1.0, 3, 32, 4, None)
    s, t = nr.ball_points(rng, 700, 3, kern.max_radius), nr.ball_points(rng, 500, 3, kern.max_radius)
    t[:20] = s[:20]
    x, v = _values(rng, (700, 2), complex_x), _values(rng, (500, 3, 2), complex_x)
    xs, ss, ts = _cuda(x).requires_grad_(True), _cuda(s), _cuda(t)
    vs = _cuda(v).requires_grad_(True)
    G = tn.nfft_nearfield_gradient(xs, kern, ss, ts)
    g, = torch.autograd.grad(G, xs, vs, create_graph=True)
    Gt = _op(kern, v, s, t, None, None, True)
    assert torch.equal(g, Gt)  # the backward IS the transposed call
    probe = _cuda(_values(rng, (700, 2), complex_x))
    gg, = torch.autograd.grad(g, vs, probe)  # d<probe, G^T v>/dv = G probe: the gradient call on the probe
    assert torch.equal(gg, _op(kern, probe.cpu().numpy(), s, t, None, None, False))
    Gd, vd, xd = G.detach().to(torch.complex128), vs.detach().to(torch.complex128), xs.detach().to(torch.complex128)
    lhs, rhs = complex((Gd * vd).sum()), complex((xd * Gt.to(torch.complex128)).sum())  # (bilinear: the matrix is real)
    # each side is off by at most its tolerance times the norms of its two factors
    scale = float(torch.linalg.vector_norm(Gd) * torch.linalg.vector_norm(vd) +
                  torch.linalg.vector_norm(xd) * torch.linalg.vector_norm(Gt))
    print("adjointness (complex %s): |<Gx, v> - <x, G^T v>| / (|Gx| |v| + |x| |G^T v|) = %.3e" % (complex_x, abs(lhs - rhs) / scale))
    assert abs(lhs - rhs) <= GRAD_TOL[kern.name] * scale
    tn.ops.check_status()


# name, c, dim, separate targets, point sets: the problems of test_gpu_nearfield.py's WHOLE
WHOLE = [("one_over_modulus", 1.0, 3, False, 1), ("logarithm", 1.0, 3, True, 2), ("multiquadric", 0.05, 2, False, 1)]


@pytest.fixture(scope="module", params=WHOLE, ids=[w[0] for w in WHOLE])
def whole(request):
    """N = 32, p = 4, 800 points: the problem, the float64 algorithm's gradient, the dense float64 gradient and the
    float64 algorithm's transpose applied to v"""
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
    x = _values(rng, (800,), False)
    v = _values(rng, (600 if separate else 800, dim), False)
    return (kern, x, v, s, t, sb, tb, ng.exact_algorithm_gradient(ref, N, x, s, t, sb, tb),
            ng.dense_gradient(name, c, x, s, t, sb, tb), ng.exact_algorithm_gradient_transpose(ref, N, v, s, t, sb, tb))


def test_whole_gradient(whole):
    import torch_nfft_amd as tn
    kern, x, v, s, t, sb, tb, alg, dense, alg_t = whole
    xs = _cuda(x).requires_grad_(True)
    G = tn.nfft_fastsum_nearfield_gradient(xs, kern, _cuda(s), _cuda(t), _cuda(sb), _cuda(tb), cutoff=4)
    tn.ops.check_status()
    assert G.dtype == torch.float32 and G.shape == alg.shape
    g, = torch.autograd.grad(G, xs, _cuda(v))
    assert g.dtype == torch.float32 and g.shape == xs.shape
    G = G.detach().cpu().numpy()
    e_alg, e_own, e_dense, e_t = rel_l2(G, alg), rel_l2(alg, dense), rel_l2(G, dense), rel_l2(g.cpu().numpy(), alg_t)
    print("whole gradient %s: vs float64 algorithm %.3e; vs dense %.3e (the algorithm's own error %.3e); gradient in x vs "
          "float64 transpose %.3e" % (kern.name, e_alg, e_dense, e_own, e_t))
    assert e_alg <= WHOLE_GRAD_TOL
    assert e_dense <= 1.1 * e_own
    assert e_t <= WHOLE_GRAD_TOL
    tn.ops.check_status()


def test_complex_values_against_the_float64_algorithm():
    """A complex x against the float64 algorithm on the same complex x, and its two parts against theirs.

    Axis a's coefficients lose the plane l_a = -N/2, not the planes l_b = -N/2 of the other axes, which carry
    (-2 pi i l_a) c_l like every other plane and, unpaired along b, a factor e^(-pi i N z_b) that is not real -- as in the
    value sum.  So for dim > 1 a complex x does NOT see the matrix of its real and imaginary parts: in float64 the two
    differ by 8.49e-5 (relative l2) on this problem, and by 2.43e-4 with the planes l_a = -N/2 kept.  (An earlier version
    of this test asked for agreement within 4e-5 and failed at 8.489e-5 on the device, the float64 figure.)  What holds is
    that each of the three device results is the float64 algorithm's, which tells the zeroed planes from the kept ones."""
    import torch_nfft_amd as tn
    rng = np.random.default_rng(33)
    kern = _kernel("logarithm", 1.0, 2, 32, 4, None, device="cuda")
    ref = nr.Restatement("logarithm", 1.0, 4, kern.eps_I, kern.eps_B)
    pts = nr.ball_points(rng, 600, 2, kern.max_radius)
    x = _values(rng, (600, 2), True)
    for label, arg in (("complex x", x), ("its real part", x.real.copy()), ("its imaginary part", x.imag.copy())):
        G = tn.nfft_fastsum_nearfield_gradient(_cuda(arg), kern, _cuda(pts), cutoff=4)
        assert G.dtype == (torch.complex64 if np.iscomplexobj(arg) else torch.float32) and G.shape == (600, 2, 2)
        err = rel_l2(G.cpu().numpy(), ng.exact_algorithm_gradient(ref, 32, arg, pts))
        print("whole gradient, %s against the float64 algorithm: rel_l2 %.3e" % (label, err))
        assert err <= WHOLE_GRAD_TOL
    tn.ops.check_status()


def test_refused_arguments():
    import torch_nfft_amd as tn
    rng = np.random.default_rng(32)
    kern = _kernel("logarithm", 1.0, 2, 32, 4, None, device="cuda")
    pts = _cuda(nr.ball_points(rng, 600, 2, kern.max_radius))
    x = _cuda(_values(rng, (600,), False)).requires_grad_(True)
    with pytest.raises(AssertionError, match="sources"):
        tn.nfft_fastsum_nearfield_gradient(x, kern, pts.clone().requires_grad_(True), cutoff=4)
    with pytest.raises(AssertionError, match="targets"):
        tn.nfft_nearfield_gradient(x, kern, pts, pts.clone().requires_grad_(True))
    with pytest.raises(AssertionError, match="source_batch"):
        tn.nfft_nearfield_gradient(x, kern, pts, None, torch.zeros(600, device="cuda", requires_grad=True))
    with pytest.raises(ValueError, match="p >= 2"):
        tn.nfft_fastsum_nearfield_gradient(x, _kernel("logarithm", 1.0, 2, 32, 1, None, device="cuda"), pts)
    with pytest.raises(RuntimeError, match="Input mismatch"):  # the transpose takes [n_t, dim, *cols]
        tn.ops.nfft_nearfield_gradient(pts, pts, x.detach(), None, None, kern.kernel_id, kern.c, kern.eps_I,
                                       kern.near_gradient_poly.tolist(), True)
    tn.ops.check_status()
