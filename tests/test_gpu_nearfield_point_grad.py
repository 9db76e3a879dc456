"""GPU tests of the contracting pair kernel (csrc/nearfield_pgrad.hip), of the operator
torch_nfft::_nfft_nearfield_point_gradient and of point_gradients=True in nfft_nearfield / nfft_fastsum_nearfield against
the float64 restatement tests/nearfield_point_grad_ref.py.

Shapes: N = 32 and eps_I = 1/8 give 4 cells per axis; 600 .. 800 points.

Tolerances.  The device evaluates (K' - T_I') / r in float32, the restatement in float64 with the
same a_k.  PGRAD_TOL is 4x the largest rel_l2 seen per kernel on the first device run, over every test that prints one
against the near restatement (the figure behind each entry is in its comment); none is more than 2.1x its section 7e
figure.  WHOLE_PGRAD_TOL is the same for sources.grad and targets.grad of nfft_fastsum_nearfield against the float64
algorithm (the far part with the unpaired planes l_a = -N/2 kept, as nfft_fastsum differentiates it).  It is 9x section
7e's figure, and the near kernel is not why: nfft_fastsum's own point gradients at cutoff m = 4 are 0.8e-5 .. 1.7e-5 from
the float64 trigonometric sum on these three problems (1.2e-5 .. 1.7e-5 where the far part is most of the gradient; with
m = 6, 0.3e-5 .. 1.2e-5) -- the differentiated window of section 7a, whose tests allow 2e-5 -- while the near part through
autograd is at 1.9e-7 .. 4.9e-7.  The stronger check there is e_dense <= 1.1 e_own.  x.grad is the value sum with the sides
swapped and keeps the tolerances of test_gpu_nearfield.py.  tests/test_nearfield_point_grad_ref.py holds the guard: on the
inputs of CASES, leaving one neighbour cell's pairs out of the restatement moves it by more than 10x the loosest tolerance.
"""
import numpy as np
import pytest
import torch

import nearfield_point_grad_ref as npg
import nearfield_ref as nr
from conftest import rel_l2
from test_gpu_fastsum_grad import T_ENTRY  # (the same arithmetic twice: only the order of the adjoint's atomics differs)
from test_gpu_nearfield import NEAR_TOL, WHOLE_TOL  # (x.grad is the value sum with the sides swapped)

pytestmark = pytest.mark.gpu

N, EPS_I, EPS_B, CELLS = 32, 0.125, 0.0625, 4

PGRAD_TOL = {  # 4 x the largest rel_l2 of the first device run (in brackets)
    "one_over_modulus": 3.0e-6,      # (7.375e-7: the crowded cell, shared; 1.1e-7 .. 3.6e-7 elsewhere)
    "one_over_square": 6.7e-7,       # (1.668e-7)
    "logarithm": 1.4e-6,             # (3.381e-7)
    "thinplate_spline": 1.4e-5,      # (3.454e-6: T_I' follows K' closely, as in section 7e)
    "multiquadric": 3.2e-6,          # (7.924e-7)
    "inverse_multiquadric": 1.3e-6,  # (3.083e-7)
    "gaussian": 1.3e-6,              # (3.190e-7)
    "laplacian_rbf": 1.1e-6,         # (2.660e-7)
}
WHOLE_PGRAD_TOL = 6.8e-5  # (1.694e-5: the 2-D multiquadric, the far part's error; 3-D log r 8.08e-6, 3-D 1/r 6.29e-7)


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _kernel(name, c, dim, p, device="cpu"):
    import torch_nfft_amd as tn
    return tn.RegularizedKernel(name, c=c, dim=dim, bandwidth=N, p=p, eps_I=EPS_I, eps_B=EPS_B, device=device)


def _values(rng, shape, complex_x):
    x = rng.standard_normal(shape)
    if complex_x:
        return (x + 1j * rng.standard_normal(shape)).astype(np.complex64)
    return x.astype(np.float32)


def _ragged_batch(rng, n):
    """three point sets, the middle one empty"""
    b = np.sort(rng.integers(0, 2, n)) * 2
    b[0], b[-1] = 0, 2
    return b.astype(np.int64)


# dim, kernel, c, p (2, 4: PT = 4; 8: PT = 8), trailing shape of x, complex, layout.  Real columns 1, 2, 3, 4 (CC = 1, 2, 4,
# 4), 5 and 10 (a second pass with a remainder), 9 (two full passes and a remainder).  Layouts: shared points (the
# symmetric sweep, and as a clone the two one-sided sweeps), separate targets with n_t != n_s, and both with a ragged batch
# of three point sets whose middle one is empty.
CASES = [
    (3, "one_over_modulus", 1.0, 4, (), False, "shared"),
    (3, "one_over_square", 1.0, 2, (2,), False, "separate"),
    (1, "logarithm", 1.0, 8, (3,), False, "ragged_shared"),
    (3, "thinplate_spline", 1.0, 4, (4,), False, "separate"),
    (2, "multiquadric", 0.01, 8, (5,), False, "shared"),
    (3, "inverse_multiquadric", 0.01, 2, (9,), False, "ragged_separate"),
    (1, "gaussian", 0.02, 4, (), True, "separate"),
    (2, "laplacian_rbf", 0.02, 4, (2,), True, "shared"),
    (3, "logarithm", 1.0, 4, (3, 3), False, "shared"),
    (3, "one_over_square", 1.0, 8, (5,), True, "ragged_shared"),
    (2, "one_over_modulus", 1.0, 2, (2,), False, "shared"),
    (2, "thinplate_spline", 1.0, 8, (), False, "ragged_separate"),
    (3, "gaussian", 0.02, 8, (2,), False, "shared"),
    (3, "laplacian_rbf", 0.02, 2, (3,), False, "separate"),
    (2, "inverse_multiquadric", 0.01, 4, (), False, "shared"),
    (1, "multiquadric", 0.01, 4, (4,), False, "separate"),
]


def case_inputs(case):
    """(kern, x, dy, s, t, sb, tb) in numpy; t is None for shared points.  Pure host code: the guard of
    tests/test_nearfield_point_grad_ref.py builds the same inputs without a GPU."""
    dim, name, c, p, cols, complex_x, layout = case
    rng = np.random.default_rng(dim * 1000 + p * 10 + len(name) + len(cols))
    kern = _kernel(name, c, dim, p)
    ns, nt = 700, 600
    ragged, shared = layout.startswith("ragged"), layout.endswith("shared")
    s = nr.ball_points(rng, ns, dim, kern.max_radius)
    x = _values(rng, (ns,) + cols, complex_x)
    sb = _ragged_batch(rng, ns) if ragged else None
    if shared:
        s[40:60] = s[0:20]  # exact duplicates: pairs with r = 0 and i != j
        if sb is not None:
            sb[40:60] = sb[0:20]
            order = np.argsort(sb, kind="stable")
            s, x, sb = s[order], x[order], sb[order]
        return kern, x, _values(rng, (ns,) + cols, complex_x), s, None, sb, None
    t = nr.ball_points(rng, nt, dim, kern.max_radius)
    t[0:25] = s[0:25]
    tb = None
    if ragged:  # the sources' middle set is empty, the targets' is not: those targets meet nothing
        tb = np.sort(rng.integers(0, 3, nt)).astype(np.int64)
        tb[0], tb[-1] = 0, 2
    return kern, x, _values(rng, (nt,) + cols, complex_x), s, t, sb, tb


def _op(kern, x, dy, s, t, sb, tb, need_sources=True, need_targets=True, clone=False):
    """the operator itself; t None: shared points -- the same tensors on both sides, or (clone) equal copies of them"""
    import torch_nfft_amd as tn
    s_, sb_ = _cuda(s), _cuda(sb)
    if t is None:
        t_, tb_ = (s_.clone(), None if sb_ is None else sb_.clone()) if clone else (s_, sb_)
    else:
        t_, tb_ = _cuda(t), _cuda(tb)
    ds, dt = tn.ops.nfft_nearfield_point_gradient(s_, t_, _cuda(x), _cuda(dy), sb_, tb_, kern.kernel_id, kern.c, kern.eps_I,
                                                  kern.near_gradient_poly.tolist(), need_sources, need_targets)
    tn.ops.check_status()
    dim = s.shape[1]
    assert ds.dtype == dt.dtype == torch.float32
    assert ds.shape == ((len(s), dim) if need_sources else (0, dim))
    assert dt.shape == ((len(s) if t is None else len(t), dim) if need_targets else (0, dim))
    return ds, dt


def _ref(kern, x, dy, s, t, sb, tb):
    return npg.near_point_gradients(kern.name, kern.c, kern.near_poly.numpy(), kern.eps_I, x, dy, s, t, sb, tb)


def _check(label, kern, got, ref):
    assert np.linalg.norm(ref) > 0 and bool(torch.isfinite(got).all())
    err = rel_l2(got.cpu().numpy(), ref)
    print("near point gradient %s %s: rel_l2 %.3e (|ref| %.3e)" % (label, kern.name, err, np.linalg.norm(ref)))
    assert err <= PGRAD_TOL[kern.name]
    return err


def _check_all_sweeps(label, kern, x, dy, s, t, sb, tb):
    """both sides at once, each side singly, and for shared points the symmetric sweep against the two one-sided ones"""
    rs, rt = _ref(kern, x, dy, s, t, sb, tb)
    shared = t is None
    ds, dt = _op(kern, x, dy, s, t, sb, tb, clone=shared)  # (shared: equal copies, so two one-sided sweeps)
    _check(label + " ds", kern, ds, rs)
    _check(label + " dt", kern, dt, rt)
    ds1, none = _op(kern, x, dy, s, t, sb, tb, need_targets=False)
    none2, dt1 = _op(kern, x, dy, s, t, sb, tb, need_sources=False)
    assert torch.equal(ds1, ds) and torch.equal(dt1, dt) and none.numel() == 0 and none2.numel() == 0
    if shared:
        total, zeros = _op(kern, x, dy, s, None, sb, None)
        assert bool((zeros == 0).all())
        _check(label + " symmetric", kern, total, rs + rt)
        gap = rel_l2(total.cpu().numpy(), (ds + dt).cpu().numpy())
        print("near point gradient %s %s: symmetric sweep vs the two one-sided sweeps %.3e" % (label, kern.name, gap))
        assert gap <= 2 * PGRAD_TOL[kern.name]  # (each within the tolerance of the same float64 sum)
    return ds, dt


@pytest.mark.parametrize("case", CASES, ids=["%dd-%s-p%d-%s-%s%s" % (c[0], c[1], c[3], "x".join(map(str, c[4])) or "1",
                                                                     c[6], "-complex" if c[5] else "") for c in CASES])
def test_operator_against_the_restatement(case):
    kern, x, dy, s, t, sb, tb = case_inputs(case)
    ds, dt = _check_all_sweeps("d=%d p=%d %s" % (case[0], case[3], case[6]), kern, x, dy, s, t, sb, tb)
    if case[6] == "ragged_separate":
        assert bool((dt[_cuda(tb == 1)] == 0).all()) and (tb == 1).sum() > 50


@pytest.fixture(scope="module")
def crowded():
    """1500 sources and 400 targets inside one cell of the 4^3 grid, every pair closer than eps_I: six LDS tiles and four
    items of that cell for the targets' gradient, two tiles and twelve items for the sources'"""
    rng = np.random.default_rng(5)
    kern = _kernel("one_over_modulus", 1.0, 3, 4)
    s = (rng.random((1500, 3)) * 0.06 + 0.01).astype(np.float32)
    t = (rng.random((400, 3)) * 0.06 + 0.01).astype(np.float32)
    t[:50] = s[:50]
    return kern, _values(rng, (1500, 2), False), _values(rng, (400, 2), False), _values(rng, (1500, 2), False), s, t


def test_one_crowded_cell(crowded):
    kern, x, dy, dy_shared, s, t = crowded
    _check_all_sweeps("crowded cell", kern, x, dy, s, t, None, None)
    _check_all_sweeps("crowded cell, shared", kern, x, dy_shared, s, None, None, None)


def test_two_calls_are_bitwise_equal(crowded):
    kern, x, dy, dy_shared, s, t = crowded
    for args in ((x, dy, s, t), (x, dy_shared, s, None)):
        a, b = _op(kern, *args, None, None), _op(kern, *args, None, None)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    kern, x, dy, s, t, sb, tb = case_inputs(CASES[9])  # ragged, complex, ten real columns
    a, b = _op(kern, x, dy, s, t, sb, tb), _op(kern, x, dy, s, t, sb, tb)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_points_on_cell_faces_and_on_the_sphere():
    rng = np.random.default_rng(7)
    kern = _kernel("one_over_modulus", 1.0, 2, 4)
    faces = (np.arange(CELLS + 1, dtype=np.float64) / (2 * CELLS) - 0.25).astype(np.float32)
    lattice = np.stack(np.meshgrid(faces, faces, indexing="ij"), -1).reshape(-1, 2)
    ang = rng.random(100) * 2 * np.pi
    sphere = (np.stack([np.cos(ang), np.sin(ang)], -1) * kern.max_radius).astype(np.float32)
    near_faces = lattice[rng.integers(0, len(lattice), 200)] + (rng.standard_normal((200, 2)) * 1e-7).astype(np.float32)
    s = np.concatenate([lattice, sphere, near_faces, nr.ball_points(rng, 300, 2, kern.max_radius)]).astype(np.float32)
    t = np.concatenate([lattice, sphere[::-1], near_faces[:100] + np.float32(0.03), nr.ball_points(rng, 200, 2, 0.25)])
    t = t.astype(np.float32)
    x, dy = _values(rng, (len(s), 2), False), _values(rng, (len(t), 2), False)
    _check_all_sweeps("cell faces", kern, x, dy, s, t, None, None)
    _check_all_sweeps("cell faces, shared", kern, x, _values(rng, (len(s), 2), False), s, None, None, None)


@pytest.mark.parametrize("name", nr.NAMES)
def test_coincident_points_weigh_exactly_zero(name):
    """clusters of identical points farther than eps_I from one another: every pair in range has r = 0, where K'(r) / r is
    infinite for five of the kernels -- the result is exactly zero, not NaN"""
    rng = np.random.default_rng(11)
    kern = _kernel(name, 0.02, 3, 4)
    centres = (np.stack(np.meshgrid(*[np.array([-0.15, 0.0, 0.15])] * 3, indexing="ij"), -1).reshape(-1, 3)).astype(np.float32)
    s = np.repeat(centres, 20, axis=0)
    t = np.repeat(centres, 7, axis=0)
    x, dy = _values(rng, (len(s), 3), False), _values(rng, (len(t), 3), False)
    for args in ((x, dy, s, t), (x, _values(rng, (len(s), 3), False), s, None)):
        ds, dt = _op(kern, *args, None, None)
        assert bool((ds == 0).all()) and bool((dt == 0).all())


def test_targets_without_a_source_in_range_get_exact_zeros():
    rng = np.random.default_rng(8)
    kern = _kernel("one_over_square", 1.0, 2, 4)
    s = (rng.random((400, 2)) * 0.05 - 0.2).astype(np.float32)  # in [-0.2, -0.15]^2
    far = (rng.random((200, 2)) * 0.15 + 0.05).astype(np.float32)  # >= 0.2 away
    ring = s[:200] + (np.float32(0.18) * np.stack([np.cos(np.arange(200.0)), np.sin(np.arange(200.0))], -1)).astype(np.float32)
    ring = ring[(np.abs(ring) < 0.25).all(1)]
    ring = ring[np.linalg.norm(ring[:, None].astype(np.float64) - s[None].astype(np.float64), axis=-1).min(1) > 0.1251]
    assert len(ring) > 20  # targets in neighbouring cells of sources, yet farther than eps_I from every one of them
    t = np.concatenate([far, ring]).astype(np.float32)
    ds, dt = _op(kern, _values(rng, (400, 3), False), _values(rng, (len(t), 3), False), s, t, None, None)
    assert bool((ds == 0).all()) and bool((dt == 0).all())


@pytest.mark.parametrize("ns,nt,cols", [(0, 7, (2,)), (9, 0, (2,)), (9, 7, (0,)), (0, 0, ())])
def test_empty_sides_and_no_columns(ns, nt, cols):
    kern = _kernel("one_over_modulus", 1.0, 3, 4)
    rng = np.random.default_rng(9)
    s, t = nr.ball_points(rng, ns, 3, 0.2), nr.ball_points(rng, nt, 3, 0.2)
    for complex_x in (False, True):
        ds, dt = _op(kern, _values(rng, (ns,) + cols, complex_x), _values(rng, (nt,) + cols, complex_x), s, t, None, None)
        assert bool((ds == 0).all()) and bool((dt == 0).all())


# name, c, dim, separate targets, point sets: the problems of test_gpu_nearfield_gradient.py's WHOLE
WHOLE = [("one_over_modulus", 1.0, 3, False, 1), ("logarithm", 1.0, 3, True, 2), ("multiquadric", 0.05, 2, False, 1)]


@pytest.fixture(scope="module", params=WHOLE, ids=[w[0] for w in WHOLE])
def whole(request):
    """N = 32, p = 4, 800 points (600 separate targets): the problem, a random dy, and in float64 the algorithm's point
    gradients (the unpaired planes kept), the dense point gradients and the algorithm's gradient in x"""
    import torch_nfft_amd as tn
    name, c, dim, separate, B = request.param
    rng = np.random.default_rng(21 + dim)
    p = 4
    kern = tn.RegularizedKernel(name, c=c, dim=dim, bandwidth=N, p=p, device="cuda")
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
    dy = _values(rng, (600 if separate else 800,), False)
    alg = npg.exact_algorithm_point_gradients(ref, N, x, dy, s, t, sb, tb)
    dense = npg.dense_point_gradients(name, c, x, dy, s, t, sb, tb)
    alg_x = nr.exact_algorithm(ref, N, dy, s if t is None else t, None if t is None else s, sb if t is None else tb,
                               None if t is None else sb)
    return kern, x, dy, s, t, sb, tb, alg, dense, alg_x


@pytest.mark.parametrize("fastsum", [False, True], ids=["nfft_nearfield", "nfft_fastsum_nearfield"])
def test_point_gradients_through_autograd(whole, fastsum):
    import torch_nfft_amd as tn
    kern, x, dy, s, t, sb, tb, alg, dense, alg_x = whole
    xs, ss = _cuda(x).requires_grad_(True), _cuda(s).requires_grad_(True)
    ts = None if t is None else _cuda(t).requires_grad_(True)
    if fastsum:
        y = tn.nfft_fastsum_nearfield(xs, kern, ss, ts, _cuda(sb), _cuda(tb), cutoff=4, point_gradients=True)
        want_s, want_t, want_x, tol = alg[0], alg[1], alg_x, WHOLE_PGRAD_TOL
    else:
        y = tn.nfft_nearfield(xs, kern, ss, ts, _cuda(sb), _cuda(tb), point_gradients=True)
        want_s, want_t = npg.near_point_gradients(kern.name, kern.c, kern.near_poly.numpy(), kern.eps_I, x, dy, s, t, sb, tb)
        want_x = nr.near_sum(kern.name, kern.c, kern.near_poly.numpy(), kern.eps_I, dy, s if t is None else t,
                             None if t is None else s, sb if t is None else tb, None if t is None else sb)
        tol = PGRAD_TOL[kern.name]
    tol_x = WHOLE_TOL if fastsum else NEAR_TOL[kern.name]
    y.backward(_cuda(dy))
    tn.ops.check_status()
    label = "whole" if fastsum else "near"
    if t is None:  # shared points: one .grad holds the sum of the two roles
        got, want = ss.grad.cpu().numpy(), want_s + want_t
        dense_ref = dense[0] + dense[1]
    else:
        got = np.concatenate([ss.grad.cpu().numpy(), ts.grad.cpu().numpy()])
        want, dense_ref = np.concatenate([want_s, want_t]), np.concatenate(dense)
        e_s, e_t = rel_l2(ss.grad.cpu().numpy(), want_s), rel_l2(ts.grad.cpu().numpy(), want_t)
        print("%s point gradients %s: sources.grad %.3e, targets.grad %.3e" % (label, kern.name, e_s, e_t))
        assert e_s <= tol and e_t <= tol
    assert ss.grad.dtype == torch.float32 and ss.grad.shape == ss.shape
    e_alg, e_x = rel_l2(got, want), rel_l2(xs.grad.cpu().numpy(), want_x)
    print("%s point gradients %s: points' grad vs float64 %.3e, x.grad vs float64 %.3e" % (label, kern.name, e_alg, e_x))
    assert e_alg <= tol and e_x <= tol_x
    if fastsum:
        e_own, e_dense = rel_l2(want, dense_ref), rel_l2(got, dense_ref)
        print("whole point gradients %s: vs dense %.3e (the float64 algorithm's own error %.3e)" % (kern.name, e_dense, e_own))
        assert e_dense <= 1.1 * e_own


def test_second_derivative_through_the_points_is_refused():
    import torch_nfft_amd as tn
    kern, x, dy, s, t, sb, tb = case_inputs(CASES[0])
    xs, ss = _cuda(x).requires_grad_(True), _cuda(s).requires_grad_(True)
    z = tn.nfft_nearfield(xs, kern, ss, point_gradients=True)
    g, = torch.autograd.grad(z, ss, _cuda(dy), create_graph=True)
    assert g.requires_grad
    with pytest.raises(RuntimeError, match="second derivatives with respect to the near field's points"):
        torch.autograd.grad(g.square().sum(), ss)
    # dx stays differentiable in dy: d<probe, W^T dy>/d dy = W probe
    dys = _cuda(dy).requires_grad_(True)
    z = tn.nfft_nearfield(xs, kern, ss, point_gradients=True)
    gx, = torch.autograd.grad(z, xs, dys, create_graph=True)
    probe = _cuda(_values(np.random.default_rng(3), x.shape, False))
    gg, = torch.autograd.grad(gx, dys, probe)
    assert torch.equal(gg, tn.nfft_nearfield(probe, kern, ss.detach()))
    tn.ops.check_status()


def test_keyword_without_point_gradients_is_the_plain_call():
    import torch_nfft_amd as tn
    kern, x, dy, s, t, sb, tb = case_inputs(CASES[3])
    kern = _kernel(kern.name, kern.c, 3, 4, device="cuda")
    xs, ss, ts = _cuda(x).requires_grad_(True), _cuda(s), _cuda(t)
    def same(a, b, bitwise):
        # the far part spreads with atomics, so two plain calls of nfft_fastsum_nearfield already differ in the last bits
        return torch.equal(a, b) if bitwise else rel_l2(b.detach().cpu().numpy(), a.detach().cpu().numpy()) <= T_ENTRY

    for fn, kw, bitwise in ((tn.nfft_nearfield, {}, True), (tn.nfft_fastsum_nearfield, {"cutoff": 4}, False)):
        a, b = fn(xs, kern, ss, ts, **kw), fn(xs, kern, ss, ts, point_gradients=True, **kw)
        assert same(a, b, bitwise)
        ga, = torch.autograd.grad(a, xs, _cuda(dy))
        gb, = torch.autograd.grad(b, xs, _cuda(dy))
        assert same(ga, gb, bitwise)
        nodes = [type(b.grad_fn).__name__] + [type(f).__name__ for f, _ in b.grad_fn.next_functions if f is not None]
        assert any(n.startswith("NfftNearfieldFunction") for n in nodes), nodes  # today's Function, not the points' one
    assert type(tn.nfft_nearfield(xs, kern, ss, ts, point_gradients=True).grad_fn).__name__.startswith("NfftNearfieldFunction")
    with pytest.raises(AssertionError, match="targets"):
        tn.nfft_nearfield(xs, kern, ss, ts.clone().requires_grad_(True))
    with pytest.raises(AssertionError, match="source_batch"):
        tn.nfft_nearfield(xs, kern, ss, ts, torch.zeros(len(s), device="cuda", requires_grad=True), None, point_gradients=True)
    with pytest.raises(ValueError, match="p >= 2"):
        tn.nfft_fastsum_nearfield(xs, _kernel("logarithm", 1.0, 3, 1, device="cuda"), ss.clone().requires_grad_(True),
                                  point_gradients=True)
    tn.ops.check_status()
