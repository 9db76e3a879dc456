"""GPU tests of the gradient with respect to the points (nfft_forward / nfft_adjoint, pos.requires_grad).

Tolerances (fp32, set from the first MI355X run with about 3x margin):
  TR  HIP vs the float64 restatement of the window-derivative gather (test_pos_grad_ref.py): relative L2 <= 4e-6
      (observed 5e-7 .. 1.2e-6)
  TE  HIP vs the exact gradient (dense float64 NDFT under torch autograd), per cutoff m: the float64 algorithm's own gap
      (observed on a 3-D N = 16 problem: 0.35, 3.0e-2, 3.1e-3, 3.4e-4, 4.0e-5, 4.8e-6, 5.8e-7, 7.1e-8 for m = 1 .. 8) times
      about 3, with an fp32 floor of ~1e-6 (observed 8.4e-7 at m = 8)
  TD  directional derivative <dpos, delta> vs a central difference of the float64 algorithm: relative 1e-4
"""
import numpy as np
import pytest
import torch

import test_pos_grad_ref as ref

pytestmark = pytest.mark.gpu

TR = 4e-6
TE = {1: 1.0, 2: 0.1, 3: 1.2e-2, 4: 1.2e-3, 5: 1.5e-4, 6: 2e-5, 7: 4e-6, 8: 3e-6}
TD = 1e-4


@pytest.fixture(scope="module")
def tn():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import torch_nfft_amd
    return torch_nfft_amd


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def rel(a, b):
    return float(np.linalg.norm(np.ravel(a - b)) / np.linalg.norm(np.ravel(b)))


def make(rng, d, N, n, cols, complex_x, B):
    pos, batch, xhat = ref.problem(rng, d, N, n, cols, complex_x, B)
    return pos, batch, (xhat.astype(np.complex64) if complex_x else xhat.astype(np.float32))


def forward_pos_grad(tn, xhat, pos, batch, m, ro, w):
    """pos.grad of sum(w * real columns of nfft_forward(xhat, pos))."""
    p = dev(pos).requires_grad_(True)
    y = tn.nfft_forward(dev(xhat), p, dev(batch), cutoff=m, real_output=ro)
    yr = y if not y.is_complex() else torch.view_as_real(y)
    (yr.reshape(len(pos), -1) * dev(w.astype(np.float32))).sum().backward()
    return p.grad


def test_pos_grad_is_set_and_exact(tn):
    """Fails without the feature: pos.grad stayed None."""
    rng = np.random.default_rng(0)
    pos, batch, xhat = make(rng, 2, 16, 300, (), True, 1)
    w = rng.standard_normal((300, 2))
    g = forward_pos_grad(tn, xhat, pos, batch, 4, False, w)
    assert g is not None and g.shape == (300, 2) and g.dtype == torch.float32
    assert rel(host(g), ref.exact_forward_pos_grad(xhat, pos, batch, False, w)) < TE[4]


CASES = [  # d, N, n, cols, complex xhat, real_output, B, m
    (1, 64, 500, (), False, True, 1, 3),
    (1, 64, 500, (3,), True, False, 3, 8),
    (2, 16, 400, (), True, False, 1, 4),          # small-grid problem: nfft_hip_plan_needed == 0
    (2, 16, 400, (2, 2), False, False, 3, 3),
    (2, 64, 800, (3,), True, True, 1, 1),
    (3, 16, 600, (), True, False, 3, 4),
    (3, 32, 3000, (2, 2), False, True, 1, 8),
    (3, 64, 3000, (), True, False, 1, 4),         # wide 3-D tiling
    (3, 64, 3000, (3,), False, False, 3, 3),      # wide tiling, column count of the paired plans
]


@pytest.mark.parametrize("d,N,n,cols,cx,ro,B,m", CASES)
def test_forward_pos_grad_matches_restatement(tn, d, N, n, cols, cx, ro, B, m):
    rng = np.random.default_rng(d * 100 + N + m)
    pos, batch, xhat = make(rng, d, N, n, cols, cx, B)
    C = int(np.prod(cols)) if cols else 1
    w = rng.standard_normal((n, C if ro else 2 * C))
    g = host(forward_pos_grad(tn, xhat, pos, batch, m, ro, w))
    assert g.shape == (n, d) and np.isfinite(g).all()
    assert rel(g, ref.pos_grad(xhat, pos, batch, m, ro, w)) < TR
    if n * N ** d <= 2e6:
        assert rel(g, ref.exact_forward_pos_grad(xhat, pos, batch, ro, w)) < TE[m]


@pytest.mark.parametrize("d,N,cols,cx,ro,B,m", [
    (1, 64, (), True, False, 1, 4),
    (2, 16, (3,), True, False, 3, 3),             # small grid
    (2, 16, (), False, True, 1, 8),
    (3, 16, (2, 2), True, True, 3, 4),
    (3, 64, (), False, False, 1, 4),              # wide tiling
])
def test_adjoint_pos_grad(tn, d, N, cols, cx, ro, B, m):
    """y = nfft_adjoint(x, pos): pos.grad against the restatement (gather of forward(dy) weighted by x) and exactly."""
    rng = np.random.default_rng(d + N + m)
    n = 700
    pos, batch, _ = ref.problem(rng, d, N, n, (), False, B)
    x = rng.standard_normal((n,) + cols)
    if cx:
        x = x + 1j * rng.standard_normal(x.shape)
    x = x.astype(np.complex64 if cx else np.float32)
    Bn = 1 if batch is None else B
    dy = rng.standard_normal((Bn,) + (N,) * d + cols)
    if not ro:
        dy = dy + 1j * rng.standard_normal(dy.shape)
    dy = dy.astype(np.float32 if ro else np.complex64)
    p = dev(pos).requires_grad_(True)
    xt = dev(x).requires_grad_(True)
    y = tn.nfft_adjoint(xt, p, dev(batch), bandwidth=N, cutoff=m, real_output=ro)
    y.backward(dev(dy))
    g = host(p.grad)
    assert g.shape == (n, d)
    expect = ref.pos_grad(dy, pos, batch, m, not cx, ref.real_columns(x, n))
    assert rel(g, expect) < TR
    if n * N ** d <= 4e6:  # (the dense adjoint of a 64^3 band is too big for the exact check)
        assert rel(g, ref.exact_adjoint_pos_grad(x, pos, batch, Bn, N, ro, dy)) < TE[m]


def test_exact_gradient_ladder(tn):
    """The gap to the exact gradient falls with m, as the transform's own error does."""
    rng = np.random.default_rng(5)
    pos, batch, xhat = make(rng, 3, 16, 500, (), True, 1)
    w = rng.standard_normal((500, 2))
    exact = ref.exact_forward_pos_grad(xhat, pos, batch, False, w)
    errs = []
    for m in (1, 2, 3, 4, 6, 8):
        errs.append(rel(host(forward_pos_grad(tn, xhat, pos, batch, m, False, w)), exact))
        assert errs[-1] < TE[m], (m, errs)
    assert errs[-1] < errs[0] / 100, errs


def test_large_chunked_problem_sampled(tn):
    """3-D N = 128, m = 4, 10^6 points, two columns: plane chunks and point splits; 2e4 sampled points."""
    rng = np.random.default_rng(11)
    n, N, m = 10 ** 6, 128, 4
    pos = (rng.random((n, 3)) - 0.5).astype(np.float32)
    xhat = (rng.standard_normal((1, N, N, N, 2)) + 1j * rng.standard_normal((1, N, N, N, 2))).astype(np.complex64)
    w = rng.standard_normal((n, 4)).astype(np.float32)
    g = host(forward_pos_grad(tn, xhat, pos, None, m, False, w))
    assert np.isfinite(g).all()
    idx = np.sort(np.random.default_rng(12).choice(n, 20000, replace=False))
    expect = ref.grad_gather(ref.grid_of(xhat, 3, m), pos[idx], None, m, False, w[idx])
    assert rel(g[idx], expect) < TR


def test_cell_boundaries_and_periodicity(tn):
    """Points on cell boundaries and at +-1/2: the gradient is periodic and continuous, no jump at a cell edge."""
    rng = np.random.default_rng(3)
    N, m = 16, 4
    M = 2 * N
    eps = 2.0 ** -20
    edge = np.array([[3 / M, -5 / M], [0.0, 0.0], [-0.5, 7 / M]])
    # +-1/2 is one point of the torus; a cell edge and both of its sides
    pos = np.concatenate([[[-0.5, -0.5], [0.5, 0.5], [-0.5, 0.25], [0.5, 0.25]], edge - eps, edge, edge + eps])
    pos = pos.astype(np.float32)
    n = len(pos)
    xhat = (rng.standard_normal((1, N, N)) + 1j * rng.standard_normal((1, N, N))).astype(np.complex64)
    w = np.repeat(rng.standard_normal((1, 2)), n, 0)  # the same weights everywhere: gradients comparable point to point
    for extra in (0, 20000):  # alone (small-grid problem) and among many points (general plan path)
        P = np.concatenate([pos, (rng.random((extra, 2)) - 0.5).astype(np.float32)])
        W = np.concatenate([w, rng.standard_normal((extra, 2))])
        g = host(forward_pos_grad(tn, xhat, P, None, m, False, W))
        assert rel(g, ref.pos_grad(xhat, P, None, m, False, W)) < TR
        g = g[:n]
        scale = np.abs(g).max()
        assert np.abs(g[0] - g[1]).max() <= 1e-5 * scale
        assert np.abs(g[2] - g[3]).max() <= 1e-5 * scale
        k = len(edge)
        lo, on, hi = g[4:4 + k], g[4 + k:4 + 2 * k], g[4 + 2 * k:]
        assert np.abs(lo - on).max() <= 1e-3 * scale and np.abs(hi - on).max() <= 1e-3 * scale


def test_bitwise_reproducible(tn):
    rng = np.random.default_rng(4)
    pos, batch, xhat = make(rng, 3, 64, 50000, (2,), True, 3)
    w = rng.standard_normal((50000, 4))
    a = forward_pos_grad(tn, xhat, pos, batch, 4, False, w)
    b = forward_pos_grad(tn, xhat, pos, batch, 4, False, w)
    assert torch.equal(a, b)


def test_x_grad_unchanged_by_pos_grad(tn):
    """x.grad does not depend on whether pos asks for a gradient.  Bitwise for nfft_adjoint (its x-gradient is a forward
    transform: a gather); nfft_forward's x-gradient is an adjoint, whose spreading kernels add with atomics."""
    rng = np.random.default_rng(6)
    n, N, m = 5000, 32, 4
    pos = dev((rng.random((n, 3)) - 0.5).astype(np.float32))
    x = dev(rng.standard_normal((n, 2)).astype(np.float32))
    dy = dev((rng.standard_normal((1, N, N, N, 2)) + 1j * rng.standard_normal((1, N, N, N, 2))).astype(np.complex64))
    grads = []
    for pg in (False, True):
        p = pos.clone().requires_grad_(pg)
        xt = x.clone().requires_grad_(True)
        tn.nfft_adjoint(xt, p, None, bandwidth=N, cutoff=m).backward(dy)
        grads.append(xt.grad)
        assert (p.grad is not None) == pg
    assert torch.equal(grads[0], grads[1])
    xh = dev((rng.standard_normal((1, N, N, N)) + 1j * rng.standard_normal((1, N, N, N))).astype(np.complex64))
    dyf = dev((rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64))
    grads = []
    for pg in (False, True):
        p = pos.clone().requires_grad_(pg)
        xt = xh.clone().requires_grad_(True)
        tn.nfft_forward(xt, p, None, cutoff=m).backward(dyf)
        grads.append(xt.grad)
    assert rel(host(grads[1]), host(grads[0])) < 1e-6


def test_directional_finite_difference(tn):
    """<dpos, delta> against (L(p + h delta) - L(p - h delta)) / 2h of the float64 algorithm."""
    rng = np.random.default_rng(8)
    d, N, m, n = 3, 16, 6, 400
    pos, batch, xhat = make(rng, d, N, n, (), True, 1)
    w = rng.standard_normal((n, 2))
    g = host(forward_pos_grad(tn, xhat, pos, batch, m, False, w)).astype(np.float64)
    delta = rng.standard_normal((n, d))
    grid = ref.grid_of(xhat, d, m)
    h = 1e-6

    def L(p):
        return float((ref.interp_f64(grid, p, m, False) * w).sum())

    p64 = pos.astype(np.float64)
    fd = (L(p64 + h * delta) - L(p64 - h * delta)) / (2 * h)
    assert abs((g * delta).sum() - fd) <= TD * np.abs(g * delta).sum()
