"""GPU tests of the second derivatives of nfft_forward / nfft_adjoint (double backward, create_graph=True).

Tolerances (fp32):
  TE2  second derivatives vs double autograd of a dense float64 NDFT, per cutoff m (test_pos_hvp_ref.TE2)
  TR2  the native backward of the point gradient (dw, dpos) vs its float64 restatement: relative L2
  TE   dxhat (spectral multipliers of the library's adjoint) vs the same multipliers of the exact adjoint: the first-order
       table of test_gpu_pos_grad.py
  TD   a directional central difference of the float64 restatement's gradient: relative 1e-4
"""
import numpy as np
import pytest
import torch

import test_pos_grad_ref as ref1
import test_pos_hvp_ref as ref
from test_gpu_pos_grad import TE, dev, host, make, rel
from test_pos_hvp_ref import TE2

pytestmark = pytest.mark.gpu

TR2 = 1e-5
TD = 1e-4


@pytest.fixture(scope="module")
def tn():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import torch_nfft_amd
    return torch_nfft_amd


def real_view(y):
    return torch.view_as_real(y) if y.is_complex() else y


def forward_hvp(tn, xhat, pos, batch, m, ro, w, u, xhat_grad=False, w_grad=False):
    """g = d/dpos sum(w * real columns of nfft_forward(xhat, pos)) under create_graph, then (g . u).sum().backward()."""
    p = dev(pos).requires_grad_(True)
    xh = dev(xhat).requires_grad_(xhat_grad)
    W = dev(w.astype(np.float32)).requires_grad_(w_grad)
    y = tn.nfft_forward(xh, p, dev(batch), cutoff=m, real_output=ro)
    L = (real_view(y).reshape(len(pos), -1) * W).sum()
    (g,) = torch.autograd.grad(L, p, create_graph=True)
    (g * dev(u.astype(np.float32))).sum().backward()
    return g.detach(), p.grad, xh.grad, W.grad


def test_forward_double_backward_matches_exact_hvp(tn):
    """Fails without the feature: the create_graph gradient carried no graph, so the second backward raised."""
    rng = np.random.default_rng(0)
    pos, batch, xhat = make(rng, 2, 16, 300, (), True, 1)
    w = rng.standard_normal((300, 2))
    u = rng.standard_normal((300, 2))
    for m in (4, 8):
        _, hp, _, _ = forward_hvp(tn, xhat, pos, batch, m, False, w, u)
        assert hp is not None and hp.shape == (300, 2)
        _, _, ex = ref.exact_g_backward(xhat, pos, batch, False, w, u)
        assert rel(host(hp), ex) < TE2[m], (m, rel(host(hp), ex))


@pytest.mark.parametrize("cx", [False, True])
def test_adjoint_double_backward_matches_exact_hvp(tn, cx):
    rng = np.random.default_rng(1 + cx)
    d, N, n, B, m = 2, 16, 200, 2, 6
    pos = (rng.random((n, d)) - 0.5).astype(np.float32)
    batch = np.sort(rng.integers(0, B, n)).astype(np.int64)
    batch[0], batch[-1] = 0, B - 1
    x = rng.standard_normal((n, 2))
    if cx:
        x = x + 1j * rng.standard_normal((n, 2))
    dy = rng.standard_normal((B, N, N, 2)) + 1j * rng.standard_normal((B, N, N, 2))
    u = rng.standard_normal((n, d))
    # GPU
    p = dev(pos).requires_grad_(True)
    xt = dev(x.astype(np.complex64 if cx else np.float32)).requires_grad_(True)
    dyt_gpu = dev(dy.astype(np.complex64)).requires_grad_(True)  # the upstream gradient is differentiated too
    y = tn.nfft_adjoint(xt, p, dev(batch), bandwidth=N, cutoff=m)
    L = (torch.view_as_real(y) * torch.view_as_real(dyt_gpu)).sum()
    (g,) = torch.autograd.grad(L, p, create_graph=True)
    (g * dev(u.astype(np.float32))).sum().backward()
    # exact
    pe = torch.tensor(pos.astype(np.float64), requires_grad=True)
    xe = torch.tensor(x).requires_grad_(True)
    ye = ref1.ndft_adjoint_t(xe.to(torch.complex128), pe, batch, B, N)
    dyt = torch.as_tensor(dy).reshape(ye.shape).clone().requires_grad_(True)
    Le = (ye.real * dyt.real + ye.imag * dyt.imag).sum()
    (ge,) = torch.autograd.grad(Le, pe, create_graph=True)
    hp, hx, hdy = torch.autograd.grad((ge * torch.as_tensor(u)).sum(), (pe, xe, dyt))
    assert rel(host(p.grad), hp.numpy()) < TE2[m]
    assert rel(host(xt.grad), hx.numpy()) < TE2[m]  # mixed pos / x
    # mixed pos / dy: the dxhat output of the native backward, reached through the adjoint's create_graph path
    assert dyt_gpu.grad is not None and rel(host(dyt_gpu.grad), hdy.reshape(dy.shape).numpy()) < TE2[m]


@pytest.mark.parametrize("cx,ro", [(True, False), (False, False), (True, True)])
def test_mixed_second_derivatives(tn, cx, ro):
    """d/dxhat and d/d(upstream weights) of <u, dpos>, against double autograd of the exact transform."""
    rng = np.random.default_rng(3 + 2 * cx + ro)
    m = 6
    pos, batch, xhat = make(rng, 3, 8, 150, (2,), cx, 2)
    w = rng.standard_normal((150, 2 if ro else 4))
    u = rng.standard_normal((150, 3))
    _, hp, hx, hw = forward_hvp(tn, xhat, pos, batch, m, ro, w, u, xhat_grad=True, w_grad=True)
    ex_dx, ex_dw, ex_dp = ref.exact_g_backward(xhat, pos, batch, ro, w, u)
    assert rel(host(hp), ex_dp) < TE2[m]
    assert rel(host(hw), ex_dw) < TE2[m]
    assert hx.dtype == (torch.complex64 if cx else torch.float32)
    assert rel(host(hx), ex_dx) < TE2[m]


def native_backward(tn, xhat, pos, batch, m, ro, w, v):
    return tn.ops.nfft_forward_grad_points_backward(dev(pos), dev(xhat), dev(batch), m, ro, dev(w.astype(np.float32)),
                                                    dev(v.astype(np.float32)), True, True, True)


NATIVE = [  # d, N, n, cols, complex xhat, real_output, B, m
    (1, 64, 500, (), False, True, 1, 1),
    (1, 64, 500, (3,), True, False, 3, 8),
    (2, 16, 400, (), True, False, 1, 4),          # the reference's small 2-D grid (N = 16)
    (2, 16, 400, (3,), False, False, 3, 8),
    (2, 64, 800, (), True, True, 1, 1),
    (3, 16, 600, (), True, False, 3, 4),
    (3, 32, 3000, (3,), False, True, 1, 8),
    (3, 32, 3000, (), True, False, 1, 1),         # narrow tiling
    (3, 64, 3000, (), True, False, 1, 4),         # wide 3-D tiling
    (3, 64, 3000, (3,), False, False, 3, 8),      # W = 18 > 16: the narrow 8 x 16 tiling on the 128^3 grid, several columns
]


@pytest.mark.parametrize("d,N,n,cols,cx,ro,B,m", NATIVE)
def test_native_backward_matches_restatement(tn, d, N, n, cols, cx, ro, B, m):
    rng = np.random.default_rng(7 * d + n + m)
    pos, batch, xhat = make(rng, d, N, n, cols, cx, B)
    C = int(np.prod(cols)) if cols else 1
    w = rng.standard_normal((n, C if ro else 2 * C))
    v = rng.standard_normal((n, d))
    dx, dw, dp = native_backward(tn, xhat, pos, batch, m, ro, w, v)
    sel = np.arange(n) if n <= 800 else rng.choice(n, 400, replace=False)
    g = ref1.grid_of(xhat, d, m)
    rdw, rdp = ref.hvp_gather(g, pos[sel], None if batch is None else batch[sel], m, ro, w[sel], v[sel])
    assert rel(host(dw)[sel], rdw) < TR2, rel(host(dw)[sel], rdw)
    assert rel(host(dp)[sel], rdp) < TR2, rel(host(dp)[sel], rdp)
    if n <= 800:
        rdx = ref.spectral_dxhat(xhat.shape, cx, pos, batch, ro, w, v)
        assert dx.shape == xhat.shape and rel(host(dx), rdx) < TE[m]


def test_ragged_batches_with_empty_sets(tn):
    rng = np.random.default_rng(11)
    d, N, n, B, m = 2, 32, 300, 5, 4
    pos = (rng.random((n, d)) - 0.5).astype(np.float32)
    batch = np.sort(rng.choice([0, 2, 4], n)).astype(np.int64)  # sets 1 and 3 empty
    xhat = (rng.standard_normal((B, N, N, 2)) + 1j * rng.standard_normal((B, N, N, 2))).astype(np.complex64)
    w = rng.standard_normal((n, 4))
    v = rng.standard_normal((n, d))
    dx, dw, dp = native_backward(tn, xhat, pos, batch, m, False, w, v)
    rdw, rdp = ref.hvp_gather(ref1.grid_of(xhat, d, m), pos, batch, m, False, w, v)
    assert rel(host(dw), rdw) < TR2 and rel(host(dp), rdp) < TR2
    hx = host(dx)
    assert np.all(hx[1] == 0) and np.all(hx[3] == 0)
    assert rel(hx, ref.spectral_dxhat(xhat.shape, True, pos, batch, False, w, v)) < TE[m]


def test_boundary_points(tn):
    """Points on cell boundaries of the oversampled grid and at -0.5."""
    rng = np.random.default_rng(12)
    d, N, m = 2, 16, 4
    M = 2 * N
    pos = (rng.integers(-M // 2, M // 2, (200, d)) / M).astype(np.float32)
    pos[:10] = -0.5
    xhat = (rng.standard_normal((1, N, N)) + 1j * rng.standard_normal((1, N, N))).astype(np.complex64)
    w = rng.standard_normal((200, 2))
    v = rng.standard_normal((200, d))
    _, dw, dp = native_backward(tn, xhat, pos, None, m, False, w, v)
    rdw, rdp = ref.hvp_gather(ref1.grid_of(xhat, d, m), pos, None, m, False, w, v)
    assert rel(host(dw), rdw) < TR2 and rel(host(dp), rdp) < TR2


CHUNKED = [  # d, N, n, cols, complex xhat, real_output, B, m: chunks of one plane (real_output) or one (re, im) pair, so
    #          chunks start inside point sets; enough points per tile for point splits (blockIdx.z > 1)
    (2, 32, 200000, (3,), True, True, 2, 4),       # narrow tiling: dxhat by the derivative spreading
    (2, 32, 200000, (3,), False, False, 2, 4),
    (3, 64, 100000, (2,), True, False, 1, 3),      # wide tiling: dxhat by the composition, its adjoints chunked too
]


@pytest.mark.parametrize("d,N,n,cols,cx,ro,B,m", CHUNKED)
def test_large_chunked_problem_sampled(tn, monkeypatch, d, N, n, cols, cx, ro, B, m):
    """The native backward with the smallest plane chunks against the same call in one chunk (dw, dpos bitwise: every
    (plane, point) is one lane's sum, the planes meet in a fixed order) and against the float64 restatement on 2 000
    sampled points."""
    rng = np.random.default_rng(20 + d + ro)
    pos, batch, xhat = make(rng, d, N, n, cols, cx, B)
    C = int(np.prod(cols))
    w = rng.standard_normal((n, C if ro else 2 * C))
    v = rng.standard_normal((n, d))
    whole = native_backward(tn, xhat, pos, batch, m, ro, w, v)
    monkeypatch.setenv("NFFT_HIP_CHUNK_BYTES", "1")  # (one chunk = the planes of one column)
    dx, dw, dp = native_backward(tn, xhat, pos, batch, m, ro, w, v)
    assert torch.equal(dw, whole[1]) and torch.equal(dp, whole[2])
    assert rel(host(dx), host(whole[0])) < 1e-5
    sel = np.sort(rng.choice(n, 2000, replace=False))
    rdw, rdp = ref.hvp_gather(ref1.grid_of(xhat, d, m), pos[sel], None if batch is None else batch[sel], m, ro, w[sel],
                              v[sel])
    assert rel(host(dw)[sel], rdw) < TR2 and rel(host(dp)[sel], rdp) < TR2


@pytest.mark.parametrize("d,N,cols,cx,ro,B,m", [(1, 64, (), False, True, 1, 3), (2, 16, (2,), True, False, 2, 4),
                                                  (2, 32, (), False, False, 1, 6), (3, 32, (2,), True, True, 2, 2)])
def test_derivative_spreading_matches_composition(tn, monkeypatch, d, N, cols, cx, ro, B, m):
    """dxhat on the narrow tilings: the derivative spreading (default) against the composition of dim adjoints
    (NFFT_HIP_DXHAT=compose), and both against the spectral multipliers of the exact adjoint."""
    rng = np.random.default_rng(30 + d + m)
    n = 600
    pos, batch, xhat = make(rng, d, N, n, cols, cx, B)
    C = int(np.prod(cols)) if cols else 1
    w = rng.standard_normal((n, C if ro else 2 * C))
    v = rng.standard_normal((n, d))
    fused = host(native_backward(tn, xhat, pos, batch, m, ro, w, v)[0])
    monkeypatch.setenv("NFFT_HIP_DXHAT", "compose")
    composed = host(native_backward(tn, xhat, pos, batch, m, ro, w, v)[0])
    exact = ref.spectral_dxhat(xhat.shape, cx, pos, batch, ro, w, v)
    assert fused.dtype == composed.dtype and fused.shape == xhat.shape
    assert rel(fused, exact) < TE[m] and rel(composed, exact) < TE[m]
    assert rel(fused, composed) < 2 * TE[m]


def test_create_graph_first_order_is_bitwise_unchanged(tn):
    """The point gradient under create_graph is the same native gather: bitwise the same."""
    rng = np.random.default_rng(13)
    pos, batch, xhat = make(rng, 3, 32, 2000, (2,), True, 2)
    w = dev(rng.standard_normal((2000, 4)).astype(np.float32))
    outs = []
    for cg in (False, True):
        p = dev(pos).requires_grad_(True)
        xh = dev(xhat).requires_grad_(True)
        y = tn.nfft_forward(xh, p, dev(batch), cutoff=4)
        L = (torch.view_as_real(y).reshape(2000, -1) * w).sum()
        outs.append([t.detach().clone() for t in torch.autograd.grad(L, (p, xh), create_graph=cg)])
    assert torch.equal(outs[0][0], outs[1][0])
    # (dxhat is the same adjoint call either way, but this route's spreading accumulates with atomics: equal to rounding)
    assert rel(host(outs[1][1]), host(outs[0][1])) < 1e-6


def test_native_backward_is_bitwise_reproducible(tn):
    rng = np.random.default_rng(14)
    pos, batch, xhat = make(rng, 3, 64, 5000, (3,), False, 1)
    w = rng.standard_normal((5000, 6))
    v = rng.standard_normal((5000, 3))
    a = native_backward(tn, xhat, pos, batch, 4, False, w, v)
    b = native_backward(tn, xhat, pos, batch, 4, False, w, v)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_hessian_symmetry(tn):
    rng = np.random.default_rng(15)
    pos, batch, xhat = make(rng, 3, 16, 400, (), True, 1)
    w = rng.standard_normal((400, 2))
    u = rng.standard_normal((400, 3))
    v = rng.standard_normal((400, 3))
    _, hu, _, _ = forward_hvp(tn, xhat, pos, batch, 6, False, w, u)
    _, hv, _, _ = forward_hvp(tn, xhat, pos, batch, 6, False, w, v)
    a, b = float((host(hu) * v).sum()), float((host(hv) * u).sum())
    assert abs(a - b) <= 1e-5 * (abs(a) + abs(b)), (a, b)


def test_directional_central_difference(tn):
    """<dpos, delta> against a central difference of the float64 restatement's own gradient (test_pos_grad_ref)."""
    rng = np.random.default_rng(16)
    d, N, n, m = 2, 16, 60, 5
    pos, _, xhat = make(rng, d, N, n, (), True, 1)
    w = rng.standard_normal((n, 2))
    v = rng.standard_normal((n, d))
    _, _, dp = native_backward(tn, xhat, pos, None, m, False, w, v)
    g = ref1.grid_of(xhat, d, m)
    p = pos.astype(np.float64)
    h = 1e-5

    def grad_at(q):  # the float64 first-order gather at float64 positions
        M = g.shape[2]
        W = 2 * m + 2
        shift = np.floor(q * M).astype(np.int64) - m
        t = (q * M - shift)[:, :, None] - np.arange(W)[None, None, :]
        psi = np.exp(-(t * t) * (0.75 * np.pi / m)) * np.sqrt(0.75 / m)
        dpsi = -2.0 * t * (0.75 * np.pi / m) * psi * M
        out = np.zeros((n, d))
        for l0 in range(W):
            for l1 in range(W):
                val = g[0, 0][(shift[:, 0] + l0) % M, (shift[:, 1] + l1) % M]
                dF0 = dpsi[:, 0, l0] * psi[:, 1, l1] * val
                dF1 = psi[:, 0, l0] * dpsi[:, 1, l1] * val
                out[:, 0] += w[:, 0] * dF0.real + w[:, 1] * dF0.imag
                out[:, 1] += w[:, 0] * dF1.real + w[:, 1] * dF1.imag
        return out

    fd = ((grad_at(p + h * v) - grad_at(p - h * v)) / (2 * h))
    assert rel(host(dp), fd) < TD


def test_edge_cases(tn):
    rng = np.random.default_rng(17)
    N = 16
    # no points
    p0 = torch.zeros(0, 2, device="cuda")
    xh = dev((rng.standard_normal((1, N, N)) + 1j * rng.standard_normal((1, N, N))).astype(np.complex64))
    dx, dw, dp = tn.ops.nfft_forward_grad_points_backward(p0, xh, None, 3, False, torch.zeros(0, 2, device="cuda"),
                                                          torch.zeros(0, 2, device="cuda"), True, True, True)
    assert dx.shape == xh.shape and not dx.abs().any() and dw.shape == (0, 2) and dp.shape == (0, 2)
    # no columns
    pos = dev((rng.random((50, 2)) - 0.5).astype(np.float32))
    xc = torch.zeros(1, N, N, 0, dtype=torch.complex64, device="cuda")
    dx, dw, dp = tn.ops.nfft_forward_grad_points_backward(pos, xc, None, 3, False, torch.zeros(50, 0, device="cuda"),
                                                          torch.ones(50, 2, device="cuda"), True, True, True)
    assert dx.shape == xc.shape and dw.shape == (50, 0) and dp.shape == (50, 2) and not dp.any()
    # v = 0: every output is zero
    w = dev(rng.standard_normal((50, 2)).astype(np.float32))
    dx, dw, dp = tn.ops.nfft_forward_grad_points_backward(pos, xh, None, 3, False, w, torch.zeros(50, 2, device="cuda"),
                                                          True, True, True)
    assert not dx.abs().any() and not dw.any() and not dp.any()
    # through autograd: n = 0 double backward gives an empty gradient
    p = p0.clone().requires_grad_(True)
    y = tn.nfft_forward(xh, p, cutoff=3)
    (g,) = torch.autograd.grad((y.abs() ** 2).sum(), p, create_graph=True)
    g.sum().backward()
    assert p.grad is not None and p.grad.shape == (0, 2)


def test_third_derivative_raises(tn):
    rng = np.random.default_rng(18)
    pos, batch, xhat = make(rng, 2, 16, 50, (), True, 1)
    p = dev(pos).requires_grad_(True)
    y = tn.nfft_forward(dev(xhat), p, cutoff=3)
    (g,) = torch.autograd.grad(torch.view_as_real(y).sum(), p, create_graph=True)
    (h,) = torch.autograd.grad(g.sum(), p, create_graph=True)
    with pytest.raises(RuntimeError):
        h.sum().backward()
