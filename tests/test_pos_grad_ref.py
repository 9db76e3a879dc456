"""CPU tests of the gradient with respect to the points, and the float64 restatement the GPU tests compare against.

The restatement: the gradient of the forward NFFT with respect to the points,

    dpos[i, a] = sum_cr w[i, cr] * d Fr[i, cr] / d pos[i, a]

with Fr the real columns of nfft_forward(xhat, pos, batch, m, real_output) (C columns with real_output, else 2C: re, im
interleaved), evaluated as the library does: the deconvolved, FFT'd grid of oracle.nfft_ref, gathered with the derivative
of the window,  d/dpos_a prod_b psi(t_b) = M psi'(t_a) prod_{b != a} psi(t_b),  psi'(t) = -2 t (0.75 pi / m) psi(t).
Built from oracle.nfft_ref's pieces (window_taps, _rolloff, _band_index).  Also a dense float64 NDFT in torch whose
autograd gives the exact gradient.
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from oracle import nfft_ref


def grid_of(xhat, d, m):
    """g [B, C, M..M] complex128 for a spectral array xhat [B, N^d, *cols]."""
    xhat = np.asarray(xhat)
    B, N = xhat.shape[0], xhat.shape[1]
    M = 2 * N
    xr = xhat.reshape((B,) + (N,) * d + (-1,)).astype(np.complex128)
    C = xr.shape[-1]
    g_hat = np.zeros((B, C) + (M,) * d, dtype=np.complex128)
    kap = nfft_ref._band_index(N)
    g_hat[(slice(None), slice(None)) + np.ix_(*([kap] * d))] = np.moveaxis(xr, -1, 1) * nfft_ref._rolloff(N, m, d)[None, None]
    return np.fft.fftn(g_hat, axes=tuple(range(2, 2 + d)))


def grad_gather(g, pos, batch, m, real_output, w):
    """dpos [n, d] float64 from the grid g of grid_of(); w [n, Cr]."""
    pos = np.asarray(pos)
    n, d = pos.shape
    B, C = g.shape[0], g.shape[1]
    M = g.shape[2]
    N = M // 2
    W = 2 * m + 2
    bvec = np.zeros(n, np.int64) if batch is None else np.asarray(batch).astype(np.int64)
    shift, psi = nfft_ref.window_taps(pos, N, m)
    p = np.asarray(pos, dtype=np.float32).astype(np.float64)
    t = (p * M - shift)[:, :, None] - np.arange(W, dtype=np.float64)[None, None, :]
    dpsi = -2.0 * t * (0.75 * np.pi / m) * psi * M  # d psi / d pos
    dF = np.zeros((n, d, C), dtype=np.complex128)
    for ls in itertools.product(range(W), repeat=d):
        idx = tuple((shift[:, a] + ls[a] + M) % M for a in range(d))
        vals = np.stack([g[(bvec, c) + idx] for c in range(C)], axis=1)  # [n, C]
        for a in range(d):
            wa = np.ones(n)
            for b in range(d):
                wa = wa * (dpsi[:, b, ls[b]] if b == a else psi[:, b, ls[b]])
            dF[:, a, :] += wa[:, None] * vals
    dFr = dF.real if real_output else np.stack([dF.real, dF.imag], axis=-1).reshape(n, d, 2 * C)
    w = np.asarray(w, dtype=np.float64).reshape(n, -1)
    return np.einsum("iac,ic->ia", dFr, w)


def interp_f64(g, pos, m, real_output):
    """Real columns [n, Cr] of the forward transform from the grid g (one point set) at float64 positions (nfft_ref
    rounds positions to float32 first: too coarse for a finite difference)."""
    pos = np.asarray(pos, dtype=np.float64)
    n, d = pos.shape
    C, M = g.shape[1], g.shape[2]
    W = 2 * m + 2
    shift = np.floor(pos * M).astype(np.int64) - m
    t = (pos * M - shift)[:, :, None] - np.arange(W, dtype=np.float64)[None, None, :]
    psi = np.exp(-(t * t) * (0.75 * np.pi / m)) * np.sqrt(0.75 / m)
    y = np.zeros((n, C), dtype=np.complex128)
    for ls in itertools.product(range(W), repeat=d):
        wt = np.ones(n)
        for a in range(d):
            wt = wt * psi[:, a, ls[a]]
        idx = tuple((shift[:, a] + ls[a] + M) % M for a in range(d))
        y += wt[:, None] * np.stack([g[(0, c) + idx] for c in range(C)], axis=1)
    return y.real if real_output else np.stack([y.real, y.imag], axis=-1).reshape(n, 2 * C)


def pos_grad(xhat, pos, batch, m, real_output, w):
    d = np.asarray(pos).shape[1]
    return grad_gather(grid_of(xhat, d, m), pos, batch, m, real_output, w)


def real_columns(a, n):
    a = np.asarray(a)
    return (np.stack([a.real, a.imag], axis=-1) if np.iscomplexobj(a) else a).reshape(n, -1).astype(np.float64)


# ---- exact gradient: dense NDFT in torch float64 ----------------------------------------------------------------------

def ndft_forward_t(xhat, pos, batch):
    """y [n, C] complex128 = sum_k xhat[batch[i], k + N/2, c] exp(-2 pi i k.pos[i]) (differentiable in pos)."""
    n, d = pos.shape
    B, N = xhat.shape[0], xhat.shape[1]
    xr = xhat.reshape((B,) + (N,) * d + (-1,))
    b = torch.zeros(n, dtype=torch.long) if batch is None else torch.as_tensor(batch)
    k = torch.arange(-N // 2, N // 2, dtype=torch.float64)
    E = [torch.exp(-2j * np.pi * pos[:, a:a + 1] * k[None, :]) for a in range(d)]
    xb = xr[b]
    letters = "pqr"[:d]
    expr = "i" + letters + "c," + ",".join("i" + l for l in letters) + "->ic"
    return torch.einsum(expr, xb, *E)


def ndft_adjoint_t(x, pos, batch, B, N):
    """y [B, N^d, C] complex128 = sum_{i in set b} x[i, c] exp(+2 pi i k.pos[i])."""
    n, d = pos.shape
    xc = x.reshape(n, -1)
    b = torch.zeros(n, dtype=torch.long) if batch is None else torch.as_tensor(batch)
    k = torch.arange(-N // 2, N // 2, dtype=torch.float64)
    E = [torch.exp(2j * np.pi * pos[:, a:a + 1] * k[None, :]) for a in range(d)]
    onehot = torch.nn.functional.one_hot(b, B).to(torch.complex128)
    letters = "pqr"[:d]
    expr = "ib,ic," + ",".join("i" + l for l in letters) + "->b" + letters + "c"
    return torch.einsum(expr, onehot, xc, *E)


def exact_forward_pos_grad(xhat, pos, batch, real_output, w):
    """d/dpos of sum_{i, cr} w[i, cr] Fr[i, cr] with the exact transform."""
    p = torch.tensor(np.asarray(pos, dtype=np.float32).astype(np.float64), requires_grad=True)
    y = ndft_forward_t(torch.as_tensor(np.asarray(xhat)).to(torch.complex128), p, batch)
    yr = y.real if real_output else torch.view_as_real(y).reshape(y.shape[0], -1)
    (yr * torch.as_tensor(np.asarray(w, dtype=np.float64))).sum().backward()
    return p.grad.numpy()


def exact_adjoint_pos_grad(x, pos, batch, B, N, real_output, dy):
    """d/dpos of <dy, y> (torch's convention: dy = dL/dRe y + i dL/dIm y) for y = the exact adjoint of x."""
    p = torch.tensor(np.asarray(pos, dtype=np.float32).astype(np.float64), requires_grad=True)
    y = ndft_adjoint_t(torch.as_tensor(np.asarray(x)).to(torch.complex128), p, batch, B, N)
    g = torch.as_tensor(np.asarray(dy)).reshape(y.shape)
    if real_output:
        loss = (y.real * g.real).sum()
    else:
        gc = g.to(torch.complex128)
        loss = (y.real * gc.real + y.imag * gc.imag).sum()
    loss.backward()
    return p.grad.numpy()


# ---- tests ------------------------------------------------------------------------------------------------------------

def rel(a, b):
    return float(np.linalg.norm(np.ravel(a - b)) / np.linalg.norm(np.ravel(b)))


def problem(rng, d, N, n, cols, complex_x, B):
    pos = (rng.random((n, d)) - 0.5).astype(np.float32)
    if B > 1:
        batch = np.sort(rng.integers(0, B, n)).astype(np.int64)
        batch[0], batch[-1] = 0, B - 1
    else:
        batch = None
    shape = (B,) + (N,) * d + cols
    xhat = rng.standard_normal(shape)
    if complex_x:
        xhat = xhat + 1j * rng.standard_normal(shape)
    return pos, batch, xhat


CASES = [  # d, N, n, cols, complex xhat, real_output, B
    (1, 32, 40, (), False, True, 1),
    (1, 32, 40, (2,), True, False, 2),
    (2, 16, 60, (), True, False, 1),
    (2, 16, 60, (3,), False, False, 3),
    (2, 16, 60, (2, 2), True, True, 1),
    (3, 8, 50, (), True, False, 1),
    (3, 8, 50, (2,), False, True, 2),
]


@pytest.mark.parametrize("d,N,n,cols,cx,ro,B", CASES)
def test_restatement_matches_exact_gradient_and_converges(d, N, n, cols, cx, ro, B):
    """The yardstick of the GPU tests: the window-derivative gather approaches the exact gradient as m grows."""
    rng = np.random.default_rng(10 * d + n + B)
    pos, batch, xhat = problem(rng, d, N, n, cols, cx, B)
    C = int(np.prod(cols)) if cols else 1
    w = rng.standard_normal((n, C if ro else 2 * C))
    exact = exact_forward_pos_grad(xhat, pos, batch, ro, w)
    errs = [rel(pos_grad(xhat, pos, batch, m, ro, w), exact) for m in (2, 4, 6, 8)]
    assert errs[0] < 5e-2 and errs[-1] < 1e-5, errs
    assert all(b < a for a, b in zip(errs, errs[1:])), errs


@pytest.mark.parametrize("d,N,cx,ro", [(1, 32, False, False), (2, 16, True, False), (2, 16, True, True), (3, 8, False, True)])
def test_adjoint_gradient_is_the_weighted_gather_of_the_forward(d, N, cx, ro):
    """y = adjoint(x, pos): dpos = the gather of F = forward(dy) weighted by the real view of x, real_output = !complex x."""
    rng = np.random.default_rng(d + 7)
    n, B = 40, 2
    pos = (rng.random((n, d)) - 0.5).astype(np.float32)
    batch = np.sort(rng.integers(0, B, n)).astype(np.int64)
    batch[0], batch[-1] = 0, B - 1
    x = rng.standard_normal((n, 2))
    if cx:
        x = x + 1j * rng.standard_normal((n, 2))
    dy = rng.standard_normal((B,) + (N,) * d + (2,))
    if not ro:
        dy = dy + 1j * rng.standard_normal(dy.shape)
    exact = exact_adjoint_pos_grad(x, pos, batch, B, N, ro, dy)
    got = pos_grad(dy, pos, batch, 8, not cx, real_columns(x, n))
    assert rel(got, exact) < 1e-5


def test_finite_difference_helper_agrees_with_the_gather():
    rng = np.random.default_rng(2)
    pos, _, xhat = problem(rng, 2, 16, 30, (), True, 1)
    w = rng.standard_normal((30, 2))
    g = grid_of(xhat, 2, 5)
    delta = rng.standard_normal((30, 2))
    h = 1e-6
    p = np.asarray(pos, dtype=np.float32).astype(np.float64)
    fd = ((interp_f64(g, p + h * delta, 5, False) - interp_f64(g, p - h * delta, 5, False)) * w).sum() / (2 * h)
    an = (grad_gather(g, pos, None, 5, False, w) * delta).sum()
    assert abs(fd - an) <= 1e-6 * np.abs(an)


def test_abi_entry_points_without_gpu():
    from torch_nfft_amd import _lib
    lib = _lib.load()
    for name in ("nfft_hip_forward_grad_workspace_bytes", "nfft_hip_forward_grad_points_planned"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    ok = _lib.Problem(3, 1000, 2, 1, 16, 4)
    bad = _lib.Problem(2, 10, 1, 1, 15, 3)
    assert lib.nfft_hip_forward_grad_workspace_bytes(ctypes.byref(bad), 0, 0) == -1
    p = ctypes.c_void_p(16)  # never dereferenced: the calls below fail before any device work
    assert lib.nfft_hip_forward_grad_points_planned(ctypes.byref(bad), p, p, 0, 0, p, p, p, 1 << 30, None) == _lib.EINVAL
    assert _lib.last_error().startswith("Input mismatch")
    assert lib.nfft_hip_forward_grad_points_planned(None, p, p, 0, 0, p, p, p, 1 << 30, None) == _lib.EINVAL
    # null or short workspace: refused before any device work (the partial gradients alone need 4 * 1000 * 3 floats)
    assert lib.nfft_hip_forward_grad_points_planned(ctypes.byref(ok), p, p, 1, 0, p, p, None, 1 << 30, None) == _lib.EWORKSPACE
    assert lib.nfft_hip_forward_grad_points_planned(ctypes.byref(ok), p, p, 1, 0, p, p, p, 4 * 1000 * 3 * 4, None) == _lib.EWORKSPACE
    assert _lib.last_error() == "workspace too small"


def test_operator_schema_and_cpu_rejection():
    import torch_nfft_amd  # noqa: F401  (registers the operators)
    op = torch.ops.torch_nfft._nfft_forward_grad_points
    assert str(op.default._schema) == ("torch_nfft::_nfft_forward_grad_points(Tensor pos, Tensor x, Tensor? batch, int m, "
                                       "int real_output, Tensor w) -> Tensor")
    with pytest.raises(RuntimeError):
        op(torch.zeros(4, 2), torch.zeros(1, 8, 8, dtype=torch.complex64), None, 3, 0, torch.zeros(4, 2))
