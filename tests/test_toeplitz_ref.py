"""The Toeplitz normal operator A^H W A on the CPU: its float64 restatement against the dense
float64 normal operator of oracle/ndft.py, and the host side of the new entry points (no GPU needed).

The restatement (steps 1-4 of section 7c, in the conventions of DESIGN.md section 2: centred spectra, frequency k at
index k + N/2, unnormalised FFTs, e^{+} in the adjoint, e^{-} in the forward transform) is what the GPU tests in
test_gpu_toeplitz.py compare the device against:

  1. t = adjoint(w, bandwidth 2N): [B, 2N, ..., 2N], lag n in [-N, N) at index n + N; lags with a component -N never
     occur in k - k' and are set to zero, which makes t Hermitian and K real;
  2. K[b, j] = M^-d sum_n t[b, n] e^{-2 pi i n.j / M},  M = 2N;
  3. g_j = sum_k' xhat_k' e^{-2 pi i k'.j / M}  (the forward FFT stage without the roll-off);
  4. y_k = sum_j K_j g_j e^{+2 pi i k.j / M}    (the adjoint FFT stage without the roll-off).
"""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from conftest import rel_l2
from oracle import ndft, nfft_ref

# the cases of the issue's table: d, N, m, points
CASES = [(2, 16, 2, 500), (2, 16, 3, 500), (2, 16, 4, 500), (2, 16, 6, 500), (2, 16, 8, 500), (1, 64, 4, 300),
         (3, 8, 4, 400), (2, 32, 4, 20000)]


# ----------------------------------------------------------------------------- the restatement

def lags_exact(w, pos, batch, N):
    """Step 1 with the exact NDFT: t [B, 2N, ..., 2N] complex128."""
    return ndft.ndft_adjoint(np.asarray(w, dtype=np.float64), pos, batch, N=2 * N)


def lags_nfft(w, pos, batch, N, m):
    """Step 1 as the device computes it: the algorithm's bandwidth-2N adjoint of the weights."""
    return nfft_ref.nfft_adjoint(np.asarray(w, dtype=np.float64), pos, batch, N=2 * N, m=m)


def kernel_from_lags(t):
    """Step 2: the -N lags zeroed, K [B, M, ..., M] complex128 (real up to rounding).  The device goes one step further
    and transforms the Hermitian part (t[-n] + conj t[n]) / 2 of the zeroed lags, so that its K is real exactly; that is
    the real part of this K, which is what the GPU tests compare against."""
    t = np.array(t, dtype=np.complex128)
    d = t.ndim - 1
    for a in range(d):
        idx = [slice(None)] * (d + 1)
        idx[a + 1] = 0
        t[tuple(idx)] = 0.0
    axes = tuple(range(1, d + 1))
    M = t.shape[1]
    return np.fft.fftn(np.fft.ifftshift(t, axes=axes), axes=axes) / float(M) ** d


def normal_apply(K, xhat):
    """Steps 3 and 4: xhat [B, N, ..., N, *cols] -> [B, N, ..., N, *cols] complex128."""
    K = np.asarray(K)
    xhat = np.asarray(xhat)
    d = K.ndim - 1
    B, M = K.shape[0], K.shape[1]
    N = M // 2
    cols = xhat.shape[1 + d:]
    x = xhat.reshape((B,) + (N,) * d + (-1,)).astype(np.complex128)
    kap = nfft_ref._band_index(N)
    band = (slice(None),) + np.ix_(*([kap] * d))
    G = np.zeros((B,) + (M,) * d + (x.shape[-1],), dtype=np.complex128)
    G[band] = x
    axes = tuple(range(1, d + 1))
    g = np.fft.fftn(G, axes=axes) * K[..., None]
    y = np.fft.ifftn(g, axes=axes) * float(M) ** d
    return y[band].reshape((B,) + (N,) * d + cols)


def normal_dense(xhat, w, pos, batch):
    """The dense float64 normal operator A^H W A xhat through oracle/ndft.py."""
    N = np.asarray(xhat).shape[1]
    f = ndft.ndft_forward(xhat, pos, batch)
    w = np.asarray(w, dtype=np.float64).reshape((-1,) + (1,) * (f.ndim - 1))
    return ndft.ndft_adjoint(f * w, pos, batch, N=N)


def cg_ref(K, b, iterations):
    """The conjugate-gradient iteration of nfft_inverse in float64 on the restatement (x0 = 0)."""
    x = np.zeros_like(b)
    r = b.copy()
    p = r.copy()
    rs = np.vdot(r, r).real
    res = []
    for _ in range(iterations):
        tp = normal_apply(K, p)
        alpha = rs / np.vdot(p, tp).real
        x = x + alpha * p
        r = r - alpha * tp
        rs_new = np.vdot(r, r).real
        res.append(np.sqrt(rs_new))
        p = r + (rs_new / rs) * p
        rs = rs_new
    return x, np.array(res)


def case_problem(d, N, n, seed):
    rng = np.random.default_rng(seed)
    pos = (rng.random((n, d)) - 0.5).astype(np.float32)
    w = 0.5 + rng.random(n)
    xhat = rng.standard_normal((1,) + (N,) * d) + 1j * rng.standard_normal((1,) + (N,) * d)
    return pos, w, xhat


# ----------------------------------------------------------------------------- restatement vs the dense operator

@pytest.mark.parametrize("d,N,m,n", CASES)
def test_restatement_against_dense_normal_operator(d, N, m, n):
    pos, w, xhat = case_problem(d, N, n, 7000 + 100 * d + N + m)
    dense = normal_dense(xhat, w, pos, None)
    # exact lags: the embedding itself is exact
    t = lags_exact(w, pos, None, N)
    K = kernel_from_lags(t)
    assert np.abs(K.imag).max() <= 1e-12 * np.abs(K.real).max()
    e_exact = rel_l2(normal_apply(K.real, xhat), dense)
    print("d=%d N=%d m=%d n=%d exact-t error %.2e" % (d, N, m, n, e_exact))
    assert e_exact <= 1e-12
    # lags from the algorithm's bandwidth-2N adjoint: the operator is no further off than those lags are
    tn = lags_nfft(w, pos, None, N, m)
    gap = rel_l2(tn, t)
    Kn = kernel_from_lags(tn)
    assert np.abs(Kn.imag).max() <= 1e-12 * np.abs(Kn.real).max()
    e_nfft = rel_l2(normal_apply(Kn.real, xhat), dense)
    print("            nfft-t error %.2e, gap of t %.2e, ratio %.2f" % (e_nfft, gap, e_nfft / gap))
    assert e_nfft <= gap


def test_restatement_is_selfadjoint_and_batched():
    rng = np.random.default_rng(5)
    d, N, n, B = 2, 8, 300, 3
    pos = (rng.random((n, d)) - 0.5).astype(np.float32)
    batch = np.sort(rng.integers(0, B, n)).astype(np.int64)
    batch[0], batch[-1] = 0, B - 1
    w = 0.5 + rng.random(n)
    K = kernel_from_lags(lags_exact(w, pos, batch, N)).real
    a = rng.standard_normal((B, N, N, 2)) + 1j * rng.standard_normal((B, N, N, 2))
    b = rng.standard_normal((B, N, N, 2)) + 1j * rng.standard_normal((B, N, N, 2))
    assert rel_l2(normal_apply(K, a), normal_dense(a, w, pos, batch)) <= 1e-12
    lhs, rhs = np.vdot(b, normal_apply(K, a)), np.vdot(normal_apply(K, b), a)
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs)
    assert np.vdot(a, normal_apply(K, a)).real >= 0.0


# ----------------------------------------------------------------------------- host side

NEW_SYMBOLS = ("nfft_hip_toeplitz_kernel_workspace_bytes", "nfft_hip_toeplitz_kernel",
               "nfft_hip_toeplitz_workspace_bytes", "nfft_hip_toeplitz_apply")


def test_library_exports_the_toeplitz_entry_points():
    from torch_nfft_amd import _lib
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert _lib.ABI_VERSION >= 5


def test_workspace_queries_reject_bad_problems():
    from torch_nfft_amd import _lib
    lib = _lib.load()
    for bad in [_lib.Problem(2, 0, 1, 1, 15, 1), _lib.Problem(4, 0, 1, 1, 16, 1), _lib.Problem(2, 0, 1, 1, 1, 1),
                _lib.Problem(1, 0, 1, 1, 0, 1)]:  # odd N, dim = 4, N < 2
        for f in (lib.nfft_hip_toeplitz_workspace_bytes, lib.nfft_hip_toeplitz_kernel_workspace_bytes):
            assert f(ctypes.byref(bad)) == -1
            assert _lib.last_error().startswith("Input mismatch")
    # the compute entry points validate before they touch the device
    ok = _lib.Problem(2, 0, 1, 1, 16, 1)
    assert lib.nfft_hip_toeplitz_apply(ctypes.byref(ok), None, None, 0, None, None, 0, None) == _lib.EINVAL
    assert _lib.last_error().startswith("Input mismatch")
    assert lib.nfft_hip_toeplitz_kernel(ctypes.byref(ok), None, None, None, 0, None) == _lib.EINVAL
    assert _lib.last_error().startswith("Input mismatch")


def test_operators_reject_cpu_tensors():
    import torch_nfft_amd as tn
    with pytest.raises(RuntimeError, match="torch_nfft._nfft_normal is currently only implemented for GPU tensors"):
        tn.nfft_normal(torch.zeros(1, 8, 8), torch.zeros(1, 16, 16))
    with pytest.raises(RuntimeError, match="torch_nfft._nfft_toeplitz_kernel is currently only implemented for GPU tensors"):
        tn.ops.nfft_toeplitz_kernel(torch.zeros(1, 16, 16, dtype=torch.complex64))
    with pytest.raises(RuntimeError, match="torch_nfft.nfft_adjoint is currently only implemented for GPU tensors"):
        tn.nfft_toeplitz_kernel(torch.zeros(5, 2))
    assert str(torch.ops.torch_nfft._nfft_toeplitz_kernel.default._schema) == \
        "torch_nfft::_nfft_toeplitz_kernel(Tensor t) -> Tensor"
    assert str(torch.ops.torch_nfft._nfft_normal.default._schema) == \
        "torch_nfft::_nfft_normal(Tensor kernel, Tensor x) -> Tensor"
    # no gradient into the kernel grid or its ingredients
    with pytest.raises(AssertionError, match="kernel requires grad"):
        tn.nfft_normal(torch.zeros(1, 8, 8), torch.zeros(1, 16, 16, requires_grad=True))
    with pytest.raises(AssertionError, match="pos requires grad"):
        tn.nfft_toeplitz_kernel(torch.zeros(5, 2, requires_grad=True))
    with pytest.raises(AssertionError, match="weights requires grad"):
        tn.nfft_toeplitz_kernel(torch.zeros(5, 2), weights=torch.ones(5, requires_grad=True))
    with pytest.raises(ValueError, match="weights must be real"):
        tn.nfft_toeplitz_kernel(torch.zeros(5, 2), weights=torch.ones(5, dtype=torch.complex64))


def test_python_signatures():
    import torch_nfft
    import torch_nfft_amd as tn
    assert str(inspect.signature(tn.nfft_toeplitz_kernel)) == "(pos, batch=None, weights=None, bandwidth=16, cutoff=3)"
    assert str(inspect.signature(tn.nfft_normal)) == "(x, kernel)"
    assert str(inspect.signature(tn.nfft_inverse)) == \
        "(y, pos, batch=None, bandwidth=16, cutoff=3, weights=None, iterations=10, x0=None)"
    for name in ("nfft_toeplitz_kernel", "nfft_normal", "nfft_inverse"):
        assert getattr(torch_nfft, name) is getattr(tn, name)
