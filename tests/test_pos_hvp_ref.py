"""CPU tests of the second derivatives of nfft_forward / nfft_adjoint with respect to the points, and the float64
restatement the GPU tests compare against.

G(pos, xhat, w)[i, a] = sum_cr w[i, cr] d Fr[i, cr] / d pos[i, a] is the first-order point gradient of both transforms
(test_pos_grad_ref.py).  For an upstream v [n, dim] its backward is
    dw[i, cr]   = sum_a v[i, a] d Fr[i, cr] / d pos[i, a]
    dpos[i, b]  = sum_cr w[i, cr] sum_a v[i, a] d^2 Fr[i, cr] / d pos[i, a] d pos[i, b]
    dxhat[k, c] = sum_i omega[i, c] sum_a v[i, a] (2 pi i k_a) exp(+2 pi i k.pos_i)
dw and dpos restated as the library evaluates them (the window's first and second derivatives on the deconvolved, FFT'd
grid), dxhat as the spectral multipliers of the exact adjoint.  The exact values come from double autograd of a dense
float64 NDFT in torch.
"""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

from oracle import nfft_ref
from test_pos_grad_ref import grid_of, ndft_adjoint_t, ndft_forward_t, problem, real_columns, rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Relative L2 tolerance per cutoff m of a second derivative computed in fp32 against the exact one (the GPU tests): the
# float64 algorithm's own gap for dpos (test_gaps_per_cutoff; largest of dims 1-3: 2.2, 0.17, 1.7e-2, 1.7e-3, 1.9e-4,
# 2.2e-5, 2.5e-6, 3.0e-7 for m = 1 .. 8) times about 3, with an fp32 floor of 2e-5.  m = 1, 2 are left out: at gaps of
# 2.2 and 0.17 a relative tolerance checks nothing (the GPU tests compare those cutoffs with the restatement, TR2).
TE2 = {3: 5e-2, 4: 5e-3, 5: 6e-4, 6: 7e-5, 7: 2e-5, 8: 2e-5}


def hvp_gather(g, pos, batch, m, real_output, w, v):
    """(dw [n, Cr], dpos [n, d]) float64 from the grid g of grid_of(); w [n, Cr], v [n, d]."""
    pos = np.asarray(pos)
    n, d = pos.shape
    C, M = g.shape[1], g.shape[2]
    N = M // 2
    W = 2 * m + 2
    c = 0.75 * np.pi / m
    bvec = np.zeros(n, np.int64) if batch is None else np.asarray(batch).astype(np.int64)
    shift, psi = nfft_ref.window_taps(pos, N, m)
    p = np.asarray(pos, dtype=np.float32).astype(np.float64)
    t = (p * M - shift)[:, :, None] - np.arange(W, dtype=np.float64)[None, None, :]
    v = np.asarray(v, dtype=np.float64).reshape(n, d)
    Q = np.zeros((n, C), np.complex128)      # sum g psi (v.t)
    S0 = np.zeros((n, C), np.complex128)     # sum g psi
    T = np.zeros((n, d, C), np.complex128)   # sum g psi t_b (v.t)
    for ls in itertools.product(range(W), repeat=d):
        idx = tuple((shift[:, a] + ls[a] + M) % M for a in range(d))
        vals = np.stack([g[(bvec, cc) + idx] for cc in range(C)], axis=1)
        wt = np.ones(n)
        for a in range(d):
            wt = wt * psi[:, a, ls[a]]
        tl = np.stack([t[:, a, ls[a]] for a in range(d)], axis=1)  # [n, d]
        q = (v * tl).sum(1)
        S0 += (wt)[:, None] * vals
        Q += (wt * q)[:, None] * vals
        T += (wt * q)[:, None, None] * tl[:, :, None] * vals[:, None, :]
    dk = -2.0 * c * M
    dW = dk * Q
    H = dk * dk * T + dk * M * v[:, :, None] * S0[:, None, :]  # sum_a v_a d^2 F / d p_a d p_b, [n, d, C]
    if real_output:
        dWr, Hr = dW.real, H.real
    else:
        dWr = np.stack([dW.real, dW.imag], axis=-1).reshape(n, 2 * C)
        Hr = np.stack([H.real, H.imag], axis=-1).reshape(n, d, 2 * C)
    w = np.asarray(w, dtype=np.float64).reshape(n, -1)
    return dWr, np.einsum("ibc,ic->ib", Hr, w)


def spectral_dxhat(xhat_shape, complex_xhat, pos, batch, real_output, w, v):
    """dxhat = sum_a 2 pi i k_a adjoint(pos, omega v_a) with the exact float64 adjoint, xhat's shape (real part for real
    xhat)."""
    pos_t = torch.tensor(np.asarray(pos, dtype=np.float32).astype(np.float64))
    n, d = pos_t.shape
    B, N = xhat_shape[0], xhat_shape[1]
    w = np.asarray(w, dtype=np.float64).reshape(n, -1)
    omega = w if real_output else w[:, 0::2] + 1j * w[:, 1::2]
    k = np.arange(-N // 2, N // 2)
    out = 0
    for a in range(d):
        u = torch.as_tensor(omega * np.asarray(v, dtype=np.float64)[:, a:a + 1]).to(torch.complex128)
        y = ndft_adjoint_t(u, pos_t, batch, B, N).numpy()  # [B, N^d, C]
        ka = k.reshape((1,) + tuple(N if b == a else 1 for b in range(d)) + (1,))
        out = out + 2j * np.pi * ka * y
    out = out.reshape(xhat_shape)
    return out if complex_xhat else out.real


def exact_g_backward(xhat, pos, batch, real_output, w, v):
    """(dxhat, dw, dpos) of <v, G(pos, xhat, w)> with the exact transform, by double autograd (torch's conventions)."""
    p = torch.tensor(np.asarray(pos, dtype=np.float32).astype(np.float64), requires_grad=True)
    xh = torch.as_tensor(np.asarray(xhat)).clone()
    xh = (xh.to(torch.complex128) if xh.is_complex() else xh.to(torch.float64)).requires_grad_(True)
    wt = torch.tensor(np.asarray(w, dtype=np.float64)).requires_grad_(True)
    y = ndft_forward_t(xh.to(torch.complex128), p, batch)
    yr = y.real if real_output else torch.view_as_real(y).reshape(y.shape[0], -1)
    (g,) = torch.autograd.grad((yr * wt).sum(), p, create_graph=True)
    dx, dw, dp = torch.autograd.grad((g * torch.as_tensor(np.asarray(v, dtype=np.float64))).sum(), (xh, wt, p))
    return dx.detach().numpy(), dw.detach().numpy(), dp.detach().numpy()


def restatement(xhat, pos, batch, m, real_output, w, v):
    d = np.asarray(pos).shape[1]
    dw, dp = hvp_gather(grid_of(xhat, d, m), pos, batch, m, real_output, w, v)
    dx = spectral_dxhat(np.shape(xhat), np.iscomplexobj(xhat), pos, batch, real_output, w, v)
    return dx, dw, dp


# ---- tests ------------------------------------------------------------------------------------------------------------

CASES = [  # d, N, n, cols, complex xhat, real_output, B
    (1, 32, 40, (), False, True, 1),
    (1, 32, 40, (2,), True, False, 2),
    (2, 16, 50, (), True, False, 1),
    (2, 16, 50, (3,), False, False, 3),
    (2, 16, 50, (2,), True, True, 1),
    (3, 8, 40, (), True, False, 1),
    (3, 8, 40, (2,), False, True, 2),
]


@pytest.mark.parametrize("d,N,n,cols,cx,ro,B", CASES)
def test_restatement_matches_double_autograd_and_converges(d, N, n, cols, cx, ro, B):
    """The yardstick of the GPU tests: dw and dpos approach the exact second derivatives as m grows; dxhat (spectral
    multipliers of the exact adjoint) is exact."""
    rng = np.random.default_rng(100 + 10 * d + n + B)
    pos, batch, xhat = problem(rng, d, N, n, cols, cx, B)
    C = int(np.prod(cols)) if cols else 1
    w = rng.standard_normal((n, C if ro else 2 * C))
    v = rng.standard_normal((n, d))
    ex_dx, ex_dw, ex_dp = exact_g_backward(xhat, pos, batch, ro, w, v)
    errs_w, errs_p = [], []
    for m in (2, 4, 6, 8):
        dw, dp = hvp_gather(grid_of(xhat, d, m), pos, batch, m, ro, w, v)
        errs_w.append(rel(dw, ex_dw))
        errs_p.append(rel(dp, ex_dp))
    assert errs_w[0] < 0.1 and errs_w[-1] < 1e-5, errs_w
    assert errs_p[0] < 0.2 and errs_p[-1] < 1e-5, errs_p
    assert all(b < a for a, b in zip(errs_w, errs_w[1:])), errs_w
    assert all(b < a for a, b in zip(errs_p, errs_p[1:])), errs_p
    dx = spectral_dxhat(np.shape(xhat), cx, pos, batch, ro, w, v)
    assert rel(dx, ex_dx) < 1e-12


def test_gaps_per_cutoff():
    """The per-m gaps of the float64 algorithm, dims 1-3: what TE2 is derived from, with room for fp32."""
    for d, N, n in ((3, 8, 30), (2, 16, 40), (1, 32, 40)):
        rng = np.random.default_rng(5)
        pos, batch, xhat = problem(rng, d, N, n, (), True, 1)
        w = rng.standard_normal((n, 2))
        v = rng.standard_normal((n, d))
        _, _, ex_dp = exact_g_backward(xhat, pos, batch, False, w, v)
        for m in range(3, 9):
            _, dp = hvp_gather(grid_of(xhat, d, m), pos, batch, m, False, w, v)
            assert rel(dp, ex_dp) < TE2[m] / 2, (d, m, rel(dp, ex_dp))


def test_abi_entry_points_without_gpu():
    from torch_nfft_amd import _lib
    lib = _lib.load()
    for name in ("nfft_hip_forward_grad_points_backward_workspace_bytes", "nfft_hip_forward_grad_points_backward_planned"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    ok = _lib.Problem(3, 1000, 2, 1, 16, 4)
    bad = _lib.Problem(2, 10, 1, 1, 15, 3)
    assert lib.nfft_hip_forward_grad_points_backward_workspace_bytes(ctypes.byref(bad), 0, 0) == -1
    p = ctypes.c_void_p(16)  # never dereferenced: the calls below fail before any device work
    f = lib.nfft_hip_forward_grad_points_backward_planned
    assert f(ctypes.byref(bad), p, p, 0, 0, p, p, p, p, p, p, 1 << 30, None) == _lib.EINVAL
    assert _lib.last_error().startswith("Input mismatch")
    assert f(None, p, p, 0, 0, p, p, p, p, p, p, 1 << 30, None) == _lib.EINVAL
    assert f(ctypes.byref(ok), p, p, 1, 0, p, p, p, p, p, None, 1 << 30, None) == _lib.EWORKSPACE
    assert f(ctypes.byref(ok), p, p, 1, 0, p, p, p, p, p, p, 4096, None) == _lib.EWORKSPACE
    assert _lib.last_error() == "workspace too small"
    assert f(ctypes.byref(ok), p, p, 1, 0, p, None, p, p, p, p, 1 << 30, None) == _lib.EINVAL  # no v
    # nothing asked for: nothing to do
    assert f(ctypes.byref(ok), p, p, 1, 0, p, p, None, None, None, None, 0, None) == _lib.OK
    need = lib.nfft_hip_forward_grad_points_backward_workspace_bytes(ctypes.byref(ok), 1, 0)
    assert need >= lib.nfft_hip_forward_grad_workspace_bytes(ctypes.byref(ok), 1, 0)


def test_operator_schema_and_cpu_rejection():
    import torch_nfft_amd  # noqa: F401  (registers the operators)
    op = torch.ops.torch_nfft._nfft_forward_grad_points_backward
    assert str(op.default._schema) == (
        "torch_nfft::_nfft_forward_grad_points_backward(Tensor pos, Tensor xhat, Tensor? batch, int m, int real_output, "
        "Tensor w, Tensor v, int need_xhat, int need_w, int need_pos) -> (Tensor, Tensor, Tensor)")
    with pytest.raises(RuntimeError, match="only implemented for GPU tensors"):
        op(torch.zeros(4, 2), torch.zeros(1, 8, 8, dtype=torch.complex64), None, 3, 0, torch.zeros(4, 2),
           torch.zeros(4, 2), 1, 1, 1)


# ---- resource usage of the second-order gather --------------------------------------------------------------------

def test_hvp_gather_resource_usage():
    """Every instantiation of interp_hvp_kernel: no scratch, no VGPR spills, and the occupancy of interp_grad_kernel with
    the same <DIM, W, WIDE> except one wave less for the three kernels GatherCfg::WPE_HVP names.  SGPR spills (into VGPR
    lanes, no memory) only for 2-D m = 1, 2."""
    from resource_usage import resource_usage
    usage = resource_usage("interp_grad.hip")
    pg = re.compile(r"interp_grad_kernelILi(\d)ELi(\d+)ELb([01])ELb0EE")
    ph = re.compile(r"interp_hvp_kernelILi(\d)ELi(\d+)ELb([01])EE")
    grad, hvp = {}, {}
    for name, u in usage.items():
        for pat, into in ((pg, grad), (ph, hvp)):
            mm = pat.search(name)
            if mm:
                into[(int(mm.group(1)), int(mm.group(2)), mm.group(3))] = u
    assert len(hvp) == 32 and set(hvp) == set(grad)
    lower = {(1, 18, "0"), (2, 18, "0"), (3, 6, "0")}
    for k, u in hvp.items():
        assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0, (k, u)
        assert u["SGPRs Spill"] == 0 or k[:2] in ((2, 4), (2, 6)) and u["SGPRs Spill"] <= 1, (k, u)
        assert u["Occupancy"] >= grad[k]["Occupancy"] - (1 if k in lower else 0), (k, u["Occupancy"], grad[k]["Occupancy"])


def test_derivative_spreading_resource_usage():
    """spread_kernel<DIM, W, DERIV = true>: no scratch, no VGPR spills and the occupancy of the plain spreading kernel of the
    same <DIM, W>.  The 3-D kernels from m = 5 on keep some SGPRs in VGPR lanes (no memory)."""
    from resource_usage import resource_usage
    usage = resource_usage("spread.hip")
    pat = re.compile(r"spread_kernelILi(\d)ELi(\d+)ELb([01])EE")
    by = {}
    for name, u in usage.items():
        mm = pat.search(name)
        if mm:
            by[(int(mm.group(1)), int(mm.group(2)), mm.group(3))] = u
    deriv = [k for k in by if k[2] == "1"]
    assert len(deriv) == 24 and len(by) == 48
    for k in deriv:
        u, base = by[k], by[k[:2] + ("0",)]
        assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0, (k, u)
        assert u["SGPRs Spill"] == 0 or k[0] == 3 and k[1] >= 10 and u["SGPRs Spill"] <= 16, (k, u)
        assert u["Occupancy"] >= base["Occupancy"], (k, u["Occupancy"], base["Occupancy"])
