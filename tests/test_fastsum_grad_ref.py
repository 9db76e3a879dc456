"""CPU tests of the gradient of nfft_fastsum with respect to its points.

The derivation, checked in float64 with exact transforms: for y_i = sum_j K(s_j - t_i) x_j, K(z) = sum_l c_l e^{2 pi i l.z},
and the loss <dy, y> (torch's convention; real parts for a real x),
    dtargets = forward_grad_points(targets, band = c A_s(x), w = real view of dy)
    dsources = forward_grad_points(sources, conj(c) A_t(dy), w = real view of x)
with real_output = !complex x in both, for any coefficient array (test_pos_grad_ref: the exact gradient of the forward
transform).  Also the C ABI and the operator schemas without a device, and the resource usage of the value-writing gather.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import test_pos_grad_ref as ref
from resource_usage import resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dense_fastsum_grads(x, c, src, tgt, dy):
    """(dsources, dtargets) of <dy, y> by torch autograd of the dense float64 trigonometric sum."""
    N, d = c.shape[0], c.ndim
    k = np.stack(np.meshgrid(*([np.arange(-N // 2, N // 2)] * d), indexing="ij"), -1).reshape(-1, d)
    kt = torch.tensor(k, dtype=torch.float64)
    s = torch.tensor(src, dtype=torch.float64, requires_grad=True)
    t = torch.tensor(tgt, dtype=torch.float64, requires_grad=True)
    ct = torch.tensor(c.reshape(-1).astype(np.complex128))
    K = torch.exp(-2j * np.pi * (t @ kt.T)) @ (ct[:, None] * torch.exp(2j * np.pi * (s @ kt.T)).T)
    y = K @ torch.tensor(x.astype(np.complex128))
    g = torch.tensor(dy.astype(np.complex128))
    loss = (y.real * g.real + y.imag * g.imag).sum() if np.iscomplexobj(x) else (y.real * g.real).sum()
    loss.backward()
    return s.grad.numpy(), t.grad.numpy()


@pytest.mark.parametrize("d,N", [(1, 16), (2, 8), (3, 4)])
@pytest.mark.parametrize("complex_x", [False, True], ids=["real-x", "complex-x"])
@pytest.mark.parametrize("complex_c", [False, True], ids=["real-c", "complex-c"])
def test_derivation_is_exact(d, N, complex_x, complex_c):
    rng = np.random.default_rng(100 * d + 10 * complex_x + complex_c)
    ns, nt, C = 17, 13, 2
    # (exact_forward_pos_grad rounds the points to float32: take them as float32 from the start)
    src = (rng.random((ns, d)) * 0.5 - 0.25).astype(np.float32).astype(np.float64)
    tgt = (rng.random((nt, d)) * 0.5 - 0.25).astype(np.float32).astype(np.float64)
    x = rng.standard_normal((ns, C)) + (1j * rng.standard_normal((ns, C)) if complex_x else 0)
    dy = rng.standard_normal((nt, C)) + (1j * rng.standard_normal((nt, C)) if complex_x else 0)
    c = rng.standard_normal((N,) * d) + (1j * rng.standard_normal((N,) * d) if complex_c else 0)
    es, et = dense_fastsum_grads(x, c, src, tgt, dy)
    ct = torch.tensor(c.astype(np.complex128)).reshape((1,) + c.shape + (1,))
    st, tt = torch.tensor(src), torch.tensor(tgt)
    band = ct * ref.ndft_adjoint_t(torch.tensor(x.astype(np.complex128)), st, None, 1, N)
    h = ct.conj() * ref.ndft_adjoint_t(torch.tensor(dy.astype(np.complex128)), tt, None, 1, N)
    dt = ref.exact_forward_pos_grad(band.numpy(), tgt, None, not complex_x, ref.real_columns(dy, nt))
    ds = ref.exact_forward_pos_grad(h.numpy(), src, None, not complex_x, ref.real_columns(x, ns))
    assert ref.rel(dt, et) < 1e-10 and ref.rel(ds, es) < 1e-10


def test_abi_entry_points_without_gpu():
    from torch_nfft_amd import _lib
    lib = _lib.load()
    for name in ("nfft_hip_forward_value_grad_points_planned", "nfft_hip_fastsum_band", "nfft_hip_fastsum_band_planned",
                 "nfft_hip_fastsum_grad_workspace_bytes", "nfft_hip_fastsum_backward_planned"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    ok = _lib.Problem(3, 1000, 2, 1, 16, 4)
    bad = _lib.Problem(2, 10, 1, 1, 15, 3)
    p = ctypes.c_void_p(16)  # never dereferenced: the calls below fail before any device work
    f = ctypes.c_void_p(16)
    # the value-writing gradient gather
    assert lib.nfft_hip_forward_value_grad_points_planned(ctypes.byref(bad), p, p, 0, 0, f, p, f, p, 1 << 30, None) == _lib.EINVAL
    assert _lib.last_error().startswith("Input mismatch")
    assert lib.nfft_hip_forward_value_grad_points_planned(ctypes.byref(ok), p, p, 1, 0, f, None, f, p, 1 << 30, None) == _lib.EINVAL
    assert lib.nfft_hip_forward_value_grad_points_planned(ctypes.byref(ok), p, p, 1, 0, f, p, f, None, 1 << 30, None) == _lib.EWORKSPACE
    assert lib.nfft_hip_forward_value_grad_points_planned(ctypes.byref(ok), p, p, 1, 0, f, p, f, p, 4 * 1000 * 3 * 4, None) == _lib.EWORKSPACE
    # the band-returning fast summation: a null band, a bad problem
    assert lib.nfft_hip_fastsum_band_planned(ctypes.byref(ok), p, ctypes.byref(ok), p, p, 0, p, 0, p, None, p, 1 << 30, None) == _lib.EINVAL
    assert lib.nfft_hip_fastsum_band(ctypes.byref(bad), p, None, ctypes.byref(bad), p, None, p, 0, p, 0, p, p, p, 1 << 30, None) == _lib.EINVAL
    # the backward
    assert lib.nfft_hip_fastsum_grad_workspace_bytes(ctypes.byref(bad), ctypes.byref(bad), 0) == -1
    assert lib.nfft_hip_fastsum_grad_workspace_bytes(None, ctypes.byref(ok), 0) == -1
    args = lambda ws, nbytes: (p, 0, p, p, 0, p, p, f, f, ws, nbytes, None)  # noqa: E731
    assert lib.nfft_hip_fastsum_backward_planned(ctypes.byref(bad), p, ctypes.byref(bad), p, p, *args(p, 1 << 30)[1:]) == _lib.EINVAL
    assert _lib.last_error().startswith("Input mismatch")
    other = _lib.Problem(3, 1000, 3, 1, 16, 4)  # another column count
    assert lib.nfft_hip_fastsum_backward_planned(ctypes.byref(ok), p, ctypes.byref(other), p, p, *args(p, 1 << 30)[1:]) == _lib.EINVAL
    assert lib.nfft_hip_fastsum_backward_planned(ctypes.byref(ok), None, ctypes.byref(ok), p, p, *args(p, 1 << 30)[1:]) == _lib.EINVAL
    # null or short workspace: refused before any route makes its rocFFT plans (the grid H alone is 2 * 16^3 * 8 bytes)
    assert lib.nfft_hip_fastsum_backward_planned(ctypes.byref(ok), p, ctypes.byref(ok), p, p, *args(None, 1 << 30)[1:]) == _lib.EWORKSPACE
    assert lib.nfft_hip_fastsum_backward_planned(ctypes.byref(ok), p, ctypes.byref(ok), p, p, *args(p, 2 * 16 ** 3 * 8)[1:]) == _lib.EWORKSPACE
    assert _lib.last_error() == "workspace too small"


def test_operator_schemas_and_cpu_rejection():
    import torch_nfft_amd  # noqa: F401  (registers the operators)
    band = torch.ops.torch_nfft._nfft_fastsum_band
    bwd = torch.ops.torch_nfft._nfft_fastsum_backward
    assert str(band.default._schema) == (
        "torch_nfft::_nfft_fastsum_band(Tensor sources, Tensor targets, Tensor x, Tensor coeffs, Tensor? source_batch, "
        "Tensor? target_batch, int m) -> (Tensor, Tensor)")
    assert str(bwd.default._schema) == (
        "torch_nfft::_nfft_fastsum_backward(Tensor sources, Tensor targets, Tensor x, Tensor dy, Tensor coeffs, "
        "Tensor? band, Tensor? source_batch, Tensor? target_batch, int m, int need_x, int need_sources, int need_targets) "
        "-> (Tensor, Tensor, Tensor)")
    s, x, c = torch.zeros(4, 2), torch.zeros(4, 1), torch.zeros(8, 8)
    with pytest.raises(RuntimeError, match="only implemented for GPU tensors"):
        band(s, s, x, c, None, None, 3)
    with pytest.raises(RuntimeError, match="only implemented for GPU tensors"):
        bwd(s, s, x, x, c, None, None, None, 3, 1, 1, 1)


# ---- resource usage of the value-writing gather ---------------------------------------------------------------------


def test_value_gather_resource_usage():
    """Every instantiation of the value-writing gather: no scratch, no VGPR spills, and at least the occupancy of the
    gradient-only kernel with the same <DIM, W, WIDE>.  SGPR spills (into VGPR lanes, no memory) only where the occupancy
    would drop without them: the 2-D m = 2 kernel (lane_gather.h GatherCfg::WPE_VALUE)."""
    usage = resource_usage("interp_grad.hip")
    # mangled: ...interp_grad_kernelILi<DIM>ELi<W>ELb<WIDE>ELb<VALUE>EE...
    pat = re.compile(r"interp_grad_kernelILi(\d)ELi(\d+)ELb([01])ELb([01])EE")
    by = {}
    for name, u in usage.items():
        m = pat.search(name)
        if m:
            by[(int(m.group(1)), int(m.group(2)), m.group(3), m.group(4))] = u
    values = [k for k in by if k[3] == "1"]
    assert len(values) == 32 and len(by) == 64  # dims 1-3 x m 1-8, the wide 3-D tiling too
    for k in values:
        u, base = by[k], by[k[:3] + ("0",)]
        assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0, (k, u)
        assert u["SGPRs Spill"] == 0 or k[:2] == (2, 6) and u["SGPRs Spill"] <= 6, (k, u)
        assert u["Occupancy"] >= base["Occupancy"], (k, u["Occupancy"], base["Occupancy"])
