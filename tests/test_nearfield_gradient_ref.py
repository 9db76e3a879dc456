"""CPU tests of the gradient of the fast summation with a regularised kernel (nfft_fastsum_nearfield_gradient, DESIGN.md
section 7e): the float64 restatement tests/nearfield_gradient_ref.py against the dense gradient, the host-side pieces of
torch_nfft_amd/nearfield.py against the restatement, the refusals, the C ABI's validation and the kernels' resources."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import nearfield_gradient_ref as ng
import nearfield_ref as nr
from conftest import rel_l2
from resource_usage import resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name,dim,n", [("one_over_modulus", 3, 120), ("logarithm", 2, 300)])
def test_float64_algorithm_against_dense_gradient(name, dim, n):
    """The algorithm's own error for the gradient in exact arithmetic (N = 32, p = 4, shared points in the ball).  Relative
    l2 against the dense gradient, recorded in DESIGN.md section 7e, with the unpaired plane l_a = -N/2 zeroed (what the
    product does) and kept:  3-D 1/r, 120 points 3.57e-4 / 3.41e-4;  2-D log r, 300 points 4.24e-4 / 3.68e-4.  Without
    the near part the gradient is wrong by O(1): 0.958 and 0.854."""
    rng = np.random.default_rng(41 + dim)
    N, p = 32, 4
    eps_B = max(1.0 / 16.0, p / N)
    pts = nr.ball_points(rng, n, dim, 0.25 - eps_B / 2)
    x = rng.standard_normal(n)
    ref = nr.Restatement(name, 1.0, p, p / N, eps_B)
    dense = ng.dense_gradient(name, 1.0, x, pts)
    G = ng.exact_algorithm_gradient(ref, N, x, pts)
    assert G.shape == dense.shape == (n, dim)
    err = rel_l2(G, dense)
    err_kept = rel_l2(ng.exact_algorithm_gradient(ref, N, x, pts, keep_nyquist=True), dense)
    near = ng.near_gradient(name, 1.0, ref.near_poly, ref.eps_I, x, pts)
    err_far_only = rel_l2(G - near, dense)
    print("float64 gradient", name, "rel_l2 vs dense %.3e (Nyquist plane kept %.3e), without the near part %.3e"
          % (err, err_kept, err_far_only))
    assert err < 1e-2 and err_kept < 1e-2
    assert err_far_only > 10 * err
    # the restatement's own transpose: <G x, v> = <x, G^T v> for the whole map
    v = rng.standard_normal((n, dim))
    lhs, rhs = (G * v).sum(), (x * ng.exact_algorithm_gradient_transpose(ref, N, v, pts)).sum()
    assert abs(lhs - rhs) <= 1e-10 * np.linalg.norm(G) * np.linalg.norm(v)


@pytest.mark.parametrize("p", [2, 3, 4, 6, 8])
@pytest.mark.parametrize("name", nr.NAMES)
def test_near_gradient_poly(name, p):
    """near_gradient_poly (Horner in u = (r / eps_I)^2) against T_I'(r) / r of the restatement: float64 autograd through
    Restatement.inner with the same a_k, and the closed form of the reference helper"""
    import torch_nfft_amd as tn
    kern = tn.RegularizedKernel(name, c=0.25, dim=2, bandwidth=64, p=p, device="cpu")
    assert kern.near_gradient_poly.dtype == torch.float64 and kern.near_gradient_poly.shape == (p - 1,)
    ref = nr.Restatement(name, 0.25, p, kern.eps_I, kern.eps_B)
    ref.near_poly = kern.near_poly.numpy().copy()
    r = torch.linspace(0.01, 1.0, 37, dtype=torch.float64) * kern.eps_I
    r.requires_grad_(True)
    dT, = torch.autograd.grad(ref.inner(r).sum(), r)
    want = (dT / r.detach()).numpy()
    u = (r.detach().numpy() / kern.eps_I) ** 2
    got = np.zeros_like(u)
    for a in reversed(kern.near_gradient_poly.tolist()):
        got = got * u + a
    assert rel_l2(got, want) <= 1e-12
    assert rel_l2(ng.inner_slope(kern.near_poly.numpy(), kern.eps_I, r.detach().numpy()), want) <= 1e-12


@pytest.mark.parametrize("name", nr.NAMES)
def test_kernel_slopes_against_autograd(name):
    """the eight closed forms K'(r) / r of the reference helper against autograd of the product's kernel expression"""
    import torch_nfft_amd as tn
    kern = tn.RegularizedKernel(name, c=0.03, dim=3, bandwidth=32, p=4, device="cpu")
    r = (torch.linspace(0.003, 0.997, 41, dtype=torch.float64) * kern.eps_I).requires_grad_(True)
    dK, = torch.autograd.grad(kern.kernel(r).sum(), r)
    want = (dK / r.detach()).numpy()
    got = ng.kernel_slope(name, r.detach().numpy(), 0.03)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert rel_l2(got, want) <= 1e-13


@pytest.mark.parametrize("name,dim,complex_x", [("one_over_modulus", 3, False), ("thinplate_spline", 2, True),
                                                ("laplacian_rbf", 1, False)])
def test_reference_transpose_is_the_adjoint(name, dim, complex_x):
    rng = np.random.default_rng(51)
    ref = nr.Restatement(name, 0.05, 4, 0.07, 0.0625)
    s, t = nr.ball_points(rng, 150, dim, 0.2), nr.ball_points(rng, 130, dim, 0.2)
    t[:10] = s[:10]
    sb, tb = np.sort(rng.integers(0, 2, 150)), np.sort(rng.integers(0, 2, 130))
    x, v = rng.standard_normal((150, 2)), rng.standard_normal((130, dim, 2))
    if complex_x:
        x, v = x + 1j * rng.standard_normal(x.shape), v + 1j * rng.standard_normal(v.shape)
    G = ng.near_gradient(name, 0.05, ref.near_poly, 0.07, x, s, t, sb, tb)
    Gt = ng.near_gradient_transpose(name, 0.05, ref.near_poly, 0.07, v, s, t, sb, tb)
    assert G.shape == v.shape and Gt.shape == x.shape and np.linalg.norm(G) > 0
    # (bilinear, no conjugation: the matrix is real)
    lhs, rhs = (G * v).sum(), (x * Gt).sum()
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), np.linalg.norm(G) * np.linalg.norm(v) * 1e-3)


def test_cpu_tensors_and_point_gradients_are_refused():
    import torch_nfft
    import torch_nfft_amd as tn
    assert torch_nfft.nfft_fastsum_nearfield_gradient is tn.nfft_fastsum_nearfield_gradient
    assert torch_nfft.nfft_nearfield_gradient is tn.nfft_nearfield_gradient
    assert torch_nfft.NfftNearfieldGradientFunction is tn.NfftNearfieldGradientFunction
    s = str(torch.ops.torch_nfft._nfft_nearfield_gradient.default._schema)
    assert s == ("torch_nfft::_nfft_nearfield_gradient(Tensor sources, Tensor targets, Tensor x, Tensor? source_batch, "
                 "Tensor? target_batch, int kernel, float c, float eps_I, float[] poly, bool transpose) -> Tensor")
    kern = tn.RegularizedKernel("one_over_modulus", dim=2, bandwidth=32, device="cpu")
    pts = torch.zeros(5, 2)
    msg = "torch_nfft._nfft_nearfield_gradient is currently only implemented for GPU tensors"
    with pytest.raises(RuntimeError, match=msg):
        tn.nfft_nearfield_gradient(torch.zeros(5), kern, pts)
    for transpose, x in ((False, torch.zeros(5)), (True, torch.zeros(5, 2))):
        with pytest.raises(RuntimeError, match=msg):
            tn.ops.nfft_nearfield_gradient(pts, pts, x, None, None, 0, 1.0, 0.25, [1.0, 2.0], transpose)
    for fn in (tn.nfft_fastsum_nearfield_gradient, tn.nfft_nearfield_gradient):
        for arg in ("sources", "targets", "source_batch"):
            t = {"sources": pts, "targets": pts.clone(), "source_batch": None}
            if arg == "source_batch":
                t[arg] = torch.zeros(5, requires_grad=True)
            else:
                t[arg] = t[arg].clone().requires_grad_(True)
            with pytest.raises(AssertionError, match=arg):
                fn(torch.zeros(5), kern, t["sources"], t["targets"], t["source_batch"], None)


def test_one_term_is_refused():
    import torch_nfft_amd as tn
    kern = tn.RegularizedKernel("logarithm", dim=2, bandwidth=32, p=1, device="cpu")
    assert kern.near_gradient_poly.shape == (0,)
    pts = torch.zeros(5, 2)
    with pytest.raises(ValueError, match="p >= 2"):
        tn.nfft_fastsum_nearfield_gradient(torch.zeros(5), kern, pts)
    with pytest.raises(ValueError, match="p >= 2"):
        tn.nfft_nearfield_gradient(torch.zeros(5), kern, pts)


def test_c_abi_validation_without_gpu():
    from torch_nfft_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 7 and lib.nfft_hip_abi_version() == 7
    assert "nfft_hip_nearfield_gradient" in _lib.SYMBOLS and "nfft_hip_nearfield_gradient_workspace_bytes" in _lib.SYMBOLS

    def problem(**kw):
        f = dict(dim=3, kernel=0, poly_terms=4, cells_per_axis=8, num_sources=1000, num_targets=900, num_columns=2,
                 batch_size=1, c=1.0, eps_I=1.0 / 16.0)
        f.update(kw)
        return _lib.NearfieldProblem(**f)

    ok = problem()
    assert lib.nfft_hip_nearfield_gradient_workspace_bytes(ctypes.byref(ok)) == lib.nfft_hip_nearfield_workspace_bytes(ctypes.byref(ok))
    assert lib.nfft_hip_nearfield_gradient_workspace_bytes(ctypes.byref(problem(poly_terms=2))) > 0
    for bad in (problem(dim=0), problem(dim=4), problem(kernel=8), problem(kernel=-1), problem(poly_terms=0),
                problem(poly_terms=1), problem(poly_terms=9), problem(cells_per_axis=9), problem(eps_I=0.0),
                problem(num_targets=-1), problem(batch_size=0), problem(kernel=7, c=0.0)):
        assert lib.nfft_hip_nearfield_gradient_workspace_bytes(ctypes.byref(bad)) == -1
        assert _lib.last_error().startswith("Input mismatch")
    null = ctypes.c_void_p(0)
    one = ctypes.c_void_p(256)  # (never dereferenced: the checks come first)
    gpoly = (ctypes.c_double * 8)(1.0, 2.0, 3.0)
    gp = ctypes.cast(gpoly, ctypes.c_void_p)

    def call(q, transpose, poly, ws=null, nbytes=0):
        return lib.nfft_hip_nearfield_gradient(ctypes.byref(q), transpose, poly, one, one, one, one, one, one, one, ws, nbytes, null)

    for transpose in (0, 1):
        assert call(ok, transpose, gp) == _lib.EWORKSPACE
        assert call(ok, transpose, gp, one, 8) == _lib.EWORKSPACE
        assert call(problem(poly_terms=1), transpose, gp) == _lib.EINVAL
        assert call(problem(dim=4), transpose, gp) == _lib.EINVAL
        assert call(problem(kernel=9), transpose, gp) == _lib.EINVAL
        assert call(ok, transpose, null) == _lib.EINVAL
        # nothing to do: no launch, no workspace needed
        assert call(problem(num_targets=0), transpose, gp) == _lib.OK
        assert call(problem(num_columns=0), transpose, gp) == _lib.OK
    assert call(ok, 2, gp) == _lib.EINVAL
    gpoly[1] = float("nan")
    assert call(ok, 0, gp) == _lib.EINVAL and _lib.last_error().startswith("Input mismatch")


def test_pair_kernel_resource_usage():
    """Every instantiation <KERNEL, CC, PT, MODE> of the gradient pair kernel: no scratch and no spills of either kind.
    (VGPRs and occupancies are recorded in DESIGN.md section 7e, not gated.)"""
    usage = resource_usage("nearfield_grad.hip")
    pat = re.compile(r"nearfield_grad_kernelILi(\d)ELi(\d)ELi(\d)ELi(\d)EE")
    by = {}
    for name, u in usage.items():
        m = pat.search(name)
        if m:
            by[tuple(int(g) for g in m.groups())] = u
    assert set(by) == {(k, cc, pt, mode) for k in range(8) for cc in (1, 2, 4) for pt in (4, 8) for mode in (0, 1)}
    for key, u in sorted(by.items()):
        print(key, "VGPRs %d occupancy %d LDS %d" % (u["VGPRs"], u["Occupancy"], u["LDS Size"]))
        assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (key, u)
