"""CPU tests of the regularised kernels of nfft_fastsum_nearfield (torch_nfft_amd/nearfield.py) against the independent
float64 restatement tests/nearfield_ref.py, of the algorithm's own error and of the host-side checks."""
import ctypes

import numpy as np
import pytest
import torch

import nearfield_ref as nr
from conftest import rel_l2

N_PIECES = 32


def _scaled_derivatives(fn, r0, h, p):
    """[h^j fn^(j)(r0) for j < p] by autograd in float64"""
    r = torch.tensor(float(r0), dtype=torch.float64, requires_grad=True)
    y = fn(r)
    out = []
    for j in range(p):
        out.append(float(y.detach()) * h ** j)
        if j + 1 < p:
            y, = torch.autograd.grad(y, r, create_graph=True)
    return np.array(out)


def _check_pieces(k, p, eps_I, eps_B):
    """k: an object with kernel / inner / boundary / __call__ (the product's RegularizedKernel or the restatement).
    Derivatives of order j are compared after scaling with (width of the piece)^j, relative 1e-8 to the largest scaled
    derivative of K at that join: that is the size of the terms the matching conditions add up."""
    r = torch.linspace(eps_I, 0.5 - eps_B, 57, dtype=torch.float64)
    assert torch.equal(k(r), k.kernel(r))
    # inner join
    dK = _scaled_derivatives(k.kernel, eps_I, eps_I, p)
    dT = _scaled_derivatives(k.inner, eps_I, eps_I, p)
    assert np.abs(dT - dK).max() <= 1e-8 * np.abs(dK).max(), (dT, dK)
    # boundary join and the flat end at 1/2
    left = 0.5 - eps_B
    dK = _scaled_derivatives(k.kernel, left, eps_B, p)
    dB = _scaled_derivatives(k.boundary, left, eps_B, p)
    assert np.abs(dB - dK).max() <= 1e-8 * np.abs(dK).max(), (dB, dK)
    dE = _scaled_derivatives(k.boundary, 0.5, eps_B, p)
    assert np.abs(dE[1:]).max(initial=0.0) <= 1e-8 * np.abs(dK).max(), dE
    # the pieces meet in K_R, and the corners of the cube carry the value at 1/2
    probe = torch.tensor([0.0, 0.5 * eps_I, left + 0.5 * eps_B, 0.5, 0.7], dtype=torch.float64)
    v = k(probe)
    assert float(v[0]) == pytest.approx(float(k.inner(probe[:1])), rel=1e-14)
    assert float(v[1]) == pytest.approx(float(k.inner(probe[1:2])), rel=1e-14)
    assert float(v[2]) == pytest.approx(float(k.boundary(probe[2:3])), rel=1e-14)
    assert float(v[4]) == float(v[3]) == pytest.approx(float(k.boundary(probe[3:4])), rel=1e-14)


@pytest.mark.parametrize("p", [2, 4, 6])
@pytest.mark.parametrize("dim", [1, 2, 3])
@pytest.mark.parametrize("name", nr.NAMES)
def test_regularised_kernel_pieces(name, dim, p):
    import torch_nfft_amd as tn
    c = 0.25
    kern = tn.RegularizedKernel(name, c=c, dim=dim, bandwidth=N_PIECES, p=p, device="cpu")
    assert kern.eps_I == p / N_PIECES and kern.eps_B == max(1.0 / 16.0, p / N_PIECES)  # NFFT3's defaults
    assert kern.max_radius == 0.25 - kern.eps_B / 2
    ref = nr.Restatement(name, c, p, kern.eps_I, kern.eps_B)
    _check_pieces(ref, p, kern.eps_I, kern.eps_B)
    _check_pieces(kern, p, kern.eps_I, kern.eps_B)
    assert kern.near_poly.dtype == torch.float64 and kern.near_poly.shape == (p,)
    assert np.abs(kern.near_poly.numpy() - ref.near_poly).max() <= 1e-8 * np.abs(ref.near_poly).max()
    # the whole K_R, both versions
    r = torch.linspace(0.0, 0.9, 419, dtype=torch.float64)
    assert rel_l2(kern(r).numpy(), ref(r).numpy()) <= 1e-9
    assert kern.coeffs.shape == (N_PIECES,) * dim and kern.coeffs.dtype == torch.float32


@pytest.mark.parametrize("name,dim,N,p", [("one_over_modulus", 3, 32, 4), ("logarithm", 2, 64, 4), ("gaussian", 1, 128, 6),
                                          ("thinplate_spline", 2, 32, 2), ("one_over_square", 3, 16, 3)])
def test_coeffs_match_float64_restatement(name, dim, N, p):
    """kern.coeffs is float32: against the restatement's float64 coefficients it differs by its rounding, 2^-24 relative
    per element, i.e. at most 6e-8 in rel_l2 (the float64 evaluation errors of K_R are eight orders below)."""
    import torch_nfft_amd as tn
    kern = tn.RegularizedKernel(name, c=0.05, dim=dim, bandwidth=N, p=p, device="cpu")
    ref = nr.Restatement(name, 0.05, p, kern.eps_I, kern.eps_B)
    err = rel_l2(kern.coeffs.numpy().astype(np.float64), ref.coeffs(N, dim))
    print("coeffs", name, dim, N, p, "rel_l2 %.2e" % err)
    assert err <= 6e-8


def test_no_boundary_piece_samples_the_kernel_itself():
    import torch_nfft_amd as tn
    kern = tn.RegularizedKernel("multiquadric", c=0.1, dim=2, bandwidth=16, p=3, eps_B=0.0, device="cpu")
    assert kern.max_radius == 0.25
    r = torch.tensor([0.2, 0.45, 0.5, 0.65], dtype=torch.float64)
    assert torch.equal(kern(r), kern.kernel(r))
    ref = nr.Restatement("multiquadric", 0.1, 3, kern.eps_I, 0.0)
    assert rel_l2(kern.coeffs.numpy().astype(np.float64), ref.coeffs(16, 2)) <= 6e-8


@pytest.fixture(scope="module")
def algorithm_problem():
    rng = np.random.default_rng(11)
    N, p, n = 32, 4, 800
    eps_B = max(1.0 / 16.0, p / N)
    pts = nr.ball_points(rng, n, 3, 0.25 - eps_B / 2)
    x = rng.standard_normal(n)
    return N, p, eps_B, pts, x


@pytest.mark.parametrize("name", ["one_over_modulus", "logarithm"])
def test_float64_algorithm_against_dense_sum(name, algorithm_problem):
    """The algorithm's own error in exact arithmetic (3-D, N = 32, p = 4, 800 shared points in the ball): what is left is
    the trigonometric approximation of K_R.  Recorded in DESIGN.md section 7d: 1/r 1.90e-4, log r 1.22e-4 (relative l2).
    The far field alone, i.e. the sum without the near field, must be wrong by O(1): that is what the near field is for."""
    N, p, eps_B, pts, x = algorithm_problem
    ref = nr.Restatement(name, 1.0, p, p / N, eps_B)
    dense = nr.dense_sum(name, 1.0, x, pts)
    y = nr.exact_algorithm(ref, N, x, pts)
    err = rel_l2(y, dense)
    near = nr.near_sum(name, 1.0, ref.near_poly, ref.eps_I, x, pts)
    err_far_only = rel_l2(y - near, dense)
    print("float64 algorithm", name, "rel_l2 vs dense %.3e, without the near field %.3e" % (err, err_far_only))
    # p = 4 derivatives match at both joins, so the Fourier coefficients of K_R decay like |l|^-(p+1) beyond the band:
    # two digits or better at N = 32; without the near field the singularity is simply missing
    assert err < 1e-2
    assert err_far_only > 10 * err


def test_parameter_validation():
    import torch_nfft_amd as tn
    K = tn.RegularizedKernel
    with pytest.raises(ValueError, match="unknown kernel"):
        K("coulomb", device="cpu")
    for p in (0, 9):
        with pytest.raises(ValueError, match="p must be in 1..8"):
            K("one_over_modulus", p=p, device="cpu")
    for kw in ({"eps_I": 0.0}, {"eps_I": -0.1}, {"eps_I": 0.45}, {"eps_I": 0.3, "eps_B": 0.2}):
        with pytest.raises(ValueError, match="eps_I must lie in"):
            K("one_over_modulus", bandwidth=16, device="cpu", **kw)
    with pytest.raises(ValueError, match="eps_B must be >= 0"):
        K("one_over_modulus", eps_B=-0.01, device="cpu")
    with pytest.raises(ValueError, match="shape parameter"):
        K("gaussian", c=0.0, device="cpu")
    with pytest.raises(ValueError, match="dim must be"):
        K("gaussian", dim=4, device="cpu")
    for p in (1, 8):  # the ends of the accepted range
        kern = K("logarithm", dim=1, bandwidth=64, p=p, device="cpu")
        assert kern.near_poly.shape == (p,) and bool(torch.isfinite(kern.coeffs).all())


def test_cpu_tensors_are_refused():
    import torch_nfft
    import torch_nfft_amd as tn
    assert torch_nfft.nfft_fastsum_nearfield is tn.nfft_fastsum_nearfield
    assert torch_nfft.nearfield.RegularizedKernel is tn.RegularizedKernel
    kern = tn.RegularizedKernel("one_over_modulus", dim=2, bandwidth=32, device="cpu")
    pts = torch.zeros(5, 2)
    with pytest.raises(RuntimeError, match="torch_nfft._nfft_nearfield is currently only implemented for GPU tensors"):
        tn.nfft_nearfield(torch.zeros(5), kern, pts)
    with pytest.raises(RuntimeError, match="torch_nfft._nfft_nearfield is currently only implemented for GPU tensors"):
        tn.ops.nfft_nearfield(pts, pts, torch.zeros(5), None, None, 0, 1.0, 0.25, [1.0, 2.0])
    s = str(torch.ops.torch_nfft._nfft_nearfield.default._schema)
    assert s == ("torch_nfft::_nfft_nearfield(Tensor sources, Tensor targets, Tensor x, Tensor? source_batch, "
                 "Tensor? target_batch, int kernel, float c, float eps_I, float[] poly) -> Tensor")
    for arg in ("sources", "targets", "source_batch"):
        t = {"sources": pts, "targets": pts.clone(), "source_batch": None}
        if arg == "source_batch":
            t[arg] = torch.zeros(5, requires_grad=True)
        else:
            t[arg] = t[arg].clone().requires_grad_(True)
        with pytest.raises(AssertionError, match=arg):
            tn.nfft_fastsum_nearfield(torch.zeros(5), kern, t["sources"], t["targets"], t["source_batch"], None)


def test_c_abi_validation_without_gpu():
    from torch_nfft_amd import _lib
    lib = _lib.load()
    assert lib.nfft_hip_nearfield_cells(3, 1.0 / 16.0, 1) == 8
    assert lib.nfft_hip_nearfield_cells(2, 0.07, 3) == 7
    assert lib.nfft_hip_nearfield_cells(1, 0.3, 1) == 1
    G = lib.nfft_hip_nearfield_cells(3, 1e-5, 4)  # capped: at most 2^20 cells in all point sets
    assert G >= 1 and 4 * G ** 3 <= 1 << 20
    assert lib.nfft_hip_nearfield_cells(3, 0.5, 1) == -1 and _lib.last_error().startswith("Input mismatch")

    def problem(**kw):
        f = dict(dim=3, kernel=0, poly_terms=4, cells_per_axis=8, num_sources=1000, num_targets=900, num_columns=2,
                 batch_size=1, c=1.0, eps_I=1.0 / 16.0)
        f.update(kw)
        q = _lib.NearfieldProblem(**f)
        for e in range(8):
            q.poly[e] = 1.0
        return q

    ok = problem()
    assert lib.nfft_hip_nearfield_workspace_bytes(ctypes.byref(ok)) >= (900 // 128 + 512) * 8
    for bad in (problem(dim=0), problem(dim=4), problem(kernel=8), problem(kernel=-1), problem(poly_terms=0),
                problem(poly_terms=9), problem(cells_per_axis=9), problem(cells_per_axis=0), problem(eps_I=0.0),
                problem(num_targets=-1), problem(num_sources=1 << 31), problem(batch_size=0), problem(kernel=6, c=0.0),
                problem(cells_per_axis=200, eps_I=0.001)):
        assert lib.nfft_hip_nearfield_workspace_bytes(ctypes.byref(bad)) == -1
        assert _lib.last_error().startswith("Input mismatch")
    # the compute entry point refuses a null or short workspace before touching the device
    null = ctypes.c_void_p(0)
    one = ctypes.c_void_p(256)  # (never dereferenced: the workspace check comes first)
    assert lib.nfft_hip_nearfield(ctypes.byref(ok), one, one, one, one, one, one, one, null, 0, null) == _lib.EWORKSPACE
