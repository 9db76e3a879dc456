"""CPU tests of the point gradients of the fast summation with a regularised kernel (point_gradients=True, DESIGN.md
section 7f): the float64 restatement tests/nearfield_point_grad_ref.py against float64 autograd and against the dense
gradient, the guard of the GPU tests' tolerances, the host side of torch_nfft_amd/nearfield.py, the C ABI's validation and
the pair kernel's resources."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import nearfield_point_grad_ref as npg
import nearfield_ref as nr
from conftest import rel_l2
from resource_usage import resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _autograd_near_gradients(ref, x, dy, s, t, sb, tb):
    """(ds, dt) of <dy, sum_j (K - T_I)(r_ij) [0 < r_ij < eps_I] x_j> by float64 torch.autograd; shared points (t None):
    the total of the one point set, returned twice"""
    ss = torch.tensor(np.asarray(s, dtype=np.float64), requires_grad=True)
    ts = ss if t is None else torch.tensor(np.asarray(t, dtype=np.float64), requires_grad=True)
    d = ts[:, None, :] - ss[None, :, :]
    r2 = (d * d).sum(-1)
    pair = (r2 > 0) & (r2 < ref.eps_I ** 2)  # (r = 0: K - T_I does not depend on the points there, or is left out)
    if sb is not None:
        pair = pair & torch.tensor((tb if t is not None else sb)[:, None] == sb[None, :])
    r = torch.sqrt(torch.where(pair, r2, torch.full_like(r2, (0.5 * ref.eps_I) ** 2)))
    W = torch.where(pair, ref.kernel(r) - ref.inner(r), torch.zeros_like(r))
    xr, dyr = torch.tensor(npg._real_columns(x)), torch.tensor(npg._real_columns(dy))
    ((W @ xr) * dyr).sum().backward()
    return ss.grad.numpy(), ts.grad.numpy()


@pytest.mark.parametrize("shared", [True, False], ids=["shared", "separate"])
@pytest.mark.parametrize("complex_x", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("dim", [1, 2, 3])
@pytest.mark.parametrize("name", nr.NAMES)
def test_restatement_against_float64_autograd(name, dim, complex_x, shared):
    rng = np.random.default_rng(61 + dim)
    ref = nr.Restatement(name, 0.05, 4, 0.07, 0.0625)
    ns, nt = 90, 70
    s = nr.ball_points(rng, ns, dim, 0.2)
    s[10:15] = s[0:5]
    t = None if shared else nr.ball_points(rng, nt, dim, 0.2)
    if t is not None:
        t[:8] = s[:8]
    sb = np.sort(rng.integers(0, 2, ns))
    tb = None if shared else np.sort(rng.integers(0, 2, nt))
    x, dy = rng.standard_normal((ns, 2)), rng.standard_normal((ns if shared else nt, 2))
    if complex_x:
        x, dy = x + 1j * rng.standard_normal(x.shape), dy + 1j * rng.standard_normal(dy.shape)
    ds, dt = npg.near_point_gradients(name, 0.05, ref.near_poly, 0.07, x, dy, s, t, sb, tb)
    want_s, want_t = _autograd_near_gradients(ref, x, dy, s, t, sb, tb)
    assert ds.shape == (ns, dim) and dt.shape == ((ns if shared else nt), dim)
    if shared:
        assert np.linalg.norm(want_s) > 0 and rel_l2(ds + dt, want_s) <= 1e-10
    else:
        assert np.linalg.norm(want_s) > 0 and np.linalg.norm(want_t) > 0
        assert rel_l2(ds, want_s) <= 1e-10 and rel_l2(dt, want_t) <= 1e-10


@pytest.mark.parametrize("name,dim,n", [("one_over_modulus", 3, 120), ("logarithm", 2, 300)])
def test_float64_algorithm_against_dense_point_gradient(name, dim, n):
    """The algorithm's own error for the point gradients in exact arithmetic (N = 32, p = 4, shared points in the ball, the
    far part with the unpaired planes l_a = -N/2 kept, as nfft_fastsum differentiates it).  Relative l2 of the total
    ds + dt against the dense gradient of sum_i dy_i sum_j K(r_ij) x_j, recorded in DESIGN.md section 7f:
    3-D 1/r, 120 points 2.26e-4 (0.976 without the near part);  2-D log r, 300 points 3.56e-4 (0.906).  With 100 and 280
    separate targets, sources / targets: 6.60e-4 / 7.86e-4 and 4.28e-4 / 4.05e-4."""
    rng = np.random.default_rng(41 + dim)
    N, p = 32, 4
    eps_B = max(1.0 / 16.0, p / N)
    pts = nr.ball_points(rng, n, dim, 0.25 - eps_B / 2)
    x, dy = rng.standard_normal(n), rng.standard_normal(n)
    ref = nr.Restatement(name, 1.0, p, p / N, eps_B)
    dense = sum(npg.dense_point_gradients(name, 1.0, x, dy, pts))
    alg = sum(npg.exact_algorithm_point_gradients(ref, N, x, dy, pts))
    near = sum(npg.near_point_gradients(name, 1.0, ref.near_poly, ref.eps_I, x, dy, pts))
    assert alg.shape == dense.shape == (n, dim)
    err, err_far_only = rel_l2(alg, dense), rel_l2(alg - near, dense)
    print("float64 point gradient", name, "rel_l2 vs dense %.3e, without the near part %.3e" % (err, err_far_only))
    assert err < 1e-2
    assert err_far_only > 10 * err
    # each side on its own against the dense one, separate targets
    t = nr.ball_points(rng, n - 20, dim, 0.25 - eps_B / 2)
    dyt = rng.standard_normal(n - 20)
    a, d = npg.exact_algorithm_point_gradients(ref, N, x, dyt, pts, t), npg.dense_point_gradients(name, 1.0, x, dyt, pts, t)
    print("   separate targets: ds %.3e, dt %.3e" % (rel_l2(a[0], d[0]), rel_l2(a[1], d[1])))
    assert rel_l2(a[0], d[0]) < 1e-2 and rel_l2(a[1], d[1]) < 1e-2


def test_no_tolerance_hides_a_missed_cell():
    """On the inputs of the GPU tests' CASES, leaving the pairs of ONE neighbour cell (the next one along the first axis)
    out of the restatement changes every result by more than 10x the loosest tolerance of the GPU tests."""
    import test_gpu_nearfield_point_grad as g
    loosest = max(max(g.PGRAD_TOL.values()), g.WHOLE_PGRAD_TOL)
    assert set(g.PGRAD_TOL) == set(nr.NAMES) and loosest < 1e-3
    smallest = np.inf
    for case in g.CASES:
        kern, x, dy, s, t, sb, tb = g.case_inputs(case)
        assert kern.eps_I == g.EPS_I and int(0.5 / kern.eps_I) == g.CELLS
        args = (kern.name, kern.c, kern.near_poly.numpy(), kern.eps_I, x, dy, s, t, sb, tb)
        skip = npg.cell_offset_pairs(s, t, g.CELLS, (1,) + (0,) * (s.shape[1] - 1))
        full, cut = npg.near_point_gradients(*args), npg.near_point_gradients(*args, skip=skip)
        for a, b in ((full[0], cut[0]), (full[1], cut[1]), (full[0] + full[1], cut[0] + cut[1])) if t is None else \
                ((full[0], cut[0]), (full[1], cut[1])):
            smallest = min(smallest, rel_l2(b, a))
    print("a missed neighbour cell moves the restatement by at least %.3e; the loosest tolerance is %.3e" % (smallest, loosest))
    assert smallest > 10 * loosest


def test_host_side():
    import torch_nfft
    import torch_nfft_amd as tn
    assert torch_nfft.NfftNearfieldPointsFunction is tn.NfftNearfieldPointsFunction
    assert "NfftNearfieldPointsFunction" in tn.__all__
    s = str(torch.ops.torch_nfft._nfft_nearfield_point_gradient.default._schema)
    assert s == ("torch_nfft::_nfft_nearfield_point_gradient(Tensor sources, Tensor targets, Tensor x, Tensor dy, "
                 "Tensor? source_batch, Tensor? target_batch, int kernel, float c, float eps_I, float[] poly, "
                 "bool need_sources, bool need_targets) -> (Tensor, Tensor)")
    kern = tn.RegularizedKernel("one_over_modulus", dim=2, bandwidth=32, device="cpu")
    pts = torch.zeros(5, 2)
    msg = "torch_nfft._nfft_nearfield_point_gradient is currently only implemented for GPU tensors"
    with pytest.raises(RuntimeError, match=msg):
        tn.ops.nfft_nearfield_point_gradient(pts, pts, torch.zeros(5), torch.zeros(5), None, None, 0, 1.0, 0.125,
                                             [1.0, 2.0, 3.0], True, True)
    for fn in (tn.nfft_fastsum_nearfield, tn.nfft_nearfield):
        for arg in ("sources", "targets", "source_batch", "target_batch"):
            for point_gradients in (False, True):
                t = {"sources": pts, "targets": pts.clone(), "source_batch": None, "target_batch": None}
                if arg.endswith("_batch"):
                    t[arg] = torch.zeros(5, requires_grad=True)
                elif point_gradients:
                    continue
                else:
                    t[arg] = t[arg].clone().requires_grad_(True)
                with pytest.raises(AssertionError, match=arg):  # point_gradients=False still refuses; batch vectors always
                    fn(torch.zeros(5), kern, t["sources"], t["targets"], t["source_batch"], t["target_batch"],
                       point_gradients=point_gradients)
    with pytest.raises(AssertionError, match=r"pass point_gradients=True"):
        tn.nfft_nearfield(torch.zeros(5), kern, pts.clone().requires_grad_(True))
    with pytest.raises(TypeError):  # keyword only
        tn.nfft_nearfield(torch.zeros(5), kern, pts, None, None, None, None, True)
    one = tn.RegularizedKernel("logarithm", dim=2, bandwidth=32, p=1, device="cpu")
    for fn in (tn.nfft_fastsum_nearfield, tn.nfft_nearfield):
        with pytest.raises(ValueError, match="p >= 2"):
            fn(torch.zeros(5), one, pts.clone().requires_grad_(True), point_gradients=True)
        with pytest.raises(ValueError, match="p >= 2"):
            fn(torch.zeros(5), one, pts, pts.clone().requires_grad_(True), point_gradients=True)
    # the two functions of the field itself keep refusing, and have no such keyword
    for fn in (tn.nfft_fastsum_nearfield_gradient, tn.nfft_nearfield_gradient):
        with pytest.raises(AssertionError, match="sources"):
            fn(torch.zeros(5), kern, pts.clone().requires_grad_(True))
        with pytest.raises(TypeError):
            fn(torch.zeros(5), kern, pts, point_gradients=True)


def test_c_abi_validation_without_gpu():
    from torch_nfft_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 7 and lib.nfft_hip_abi_version() == 7
    assert "nfft_hip_nearfield_point_gradient" in _lib.SYMBOLS
    assert "nfft_hip_nearfield_point_gradient_workspace_bytes" in _lib.SYMBOLS

    def problem(**kw):
        f = dict(dim=3, kernel=0, poly_terms=4, cells_per_axis=8, num_sources=900, num_targets=900, num_columns=2,
                 batch_size=1, c=1.0, eps_I=1.0 / 16.0)
        f.update(kw)
        return _lib.NearfieldProblem(**f)

    ok = problem()
    assert lib.nfft_hip_nearfield_point_gradient_workspace_bytes(ctypes.byref(ok)) == lib.nfft_hip_nearfield_gradient_workspace_bytes(ctypes.byref(ok))
    assert lib.nfft_hip_nearfield_point_gradient_workspace_bytes(ctypes.byref(problem(poly_terms=2))) > 0
    for bad in (problem(dim=0), problem(dim=4), problem(kernel=8), problem(kernel=-1), problem(poly_terms=0),
                problem(poly_terms=1), problem(poly_terms=9), problem(cells_per_axis=9), problem(eps_I=0.0),
                problem(num_targets=-1), problem(batch_size=0), problem(kernel=7, c=0.0)):
        assert lib.nfft_hip_nearfield_point_gradient_workspace_bytes(ctypes.byref(bad)) == -1
        assert _lib.last_error().startswith("Input mismatch")
    null = ctypes.c_void_p(0)
    one = ctypes.c_void_p(256)  # (never dereferenced: the checks come first)
    gpoly = (ctypes.c_double * 8)(1.0, 2.0, 3.0)
    gp = ctypes.cast(gpoly, ctypes.c_void_p)

    def call(q, symmetric, poly, ws=null, nbytes=0):
        return lib.nfft_hip_nearfield_point_gradient(ctypes.byref(q), symmetric, poly, one, one, one, one, one, one, one, one,
                                                     ws, nbytes, null)

    for symmetric in (0, 1):
        assert call(ok, symmetric, gp) == _lib.EWORKSPACE
        assert call(ok, symmetric, gp, one, 8) == _lib.EWORKSPACE
        assert call(problem(poly_terms=1), symmetric, gp) == _lib.EINVAL
        assert call(problem(dim=4), symmetric, gp) == _lib.EINVAL
        assert call(problem(kernel=9), symmetric, gp) == _lib.EINVAL
        assert call(ok, symmetric, null) == _lib.EINVAL
        # nothing to do: no launch, no workspace needed
        assert call(problem(num_targets=0, num_sources=0), symmetric, gp) == _lib.OK
        assert call(problem(num_columns=0), symmetric, gp) == _lib.OK
    assert call(problem(num_targets=0), 0, gp) == _lib.OK
    assert call(ok, 2, gp) == _lib.EINVAL and call(ok, -1, gp) == _lib.EINVAL
    assert call(problem(num_sources=800), 1, gp) == _lib.EINVAL  # one point set on both sides
    assert call(problem(num_sources=800), 0, gp) == _lib.EWORKSPACE
    gpoly[1] = float("nan")
    assert call(ok, 0, gp) == _lib.EINVAL and _lib.last_error().startswith("Input mismatch")


def test_pair_kernel_resource_usage():
    """Every instantiation <KERNEL, CC, PT, SYM> of the contracting pair kernel: no scratch and no spills of either kind.
    (VGPRs and occupancies are recorded in DESIGN.md section 7f, not gated.)"""
    usage = resource_usage("nearfield_pgrad.hip")
    pat = re.compile(r"nearfield_pgrad_kernelILi(\d)ELi(\d)ELi(\d)ELi(\d)EE")
    by = {}
    for name, u in usage.items():
        m = pat.search(name)
        if m:
            by[tuple(int(g) for g in m.groups())] = u
    assert set(by) == {(k, cc, pt, sym) for k in range(8) for cc in (1, 2, 4) for pt in (4, 8) for sym in (0, 1)}
    assert len(by) == 96
    for key, u in sorted(by.items()):
        print(key, "VGPRs %d occupancy %d LDS %d" % (u["VGPRs"], u["Occupancy"], u["LDS Size"]))
        assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (key, u)
