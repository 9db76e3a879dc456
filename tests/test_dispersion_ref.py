"""CPU tests of the dispersion Ewald sum, the periodic 1/r^6 (nfft_ewald_dispersion): the float64
restatement tests/dispersion_ref.py against a brute-force lattice sum and against the mistakes a pair sweep can make, the
host-side pieces of torch_nfft_amd/dispersion.py against the restatement, the refusals, the C ABI and the registers of the
pair kernel."""
import ctypes
import math
import re

import numpy as np
import pytest
import torch

import dispersion_ref as dr
from conftest import rel_l2
from ewald_box_ref import O, T

BOXES = {"cube": None, "T": T, "O": O}


@pytest.mark.parametrize("box", ["cube", "T", "O"])
def test_split_against_lattice_sum(box):
    """near (every image within two cells, no cut) + far (|k| <= 14) - self against the brute-force sum over every image
    within 14 box lengths plus its continuum tail.  Agreement 2e-12 was seen when the formulas were derived; 1e-9 leaves
    room for other seeds and boxes."""
    A = BOXES[box]
    rng = np.random.default_rng(5)
    n = 12
    s = rng.random((n, 3)) - 0.5
    c = rng.random(n) + 0.5
    want, gwant = dr.lattice_sum(c, s, A, 14.0)
    got, ggot = dr.dispersion(c, s, A, None, 3.2, None, 30, nimg=2)
    e, ge = rel_l2(got, want), rel_l2(ggot, gwant)
    print("dispersion split in %s: potential rel_l2 %.3e, field rel_l2 %.3e" % (box, e, ge))
    assert e <= 1e-9 and ge <= 1e-9
    # the split does not depend on alpha
    other, gother = dr.dispersion(c, s, A, None, 4.0, None, 30, nimg=2)
    assert rel_l2(other, got) <= 1e-9 and rel_l2(gother, ggot) <= 1e-9


@pytest.mark.parametrize("box", ["cube", "T", "O"])
def test_splitting_coefficients(box):
    import torch_nfft
    import torch_nfft_amd as tn
    assert torch_nfft.DispersionSplitting is tn.DispersionSplitting
    assert torch_nfft.nfft_ewald_dispersion is tn.nfft_ewald_dispersion
    assert torch_nfft.nfft_ewald_dispersion_energy is tn.nfft_ewald_dispersion_energy
    A = BOXES[box]
    V = 1.0 if A is None else float(np.linalg.det(A))
    for alpha, N in ((11.5, 32), (6.0, 16)):
        sp = tn.DispersionSplitting(alpha, 0.25, N, box=None if A is None else torch.from_numpy(A), device="cpu")
        assert sp.coeffs.shape == (N, N, N) and sp.coeffs.dtype == torch.float32
        assert sp.volume == pytest.approx(V, rel=1e-14) and sp.bandwidth == N and sp.alpha == alpha and sp.r_cut == 0.25
        want = dr.coeffs(A, alpha, N)
        b = sp.coeffs.numpy()
        assert np.abs(b - want).max() <= 6e-8 * np.abs(want).max()  # (float32 rounding of float64 values)
        h = N // 2
        assert abs(b[h, h, h] - math.pi ** 1.5 * alpha ** 3 / (3 * V)) <= 6e-8 * b[h, h, h] and b[h, h, h] == b.max()
        assert not b[0].any() and not b[:, 0].any() and not b[:, :, 0].any()
        assert (b[1:, 1:, 1:] == b[1:, 1:, 1:][::-1, ::-1, ::-1]).all()  # b_k = b_-k: a real c gives a real psi
        assert (b >= 0).all()
        fc = sp.field_coeffs()
        assert fc.shape == (N, N, N, 4) and fc.dtype == torch.complex64
        _, kap = dr.kappa(A, N)
        assert rel_l2(fc[..., 0].numpy(), want.astype(np.complex128)) <= 1e-7
        for a in range(3):
            assert rel_l2(fc[..., 1 + a].numpy(), 2j * math.pi * kap[..., a] * want) <= 2e-7


@pytest.mark.parametrize("box", ["cube", "T"])
@pytest.mark.parametrize("tol", [1e-3, 1e-5])
def test_from_tolerance(box, tol):
    import torch_nfft_amd as tn
    A = BOXES[box]
    sp = tn.DispersionSplitting.from_tolerance(tol, 0.25, box=None if A is None else torch.from_numpy(A), device="cpu")
    assert sp.r_cut == 0.25
    # alpha: the pair factor at r_cut is tol (from below)
    pf = dr.pair_factor(sp.alpha * sp.r_cut)
    assert pf <= tol and pf >= tol * (1 - 1e-9)
    # N: the first even integer whose plane k_a = N/2 of the longest lattice vector has f(b) <= tol
    longest = 1.0 if A is None else max(np.linalg.norm(A, axis=1))
    N = sp.bandwidth
    assert N % 2 == 0 and N >= 2
    assert dr.far_factor(math.pi * (N / 2) / (sp.alpha * longest)) <= tol
    assert N == 2 or dr.far_factor(math.pi * (N / 2 - 1) / (sp.alpha * longest)) > tol
    with pytest.raises(ValueError):
        tn.DispersionSplitting.from_tolerance(1.5, 0.25, device="cpu")
    with pytest.raises(ValueError):
        tn.DispersionSplitting.from_tolerance(tol, 0.34, device="cpu")


def test_far_factor_limits():
    assert dr.far_factor(0.0) == 1.0
    b = np.array([3.0, 5.0, 8.0])
    assert np.abs(dr.far_factor(b) / (1.5 * np.exp(-b * b) / (b * b)) - 1).max() <= 2.5 / 9.0  # (next term: -5 / (2 b^2))
    assert (dr.far_factor(np.array([30.0, 1e3])) == 0).all()
    import torch_nfft_amd.dispersion as d
    assert np.abs(d._far_factor(torch.from_numpy(b)).numpy() - dr.far_factor(b)).max() <= 1e-16


def test_exports_symbols_and_schemas():
    import torch_nfft_amd as tn
    from torch_nfft_amd import _lib
    for name in ("DispersionSplitting", "nfft_ewald_dispersion", "nfft_ewald_dispersion_energy", "NfftEwaldDispersionFunction"):
        assert name in tn.__all__ and hasattr(tn, name)
    lib = _lib.load()
    assert _lib.ABI_VERSION == 7 and lib.nfft_hip_abi_version() == 7
    for name in ("nfft_hip_ewald_dispersion_near", "nfft_hip_ewald_dispersion_near_box"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    s = str(torch.ops.torch_nfft._nfft_ewald_dispersion_near.default._schema)
    assert s == ("torch_nfft::_nfft_ewald_dispersion_near(Tensor pos, Tensor x, Tensor? batch, float alpha, float r_cut, "
                 "bool with_field) -> (Tensor, Tensor)")
    s = str(torch.ops.torch_nfft._nfft_ewald_dispersion_near_box.default._schema)
    assert s == ("torch_nfft::_nfft_ewald_dispersion_near_box(Tensor pos, Tensor x, Tensor? batch, float[] box, float alpha, "
                 "float r_cut, bool with_field) -> (Tensor, Tensor)")
    c, pos = torch.zeros(5), torch.zeros(5, 3)
    with pytest.raises(RuntimeError, match="torch_nfft._nfft_ewald_dispersion_near is currently only implemented for GPU tensors"):
        tn.ops.nfft_ewald_dispersion_near(pos, c, None, 5.0, 0.3, True)
    with pytest.raises(RuntimeError, match="torch_nfft._nfft_ewald_dispersion_near_box is currently only implemented for GPU tensors"):
        tn.ops.nfft_ewald_dispersion_near_box(pos, c, None, (1.0, 0.0, 1.3, 0.0, 0.0, 0.8), 5.0, 0.25, False)


def test_refusals():
    import torch_nfft_amd as tn
    for bad in (dict(r_cut=0.34), dict(r_cut=0.0), dict(bandwidth=31), dict(bandwidth=0), dict(alpha=0.0), dict(alpha=-1.0),
                dict(box=[1.0, 1.0]), dict(box=[[1.0, 0.1, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]), dict(box=[1.0, -1.0, 1.0]),
                dict(box=[1.0, 1.0, 0.8])):  # (r_cut = 0.3 > 0.8 / 3)
        kw = dict(alpha=6.0, r_cut=0.3, bandwidth=16, device="cpu")
        kw.update(bad)
        with pytest.raises(ValueError, match="DispersionSplitting"):
            tn.DispersionSplitting(**kw)
    with pytest.raises(AssertionError, match="box requires grad"):
        tn.DispersionSplitting(6.0, 0.3, 16, box=torch.ones(3, requires_grad=True), device="cpu")
    assert tn.DispersionSplitting(6.0, 1.0 / 3.0, 16, device="cpu").cells == (3, 3, 3)
    spb = tn.DispersionSplitting(6.0, 0.25, 16, box=[1.0, 1.3, 0.8], device="cpu")
    assert spb.cells == (4, 5, 3) and spb.box6 == (1.0, 0.0, 1.3, 0.0, 0.0, 0.8)
    sp = tn.DispersionSplitting(6.0, 0.3, 16, device="cpu")
    c, pos = torch.zeros(5), torch.zeros(5, 3)
    for fn in (tn.nfft_ewald_dispersion, tn.nfft_ewald_dispersion_energy):
        with pytest.raises(ValueError, match="three-dimensional"):
            fn(c, torch.zeros(5, 2), splitting=sp)
        with pytest.raises(AssertionError, match="batch"):
            fn(c, pos, torch.zeros(5, requires_grad=True), splitting=sp)
        with pytest.raises(RuntimeError, match="is currently only implemented for GPU tensors"):
            fn(c, pos, splitting=sp)
        with pytest.raises(RuntimeError, match="is currently only implemented for GPU tensors"):
            fn(c, pos, splitting=spb)
        with pytest.raises(TypeError, match="DispersionSplitting"):
            fn(c, pos)
        with pytest.raises(TypeError, match="DispersionSplitting"):  # the Coulomb splitting is the wrong class
            fn(c, pos, splitting=tn.EwaldSplitting(6.0, 0.3, 16, device="cpu"))
        with pytest.raises(ValueError, match="fractional"):
            fn(c, pos, splitting=sp, fractional=True)
    with pytest.raises(TypeError):  # ... and the other way round
        tn.nfft_ewald(c, pos, splitting=sp)
    with pytest.raises(RuntimeError, match="is currently only implemented for GPU tensors"):
        tn.nfft_ewald_dispersion(c, pos, splitting=sp, field=True)


def test_c_abi_validation_without_gpu():
    """the two entry points validate as their Coulomb twins do and take the workspace that the shared functions report"""
    from torch_nfft_amd import _lib
    lib = _lib.load()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(256)  # (never dereferenced: the checks come first)

    def problem(**kw):
        f = dict(cells_per_axis=4, with_field=1, num_points=1000, num_columns=2, batch_size=1, alpha=6.0, r_cut=0.25)
        f.update(kw)
        return _lib.EwaldProblem(**f)

    def call(q, ws=null, nbytes=0, z=one, field=one, points=one):
        return lib.nfft_hip_ewald_dispersion_near(ctypes.byref(q), points, one, one, one, z, field, ws, nbytes, null)

    ok = problem()
    need = lib.nfft_hip_ewald_near_workspace_bytes(ctypes.byref(ok))
    assert need > 0
    assert call(ok) == _lib.EWORKSPACE and _lib.last_error() == "workspace too small"
    assert call(ok, one, need - 1) == _lib.EWORKSPACE
    assert call(problem(with_field=0), field=null) == _lib.EWORKSPACE
    assert call(ok, field=null) == _lib.EINVAL and _lib.last_error().startswith("Input mismatch")
    assert call(ok, z=null) == _lib.EINVAL and call(ok, points=null) == _lib.EINVAL
    for bad in (problem(cells_per_axis=2), problem(cells_per_axis=5), problem(with_field=2), problem(num_points=-1),
                problem(alpha=0.0), problem(r_cut=0.34, cells_per_axis=3), problem(batch_size=0)):
        assert call(bad) == _lib.EINVAL and _lib.last_error().startswith("Input mismatch")
    assert call(problem(num_points=0)) == _lib.OK and call(problem(num_columns=0)) == _lib.OK

    def box_problem(**kw):
        f = dict(cells=(ctypes.c_int32 * 3)(4, 5, 3), with_field=1, num_points=1000, num_columns=2, batch_size=1, alpha=6.0,
                 r_cut=0.25, box=(ctypes.c_double * 6)(1.0, 0.0, 1.3, 0.0, 0.0, 0.8))
        f.update(kw)
        return _lib.EwaldBoxProblem(**f)

    def box_call(q, ws=null, nbytes=0, z=one, field=one):
        return lib.nfft_hip_ewald_dispersion_near_box(ctypes.byref(q), one, one, one, one, z, field, ws, nbytes, null)

    okb = box_problem()
    needb = lib.nfft_hip_ewald_near_box_workspace_bytes(ctypes.byref(okb))
    assert needb > 0
    assert box_call(okb) == _lib.EWORKSPACE and box_call(okb, one, needb - 1) == _lib.EWORKSPACE
    assert box_call(okb, field=null) == _lib.EINVAL and box_call(okb, z=null) == _lib.EINVAL
    for bad in (box_problem(cells=(ctypes.c_int32 * 3)(4, 6, 3)), box_problem(r_cut=0.3), box_problem(alpha=float("nan")),
                box_problem(box=(ctypes.c_double * 6)(1.0, 0.0, -1.3, 0.0, 0.0, 0.8))):
        assert box_call(bad) == _lib.EINVAL and _lib.last_error().startswith("Input mismatch")
    assert box_call(box_problem(num_points=0)) == _lib.OK


def test_pair_kernel_resource_usage():
    """exactly the twelve instantiations <CC, FIELD, BOX> of the dispersion pair kernel, each without scratch and without
    spills (the library's own flags; VGPRs and occupancy are recorded in DESIGN.md section 7j, not gated)"""
    from resource_usage import resource_usage
    usage = resource_usage("ewald_disp.hip")
    by = {}
    for name, u in usage.items():
        m = re.search(r"ewald_disp_near_kernelILi(\d)ELb(\d)ELb(\d)EE", name)
        assert m, name  # (nothing else in that file)
        by[(int(m.group(1)), int(m.group(2)), int(m.group(3)))] = u
    assert set(by) == {(cc, f, box) for cc in (1, 2, 4) for f in (0, 1) for box in (0, 1)} and len(usage) == 12
    for key, u in sorted(by.items()):
        print(key, "VGPRs %d occupancy %d LDS %d" % (u["VGPRs"], u["Occupancy"], u["LDS Size"]))
        assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (key, u)


# (alpha, r_c) of the GPU near-sweep tests: alpha r_c ~ 1.5, G = 3, 4, 8 cells per axis
NEAR_CASES = [(5.0, 0.3), (6.0, 0.25), (12.0, 0.12)]
CEILING = 1e-4  # what a first device run may show at most (tests/test_gpu_dispersion.py)


@pytest.mark.parametrize("alpha,r_c", NEAR_CASES)
def test_near_sum_is_sensitive_to_mistakes(alpha, r_c):
    """On the points of the GPU near-sweep test (the 8^3 jittered lattice) three mistakes of a pair sweep each move the value
    and the field sums by at least three times the ceiling of a device run's error: no wrap, a cut at 0.95 r_c, the top
    term of the polynomial dropped.  The smallest move seen is 5.3e-4 (the field under the cut at (5, 0.3)); the missing wrap moves them
    by 0.3 .. 0.5.  At alpha r_c ~ 3.5 the cut would hide at 4e-6: that is why these tests use a loose alpha."""
    x = dr.jittered_lattice(np.random.default_rng(0), 8, 1.0 / 8, 0.03).reshape(-1, 3)
    c = (np.random.default_rng(1).random(512) + 0.5).astype(np.float32)
    z, f = dr.near_sum(c, x, None, None, alpha, r_c), dr.near_field(c, x, None, None, alpha, r_c)
    assert np.linalg.norm(z) > 0 and np.linalg.norm(f) > 0
    for what, kw, rc in (("no wrap", dict(wrap=False), r_c), ("0.95 r_c", {}, 0.95 * r_c), ("top term", dict(top_term=False), r_c)):
        ez = rel_l2(dr.near_sum(c, x, None, None, alpha, rc, **kw), z)
        ef = rel_l2(dr.near_field(c, x, None, None, alpha, rc, **kw), f)
        print("(%g, %g) %s: value moves by %.3e, field by %.3e" % (alpha, r_c, what, ez, ef))
        assert ez >= 3 * CEILING and ef >= 3 * CEILING


def test_field_is_the_gradient():
    """G = -grad psi of the split sum by central differences (h = 1e-5, error O(h^2) ~ 1e-8 relative to the field's scale)"""
    rng = np.random.default_rng(3)
    s = dr.jittered_lattice(rng, 3, 1.0 / 3, 0.05).reshape(-1, 3).astype(np.float64)
    c = rng.random(27) + 0.5
    _, G = dr.dispersion(c, s, T, None, 6.0, None, 16, nimg=1)
    h = 1e-5
    inv = np.linalg.inv(T)
    for i, a in ((0, 0), (13, 1), (26, 2)):
        e = np.zeros(3)
        e[a] = h
        sp, sm = s.copy(), s.copy()
        sp[i] += e @ inv
        sm[i] -= e @ inv
        up = 0.5 * (c * dr.dispersion(c, sp, T, None, 6.0, None, 16, nimg=1)[0]).sum()
        um = 0.5 * (c * dr.dispersion(c, sm, T, None, 6.0, None, 16, nimg=1)[0]).sum()
        assert abs(-(up - um) / (2 * h) - c[i] * G[i, a]) <= 1e-6 * np.abs(c[:, None] * G).max()
