"""CPU tests of the Ewald virial tensor: the float64 restatement tests/ewald_virial_ref.py against
the strain derivative of the converged energy, its trace, its symmetry, its independence of alpha and the fixed points of
the lattice sums; the truncation of the algorithm; virial_to_box_gradient against difference quotients of the energy in
the box entries; how far off five wrong formulas are; the host-side refusals and the C ABI's validation."""
import ctypes
import math

import numpy as np
import pytest
import torch

import ewald_box_ref as eb
import ewald_ref as er
import ewald_virial_ref as ev

BOXES = {"T": eb.T, "O": eb.O, "S": eb.S}
H = 1e-5  # step of the central differences


@pytest.fixture(scope="module")
def few():
    """24 fractional positions with a neutral and a charged column of charges"""
    rng = np.random.default_rng(11)
    s = rng.random((24, 3)) - 0.5
    q = rng.standard_normal(24)
    return s, np.stack([q - q.mean(), q], 1)


def _energy(q, s, A, **kw):
    """U [cols] of the converged sum, from the potential of tests/ewald_box_ref.py (not from this restatement)"""
    return 0.5 * (q * eb.converged(q, s, A, **kw)).sum(0)


@pytest.mark.parametrize("name", ["T", "O"])
def test_virial_is_the_strain_derivative_of_the_energy(few, name):
    """W_ab = -dU / d eps_ab for A -> A (1 + eps) at fixed s, all nine entries, central differences with h = 1e-5 at
    kmax = 10.  Measured when this was written: 3.1e-9 (neutral) and 3.3e-9 (charged) of |W|_max = 36.2 in T, 3.8e-9 and
    3.7e-9 of 34.4 in O (on another set of 24 charges in T: 2.0e-9 and 2.6e-9 of 23.5).  The error is that of the
    difference quotient: its h^2 term plus the rounding of U over 2 h.  The bound is 4 x 3e-9, absolute."""
    s, q = few
    A = BOXES[name]
    U, W = ev.converged_virial(q, s, A, kmax=10)
    fd = np.zeros((3, 3, 2))
    for a in range(3):
        for b in range(3):
            eps = np.zeros((3, 3))
            eps[a, b] = H
            fd[a, b] = -(_energy(q, s, A @ (np.eye(3) + eps), kmax=10) - _energy(q, s, A @ (np.eye(3) - eps), kmax=10)) / (2 * H)
    err = np.abs(W[0] - fd).max((0, 1))
    print("box %s: |W + dU/d eps|_max neutral %.2e charged %.2e, |W|_max %.3g" % (name, err[0], err[1], np.abs(W).max()))
    assert np.abs(W).max() > 1.0
    assert err.max() <= 4 * 3e-9
    assert np.abs(U[0] - _energy(q, s, A, kmax=10)).max() <= 1e-11  # U is the energy of the potential
    assert np.abs(W - W.transpose(0, 2, 1, 3)).max() <= 1e-12


@pytest.mark.parametrize("name", ["T", "O"])
def test_trace_of_the_virial_is_the_energy(few, name):
    """tr W = U: 1/r is homogeneous of degree -1, with the neutralising background too.  It holds for the CONVERGED sum
    (|k|_inf <= 14: at 10 the far sum of the box O, whose longest edge is 1.3, is cut at |kappa| = 7.7 and the two differ
    by 1.5e-7).  The two agreed to 1e-12 when this was written; the bound is 4 x 1e-9, the accuracy to which the converged
    sums are pinned elsewhere"""
    s, q = few
    U, W = ev.converged_virial(q, s, BOXES[name])
    tr = np.trace(W[0])
    print("box %s: tr W = %s, U = %s, difference %s" % (name, tr, U[0], tr - U[0]))
    assert np.abs(tr - U[0]).max() <= 4 * 1e-9
    assert np.abs(W - W.transpose(0, 2, 1, 3)).max() <= 1e-12


def test_virial_does_not_depend_on_alpha(few):
    s, q = few
    for A in (eb.T, eb.O):
        U5, W5 = ev.converged_virial(q, s, A, alpha=5.0)
        U6, W6 = ev.converged_virial(q, s, A)
        print("alpha 5 vs 6: W %.1e U %.1e" % (np.abs(W5 - W6).max(), np.abs(U5 - U6).max()))
        assert np.abs(W5 - W6).max() <= 4 * 7e-10 and np.abs(U5 - U6).max() <= 4 * 7e-10


def test_point_sets_and_columns(few):
    """two sets with an empty one between them: each row is the sum of its own set, the empty one zero"""
    s, q = few
    batch = np.array([0] * 10 + [2] * 14)
    U, W = ev.converged_virial(q, s, eb.T, batch, kmax=8)
    assert U.shape == (3, 2) and W.shape == (3, 3, 3, 2)
    assert not U[1].any() and not W[1].any()
    for b, sel in ((0, slice(0, 10)), (2, slice(10, 24))):
        U1, W1 = ev.converged_virial(q[sel, 1], s[sel], eb.T, kmax=8)
        assert U1.shape == (1,) and W1.shape == (1, 3, 3)
        assert np.abs(U1[0] - U[b, 1]) <= 1e-12 and np.abs(W1[0] - W[b, :, :, 1]).max() <= 1e-12


def test_fixed_points():
    """cubic symmetry: W = (U / 3) I with U / q^2 at the lattice constants that tests/ewald_ref.py pins"""
    A_rs, _ = eb.lower_triangular(eb.ROCK_SALT_PRIMITIVE)
    cases = [("one charge in the unit cube", np.array([1.5]), np.array([[0.2, -0.4, 0.1]]), np.eye(3), 0.5 * er.CUBIC_LATTICE * 2.25),
             ("one charge in S", np.array([1.5]), np.array([[0.31, -0.47, 0.123]]), eb.S, 0.5 * er.CUBIC_LATTICE * 2.25),
             ("primitive rock salt", np.array([1.0, -1.0]), np.array([[0.0, 0.0, 0.0], [-0.5, -0.5, -0.5]]), A_rs,
              -2.0 * er.MADELUNG_NACL)]
    for what, q, s, A, want in cases:
        U, W = ev.converged_virial(q, s, A)
        print("%s: U = %.10f (%.10f), W = diag %s" % (what, U[0], want, np.diag(W[0])))
        assert abs(U[0] - want) <= 1e-9 * abs(want) + 1e-9
        assert np.abs(W[0] - want / 3.0 * np.eye(3)).max() <= 4e-9


@pytest.fixture(scope="module")
def charges():
    """300 float32 fractional positions with neutral float64 charges (those of tests/test_ewald_box_ref.py)"""
    rng = np.random.default_rng(0)
    s = (rng.random((300, 3)) - 0.5).astype(np.float32)
    q = rng.standard_normal(300)
    q -= q.mean()
    return s, q


# box, (alpha, r_c, N) -- the rows of section 7h's table -- and the truncation error of W (relative Frobenius norm on the
# 300 neutral charges), measured when this was written.  They are 10 to 50 times those of the potential in 7h's table: at
# r_c the pair weight of the virial, -g r^2 = erfc(alpha r) / r + (2 alpha / sqrt(pi)) e^(-alpha^2 r^2), is about
# 1 + 2 alpha^2 r_c^2 = 24 .. 27 times that of the potential.
TRUNCATION = [("T", (12.0, 0.3, 32), 3.34e-6),
              ("T", (14.0, 0.25, 48), 2.27e-6),
              ("O", (14.0, 0.25, 48), 1.36e-6),
              ("S", (16.0, 0.22, 48), 2.42e-5)]


@pytest.fixture(scope="module")
def converged_300(charges):
    s, q = charges
    done = {}

    def get(name):
        if name not in done:
            done[name] = ev.converged_virial(q, s, BOXES[name])
        return done[name]

    return get


@pytest.mark.parametrize("name,split,recorded", TRUNCATION)
def test_exact_algorithm_against_converged(charges, converged_300, name, split, recorded):
    s, q = charges
    alpha, r_c, N = split
    U, W = converged_300(name)
    Ua, Wa = ev.exact_algorithm_virial(q, s, BOXES[name], None, alpha, r_c, N)
    e_W, e_U = ev.rel_fro(Wa, W), ev.rel_fro(Ua, U)
    print("box %s (%g, %g, %d): W %.3e (recorded %.2e), U %.3e" % (name, alpha, r_c, N, e_W, recorded, e_U))
    assert e_W <= 1.5 * recorded
    # U of the algorithm is the energy of its potential
    want = 0.5 * (q * eb.exact_algorithm(q, s, BOXES[name], None, alpha, r_c, N)).sum()
    assert abs(Ua[0] - want) <= 1e-10 * abs(want)


# the relative error of W (Frobenius) that each wrong formula makes on the 300 charges + 0.1 in T at (12, 0.3, 32), measured
# when this was written; the largest tolerance of tests/test_gpu_ewald_virial.py is far below the smallest of them
MUTANTS = {"ds": 1.47e-1, "AT": 1.65e-1, "k": 2.71, "no_pi2": 2.54, "no_background": 3.64e-2}
LARGEST_GPU_TOLERANCE = 1e-4  # (a first-run figure above this is a defect, whatever the tolerance derived from it)


def test_mutants_are_far_off(charges):
    s, q = charges
    qn = q + 0.1  # (the background needs a net charge: Q = 30)
    alpha, r_c, N = 12.0, 0.3, 32
    _, W = ev.exact_algorithm_virial(qn, s, eb.T, None, alpha, r_c, N)
    for mutant, recorded in MUTANTS.items():
        _, Wm = ev.exact_algorithm_virial(qn, s, eb.T, None, alpha, r_c, N, mutant=mutant)
        err = ev.rel_fro(Wm, W)
        print("mutant %-14s relative error of W %.3e" % (mutant, err))
        assert err >= 100 * LARGEST_GPU_TOLERANCE
        assert 0.5 * recorded <= err <= 2.0 * recorded
    # the part-wise operators see the first four on their own
    for mutant in ("ds", "AT"):
        assert ev.rel_fro(ev.near_virial(q, s, eb.T, None, alpha, r_c, mutant)[1], ev.near_virial(q, s, eb.T, None, alpha, r_c)[1]) >= 0.1
    band = np.random.default_rng(2).standard_normal((1, 8, 8, 8, 2)) + 1j
    b = eb.coeffs(eb.T, 4.0, 8)
    for mutant in ("k", "no_pi2"):
        assert ev.rel_fro(ev.far_virial(band, b, eb.T, 4.0, mutant)[1], ev.far_virial(band, b, eb.T, 4.0)[1]) >= 0.1


def test_virial_to_box_gradient(few):
    """tril(-A^-T W) against the difference quotient of the energy in each of the six free entries of A, at fixed s"""
    import torch_nfft_amd as tn
    s, q = few
    A = eb.T
    U, W = ev.converged_virial(q, s, A, kmax=10)
    G = tn.virial_to_box_gradient(torch.from_numpy(W), A)
    assert G.shape == (1, 3, 3, 2) and G.dtype == torch.float64
    G = G.numpy()
    worst = 0.0
    for i in range(3):
        for j in range(3):
            if j > i:
                assert not G[0, i, j].any()
                continue
            Ap, Am = A.copy(), A.copy()
            Ap[i, j] += H
            Am[i, j] -= H
            fd = (_energy(q, s, Ap, kmax=10) - _energy(q, s, Am, kmax=10)) / (2 * H)
            worst = max(worst, np.abs(G[0, i, j] - fd).max())
    print("box gradient against difference quotients: %.2e of %.3g" % (worst, np.abs(G).max()))
    assert np.abs(G).max() > 1.0 and worst <= 4 * 1.6e-9
    # the forms of `box`: three edges, None; columns and point sets pass through; float32 stays float32
    W32 = torch.randn(2, 3, 3, 5)
    W32 = W32 + W32.transpose(1, 2)
    g = tn.virial_to_box_gradient(W32, (1.0, 1.3, 0.8))
    assert g.shape == (2, 3, 3, 5) and g.dtype == torch.float32
    want = -np.einsum("ki,bkjc->bijc", np.linalg.inv(eb.O), W32.double().numpy()) * np.tril(np.ones((3, 3)))[None, :, :, None]
    assert np.abs(g.numpy() - want).max() <= 1e-6 * np.abs(want).max()
    assert torch.equal(tn.virial_to_box_gradient(W32, None), tn.virial_to_box_gradient(W32, (1, 1, 1)))
    assert torch.equal(tn.virial_to_box_gradient(W32, None), -torch.tril(W32.permute(0, 3, 1, 2)).permute(0, 2, 3, 1))
    assert tn.virial_to_box_gradient(W32[..., 0], eb.T).shape == (2, 3, 3)
    with pytest.raises(ValueError):
        tn.virial_to_box_gradient(torch.zeros(2, 3), None)
    with pytest.raises(ValueError):
        tn.virial_to_box_gradient(W32, eb.T.T)


def test_refusals_without_gpu():
    import torch_nfft_amd as tn
    assert "nfft_ewald_virial" in tn.__all__ and "virial_to_box_gradient" in tn.__all__
    sp = tn.EwaldSplitting(12.0, 0.3, 16, box=eb.T, device="cpu")
    cube = tn.EwaldSplitting(12.0, 0.3, 16, device="cpu")
    q, pos = torch.zeros(5), torch.zeros(5, 3)
    with pytest.raises(ValueError, match="real"):
        tn.nfft_ewald_virial(q.to(torch.complex64), pos, splitting=sp)
    with pytest.raises(ValueError, match="fractional"):
        tn.nfft_ewald_virial(q, pos, splitting=cube, fractional=True)
    with pytest.raises(ValueError, match="three-dimensional"):
        tn.nfft_ewald_virial(q, torch.zeros(5, 2), splitting=sp)
    with pytest.raises(TypeError):
        tn.nfft_ewald_virial(q, pos)
    with pytest.raises(AssertionError, match="batch holds point-set indices and must not require grad"):
        tn.nfft_ewald_virial(q, pos, torch.zeros(5, requires_grad=True), splitting=sp)
    with pytest.raises(AssertionError, match="differentiable w.r.t. q and pos only, but batch requires grad"):
        tn.nfft_ewald(q, pos, torch.zeros(5, requires_grad=True), splitting=sp)
    with pytest.raises(RuntimeError, match="is currently only implemented for GPU tensors"):
        tn.nfft_ewald_virial(q, pos, splitting=sp)
    s = str(torch.ops.torch_nfft._nfft_ewald_virial_near.default._schema)
    assert s == ("torch_nfft::_nfft_ewald_virial_near(Tensor pos, Tensor x, Tensor? batch, float[] box, float alpha, "
                 "float r_cut) -> Tensor")
    s = str(torch.ops.torch_nfft._nfft_ewald_virial_far.default._schema)
    assert s == "torch_nfft::_nfft_ewald_virial_far(Tensor band, Tensor coeffs, float[] box, float alpha) -> Tensor"
    with pytest.raises(RuntimeError, match="_nfft_ewald_virial_near is currently only implemented for GPU tensors"):
        tn.ops.nfft_ewald_virial_near(pos, q, None, sp.box6, 12.0, 0.3)
    with pytest.raises(RuntimeError, match="_nfft_ewald_virial_far is currently only implemented for GPU tensors"):
        tn.ops.nfft_ewald_virial_far(torch.zeros(1, 16, 16, 16, dtype=torch.complex64), sp.coeffs, sp.box6, 12.0)


def _six(A):
    A = np.asarray(A, dtype=np.float64)
    return (ctypes.c_double * 6)(A[0, 0], A[1, 0], A[1, 1], A[2, 0], A[2, 1], A[2, 2])


def test_c_abi_validation_without_gpu():
    from torch_nfft_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 7 and lib.nfft_hip_abi_version() == 7
    for name in ("nfft_hip_ewald_virial_near_workspace_bytes", "nfft_hip_ewald_virial_near",
                 "nfft_hip_ewald_virial_far_workspace_bytes", "nfft_hip_ewald_virial_far"):
        assert name in _lib.SYMBOLS

    def problem(A=eb.O, **kw):
        f = dict(cells=(4, 5, 3), with_field=0, num_points=1000, num_columns=2, batch_size=1, alpha=14.0, r_cut=0.25,
                 box=_six(A))
        f.update(kw)
        f["cells"] = (ctypes.c_int32 * 3)(*f["cells"])
        return _lib.EwaldBoxProblem(**f)

    ok = problem()
    slots = 1000 // 128 + 60 + 1
    need = lib.nfft_hip_ewald_virial_near_workspace_bytes(ctypes.byref(ok))
    assert need == (slots * 8 + 255) // 256 * 256 + slots * 7 * 2 * 8 + 256  # the items, one partial [7, Cr] float64 per slot
    for bad in (problem(cells=(5, 5, 3)), problem(cells=(2, 5, 3)), problem(with_field=2), problem(num_points=-1),
                problem(num_columns=-1), problem(batch_size=0), problem(alpha=0.0), problem(r_cut=0.0),
                problem(r_cut=0.27, cells=(3, 4, 3)), problem(num_columns=1 << 21), problem(batch_size=2048, num_columns=1 << 20)):
        assert lib.nfft_hip_ewald_virial_near_workspace_bytes(ctypes.byref(bad)) == -1
        assert _lib.last_error().startswith("Input mismatch")
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(256)  # (never dereferenced: the checks come first)

    def near(q, ws=null, nbytes=0, out=one, points=one):
        return lib.nfft_hip_ewald_virial_near(ctypes.byref(q), points, one, one, out, ws, nbytes, null)

    assert near(ok) == _lib.EWORKSPACE and _lib.last_error() == "workspace too small"
    assert near(ok, one, need - 1) == _lib.EWORKSPACE
    assert near(ok, out=null) == _lib.EINVAL and near(ok, points=null) == _lib.EINVAL
    assert near(problem(cells=(2, 5, 3))) == _lib.EINVAL
    assert near(problem(num_columns=0)) == _lib.OK  # nothing to do

    inv = _six(np.linalg.inv(eb.T))
    assert lib.nfft_hip_ewald_virial_far_workspace_bytes(6, 2, 3) == 2 * 1 * 7 * 3 * 8 + 256       # 216 cells: one workgroup
    assert lib.nfft_hip_ewald_virial_far_workspace_bytes(32, 2, 3) == 2 * 128 * 7 * 3 * 8 + 256    # 32^3 / 256
    assert lib.nfft_hip_ewald_virial_far_workspace_bytes(256, 1, 1) == 1024 * 7 * 8 + 256          # at most 1024 per set
    for N, B, C in ((7, 1, 1), (0, 1, 1), (4096, 1, 1), (8, 0, 1), (8, 1, -1), (8, 1 << 14, 1), (8, 2, 1 << 20)):
        assert lib.nfft_hip_ewald_virial_far_workspace_bytes(N, B, C) == -1
        assert _lib.last_error().startswith("Input mismatch")

    def far(N=8, B=1, C=1, band=one, coeffs=one, inv=inv, p2a2=0.1, out=one, ws=null, nbytes=0):
        return lib.nfft_hip_ewald_virial_far(N, B, C, band, coeffs, inv, p2a2, out, ws, nbytes, null)

    assert far() == _lib.EWORKSPACE
    assert far(ws=one, nbytes=lib.nfft_hip_ewald_virial_far_workspace_bytes(8, 1, 1) - 1) == _lib.EWORKSPACE
    nan = np.linalg.inv(eb.T)
    nan[1, 0] = float("nan")
    for kw in (dict(N=7), dict(band=null), dict(coeffs=null), dict(out=null), dict(p2a2=0.0), dict(p2a2=float("inf")),
               dict(inv=_six(nan)), dict(inv=_six(-np.eye(3))), dict(inv=None)):
        assert far(**kw) == _lib.EINVAL and _lib.last_error().startswith("Input mismatch")
    assert far(C=0) == _lib.OK  # nothing to do


def test_kernel_resource_usage():
    """every instantiation of the two reduction kernels: no scratch and no spills (the library's own flags; the VGPR and
    LDS figures are recorded in DESIGN.md section 7i, not gated)"""
    import re
    from resource_usage import resource_usage
    usage = resource_usage("ewald_virial.hip")
    seen = set()
    for name, u in sorted(usage.items()):
        # (the frames' kernels with this file's policies)
        m = re.search(r"(virial_near_kernel)ILi(\d)E\w*?CoulombVirialWeightE|(virial_far_kernel)ILi(\d)E\w*?CoulombStrainE|(virial_sum_kernel)", name)
        if not m:
            continue
        key = (m.group(1) or m.group(3) or m.group(5), int(m.group(2) or m.group(4) or 0))
        seen.add(key)
        print(key, "VGPRs %d AGPRs %d occupancy %d LDS %d" % (u["VGPRs"], u.get("AGPRs", 0), u["Occupancy"], u["LDS Size"]))
        assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (key, u)
    assert seen == {(k, cc) for k in ("virial_near_kernel", "virial_far_kernel") for cc in (1, 2, 4)} | {("virial_sum_kernel", 0)}
