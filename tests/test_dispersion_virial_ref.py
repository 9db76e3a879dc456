"""CPU tests of the virial tensor of the dispersion Ewald sum (nfft_ewald_dispersion_virial): the
float64 restatement tests/dispersion_virial_ref.py against strain difference quotients of the brute-force lattice sum, its
trace and its symmetry; the splitting's strain_coeffs() against the restatement; virial_to_box_gradient on this W; how far
off six wrong formulas are on the inputs of the GPU tests; exports, schemas, refusals, the C ABI's validation and the
registers of the two kernels."""
import ctypes
import re

import numpy as np
import pytest
import torch

import dispersion_ref as dr
import dispersion_virial_ref as dv
import ewald_box_ref as eb

BOXES = {"cube": np.eye(3), "T": eb.T, "O": eb.O}
H = 1e-5  # step of the central differences


@pytest.fixture(scope="module")
def few():
    """twelve fractional positions in [-1/2, 1/2)^3 with coefficients in [0.5, 1.5)"""
    rng = np.random.default_rng(5)
    return rng.random((12, 3)) - 0.5, rng.random(12) + 0.5


def _lattice_energy(c, s, A, R):
    return 0.5 * (c * dr.lattice_sum(c, s, A, R)[0]).sum()


@pytest.mark.parametrize("name", ["cube", "T", "O"])
def test_virial_is_the_strain_derivative_of_the_lattice_sum(few, name):
    """W_ab = -dU / d eps_ab for A -> A (1 + eps) at fixed s, all nine entries: the analytic W of the split (alpha = 3.2,
    N = 30, two shells of images) against central differences (h = 1e-5) of the energy of dr.lattice_sum, which knows
    nothing of the split.  Measured when this was written, relative to |W|_max = 5.9e6, 3.6e6, 4.8e6: 9.3e-7 (cube), 1.6e-7
    (T), 3.7e-7 (O) with every image within R = 10 as here (3.4e-7, 1.9e-8, 7.9e-8 within R = 14, at three times the
    time).  That is the quotient's own noise, not the formula's error: the lattice sum cuts sharply at |d| = R, the strain
    carries images across that sphere, and a sum that a few close pairs dominate is rounded at their size; it falls as R
    grows.  The bound is 4 x 9.3e-7.  U of the split against the lattice sum's energy (R = 14): 2.2e-11, 4.5e-11, 3.2e-11,
    bound 4 x 4.5e-11.  tr W = 6 U (psi is homogeneous of degree -6 in the box) to 4e-15; W = W^T to rounding."""
    s, c = few
    A = BOXES[name]
    U, W = dv.converged_virial(c, s, A)
    fd = np.zeros((3, 3))
    for a in range(3):
        for b in range(3):
            eps = np.zeros((3, 3))
            eps[a, b] = H
            fd[a, b] = -(_lattice_energy(c, s, A @ (np.eye(3) + eps), 10.0) - _lattice_energy(c, s, A @ (np.eye(3) - eps), 10.0)) / (2 * H)
    scale = np.abs(W).max()
    err = np.abs(W[0] - fd).max() / scale
    e_U = abs(U[0] - dv.converged_virial(c, s, A, R=14.0)[0][0]) / abs(U[0])
    e_tr = abs(np.trace(W[0]) / U[0] - 6.0)
    print("box %s: |W + dU/d eps|_max / |W|_max %.2e (|W|_max %.3g), U vs the lattice sum %.2e, tr W / U - 6 = %.1e"
          % (name, err, scale, e_U, e_tr))
    assert U.shape == (1,) and W.shape == (1, 3, 3) and scale > 1e6
    assert err <= 4 * 9.3e-7
    assert e_U <= 4 * 4.5e-11
    assert e_tr <= 1e-13
    assert np.abs(W - W.transpose(0, 2, 1)).max() <= 1e-15 * scale


def test_virial_does_not_depend_on_alpha_and_sets_add_up(few):
    s, c = few
    U0, W0 = dv.converged_virial(c, s, eb.T)
    U1, W1 = dv.converged_virial(c, s, eb.T, alpha=4.0)
    print("alpha 3.2 vs 4: W %.1e U %.1e" % (dv.rel_fro(W1, W0), dv.rel_fro(U1, U0)))
    assert dv.rel_fro(W1, W0) <= 1e-9 and dv.rel_fro(U1, U0) <= 1e-9
    # two sets with an empty one between them, two columns: each row is the sum of its own set, the empty one zero
    batch = np.array([0] * 5 + [2] * 7)
    c2 = np.stack([c, c[::-1]], 1)
    U, W = dv.exact_algorithm_virial(c2, s, eb.T, batch, 6.0, 0.3, 12)
    assert U.shape == (3, 2) and W.shape == (3, 3, 3, 2) and not U[1].any() and not W[1].any()
    for b, sel in ((0, slice(0, 5)), (2, slice(5, 12))):
        Ub, Wb = dv.exact_algorithm_virial(c2[sel, 1], s[sel], eb.T, None, 6.0, 0.3, 12)
        assert abs(Ub[0] - U[b, 1]) <= 1e-12 * abs(Ub[0]) and np.abs(Wb[0] - W[b, :, :, 1]).max() <= 1e-12 * np.abs(Wb).max()


def test_virial_to_box_gradient_takes_this_virial(few):
    """tril(-A^-T W) against the difference quotient of the split's energy in each of the six free entries of A, at fixed s
    (2.1e-10 of the largest entry, 2.7e6, when this was written -- the split's energy is smooth in the box, so what is left
    is the quotient's h^2 term and rounding; bound 4 x that)"""
    import torch_nfft_amd as tn
    s, c = few
    A = eb.T
    U, W = dv.converged_virial(c, s, A)
    G = tn.virial_to_box_gradient(torch.from_numpy(W), A).numpy()
    worst = 0.0
    for i in range(3):
        for j in range(i + 1):
            Ap, Am = A.copy(), A.copy()
            Ap[i, j] += H
            Am[i, j] -= H
            fd = (dv.converged_virial(c, s, Ap)[0][0] - dv.converged_virial(c, s, Am)[0][0]) / (2 * H)
            worst = max(worst, abs(G[0, i, j] - fd))
    print("box gradient against difference quotients: %.2e of %.3g" % (worst, np.abs(G).max()))
    assert not np.triu(G[0], 1).any() and np.abs(G).max() > 1e6
    assert worst <= 4 * 2.1e-10 * np.abs(G).max()


@pytest.mark.parametrize("name", ["cube", "T", "O"])
def test_strain_coeffs(name):
    import torch_nfft_amd as tn
    A = None if name == "cube" else BOXES[name]
    for alpha, N in ((11.5, 32), (6.0, 16)):
        sp = tn.DispersionSplitting(alpha, 0.25, N, box=None if A is None else torch.from_numpy(A), device="cpu")
        t = sp.strain_coeffs()
        assert t.shape == (N, N, N) and t.dtype == torch.float32 and t.device == sp.coeffs.device
        assert sp.strain_coeffs() is t  # built once
        want = dv.strain_coeffs(A, alpha, N)
        t = t.numpy()
        assert np.abs(t - want).max() <= 6e-8 * np.abs(want).max()  # (float32 rounding of float64 values)
        h = N // 2
        V = 1.0 if A is None else float(np.linalg.det(A))
        assert abs(t[h, h, h] + 2.0 * np.pi ** 3.5 * alpha / V) <= 6e-8 * abs(t[h, h, h]) and t[h, h, h] == t.min()
        assert (t <= 0).all()
        assert not t[0].any() and not t[:, 0].any() and not t[:, :, 0].any()
        assert not t[sp.coeffs.numpy() == 0].any()
        assert (t[1:, 1:, 1:] == t[1:, 1:, 1:][::-1, ::-1, ::-1]).all()  # t_k = t_-k
    # t_k is (d b_k / d |kappa|) / |kappa|: a central difference of the restatement's own f along b
    b = np.array([0.3, 1.0, 2.5, 4.0])
    fd = (dr.far_factor(b + 1e-6) - dr.far_factor(b - 1e-6)) / 2e-6 / (6.0 * b)
    assert np.abs(dv.strain_factor(b) - fd).max() <= 1e-9
    assert dv.strain_factor(0.0) == -1.0 and (dv.strain_factor(np.array([30.0, 1e3])) == 0).all()
    import torch_nfft_amd.dispersion as d
    bb = np.array([0.0, 0.3, 3.0, 5.0, 8.0])
    assert np.abs(d._strain_factor(torch.from_numpy(bb)).numpy() - dv.strain_factor(bb)).max() <= 1e-16


# box, alpha, r_c of the GPU near tests (alpha r_c = 1.5, the cells of tests/test_gpu_ewald_virial.py)
NEAR_SPLITS = [("O", 6.0, 0.25), ("T", 5.0, 0.3), ("T", 12.5, 0.12), ("S", 7.0, 0.22), ("I", 5.0, 0.3)]
NEAR_BOXES = {"T": eb.T, "O": eb.O, "S": eb.S, "I": np.eye(3)}
CEILING = 1e-4  # what a first device run may show at most (tests/test_gpu_dispersion_virial.py)


def test_mutants_are_far_off():
    """On the very inputs of the GPU tests each of six wrong formulas moves W by at least three times the ceiling of a
    device run's error.  Measured when this was written (relative Frobenius norm of the change of W):
    near, the 700 points -- the fractional difference in place of d 0.37 .. 1.6 (O, T, S; nothing in the identity box), A^T
    in place of A 0.23 .. 0.85 (T and S; O and I are symmetric), a^6 dropped from mg 1.2e-3 .. 1.2e-2: the pairs 0.02 ..
    0.05 apart that carry most of W have a << 1, so this one needs the loose alpha r_c = 1.5 to show at all;
    far, the bands of N = 6, 8, 12, 32 -- k in place of kappa 0.08 .. 2.9, t_k left out 0.19 .. 6.7, the k = 0 term left
    out 0.61 .. 1.0;
    whole, the 343 points in T at (14, 0.25, 32) -- 0.25, 0.31, 0.16, 0.36, 0.82, 0.61 in the order above."""
    x = dv.near_points()
    c = dv.values(np.random.default_rng(1), 700, ())
    for name, alpha, r_c in NEAR_SPLITS:
        A = NEAR_BOXES[name]
        W = dv.near_virial(c, x, A, None, alpha, r_c)[1]
        for mutant in ("ds", "AT", "top_term"):
            move = dv.rel_fro(dv.near_virial(c, x, A, None, alpha, r_c, mutant)[1], W)
            print("near %s (%g, %g) mutant %-8s moves W by %.3e" % (name, alpha, r_c, mutant, move))
            if (mutant == "ds" and name == "I") or (mutant == "AT" and name in ("O", "I")):
                assert move == 0.0  # (the same formula in that box)
            else:
                assert move >= 3 * CEILING
    for N, name in ((6, "T"), (8, "O"), (12, "T"), (32, "O")):
        A, alpha = NEAR_BOXES[name], dv.far_alpha(N)
        band = dv.far_band(N, name, ())
        b, t = dr.coeffs(A, alpha, N), dv.strain_coeffs(A, alpha, N)
        W = dv.far_virial(band, b, t, A)[1]
        for mutant in ("k", "no_t", "no_k0"):
            move = dv.rel_fro(dv.far_virial(band, b, t, A, mutant)[1], W)
            print("far N %d %s mutant %-6s moves W by %.3e" % (N, name, mutant, move))
            assert move >= 3 * CEILING
    s, c, batch = dv.whole_points()
    alpha, r_c, N = dv.WHOLE
    W = dv.exact_algorithm_virial(c, s, eb.T, batch, alpha, r_c, N)[1]
    for mutant in ("ds", "AT", "top_term", "k", "no_t", "no_k0"):
        move = dv.rel_fro(dv.exact_algorithm_virial(c, s, eb.T, batch, alpha, r_c, N, mutant)[1], W)
        print("whole T mutant %-8s moves W by %.3e" % (mutant, move))
        assert move >= 3 * CEILING


def test_gpu_point_sets():
    """what tests/test_gpu_dispersion_virial.py relies on: no pair of the 700 points closer than 0.018 (the exact duplicates
    apart), so no single 1/r^8 is the whole sum; the first hundred in one point set"""
    x = dv.near_points()
    assert x.shape == (700, 3) and x.dtype == np.float32
    assert (x[40:60] == x[0:20]).all() and (np.abs(x[72:88]) > 0.5).any()
    for name, A in NEAR_BOXES.items():
        assert dr.min_separation(x, A) >= 0.018
    assert (dv.ragged_batch()[:100] == 0).all() and set(dv.ragged_batch()) == {0, 2}


def test_exports_schemas_and_refusals():
    import torch_nfft
    import torch_nfft_amd as tn
    assert "nfft_ewald_dispersion_virial" in tn.__all__ and torch_nfft.nfft_ewald_dispersion_virial is tn.nfft_ewald_dispersion_virial
    s = str(torch.ops.torch_nfft._nfft_ewald_dispersion_virial_near.default._schema)
    assert s == ("torch_nfft::_nfft_ewald_dispersion_virial_near(Tensor pos, Tensor x, Tensor? batch, float[] box, "
                 "float alpha, float r_cut) -> Tensor")
    s = str(torch.ops.torch_nfft._nfft_ewald_dispersion_virial_far.default._schema)
    assert s == ("torch_nfft::_nfft_ewald_dispersion_virial_far(Tensor band, Tensor coeffs, Tensor strain_coeffs, float[] box) "
                 "-> Tensor")
    sp = tn.DispersionSplitting(6.0, 0.25, 16, box=torch.from_numpy(eb.T), device="cpu")
    cube = tn.DispersionSplitting(6.0, 0.3, 16, device="cpu")
    c, pos = torch.zeros(5), torch.zeros(5, 3)
    with pytest.raises(ValueError, match="real"):
        tn.nfft_ewald_dispersion_virial(c.to(torch.complex64), pos, splitting=sp)
    with pytest.raises(ValueError, match="fractional"):
        tn.nfft_ewald_dispersion_virial(c, pos, splitting=cube, fractional=True)
    with pytest.raises(ValueError, match="three-dimensional"):
        tn.nfft_ewald_dispersion_virial(c, torch.zeros(5, 2), splitting=sp)
    with pytest.raises(TypeError, match="DispersionSplitting"):
        tn.nfft_ewald_dispersion_virial(c, pos)
    with pytest.raises(TypeError, match="DispersionSplitting"):  # the Coulomb splitting is the wrong class
        tn.nfft_ewald_dispersion_virial(c, pos, splitting=tn.EwaldSplitting(6.0, 0.3, 16, device="cpu"))
    with pytest.raises(TypeError):  # ... and the other way round
        tn.nfft_ewald_virial(c, pos, splitting=sp)
    with pytest.raises(AssertionError, match="batch holds point-set indices and must not require grad"):
        tn.nfft_ewald_dispersion_virial(c, pos, torch.zeros(5, requires_grad=True), splitting=sp)
    with pytest.raises(AssertionError, match="differentiable w.r.t. c and pos only, but batch requires grad"):
        tn.nfft_ewald_dispersion(c, pos, torch.zeros(5, requires_grad=True), splitting=sp)
    for splitting in (sp, cube):
        with pytest.raises(RuntimeError, match="is currently only implemented for GPU tensors"):
            tn.nfft_ewald_dispersion_virial(c, pos, splitting=splitting)
    with pytest.raises(RuntimeError, match="_nfft_ewald_dispersion_virial_near is currently only implemented for GPU tensors"):
        tn.ops.nfft_ewald_dispersion_virial_near(pos, c, None, sp.box6, 6.0, 0.25)
    with pytest.raises(RuntimeError, match="_nfft_ewald_dispersion_virial_far is currently only implemented for GPU tensors"):
        tn.ops.nfft_ewald_dispersion_virial_far(torch.zeros(1, 16, 16, 16, dtype=torch.complex64), sp.coeffs, sp.strain_coeffs(),
                                                sp.box6)


def _six(A):
    A = np.asarray(A, dtype=np.float64)
    return (ctypes.c_double * 6)(A[0, 0], A[1, 0], A[1, 1], A[2, 0], A[2, 1], A[2, 2])


def test_c_abi_validation_without_gpu():
    """the two entry points validate as their Coulomb twins do and take the workspaces that the shared functions report"""
    from torch_nfft_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 7 and lib.nfft_hip_abi_version() == 7
    for name in ("nfft_hip_ewald_dispersion_virial_near", "nfft_hip_ewald_dispersion_virial_far"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)

    def problem(A=eb.O, **kw):
        f = dict(cells=(4, 5, 3), with_field=0, num_points=1000, num_columns=2, batch_size=1, alpha=6.0, r_cut=0.25,
                 box=_six(A))
        f.update(kw)
        f["cells"] = (ctypes.c_int32 * 3)(*f["cells"])
        return _lib.EwaldBoxProblem(**f)

    ok = problem()
    need = lib.nfft_hip_ewald_virial_near_workspace_bytes(ctypes.byref(ok))
    assert need > 0
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(256)  # (never dereferenced: the checks come first)

    def near(q, ws=null, nbytes=0, out=one, points=one):
        return lib.nfft_hip_ewald_dispersion_virial_near(ctypes.byref(q), points, one, one, out, ws, nbytes, null)

    assert near(ok) == _lib.EWORKSPACE and _lib.last_error() == "workspace too small"
    assert near(ok, one, need - 1) == _lib.EWORKSPACE
    assert near(ok, out=null) == _lib.EINVAL and near(ok, points=null) == _lib.EINVAL
    for bad in (problem(cells=(5, 5, 3)), problem(cells=(2, 5, 3)), problem(with_field=2), problem(num_points=-1),
                problem(num_columns=-1), problem(batch_size=0), problem(alpha=0.0), problem(r_cut=0.0),
                problem(r_cut=0.27, cells=(3, 4, 3)), problem(num_columns=1 << 21), problem(batch_size=2048, num_columns=1 << 20)):
        assert near(bad) == _lib.EINVAL and _lib.last_error().startswith("Input mismatch")
    assert near(problem(num_columns=0)) == _lib.OK  # nothing to do

    inv = _six(np.linalg.inv(eb.T))

    def far(N=8, B=1, C=1, band=one, coeffs=one, strain=one, inv=inv, out=one, ws=null, nbytes=0):
        return lib.nfft_hip_ewald_dispersion_virial_far(N, B, C, band, coeffs, strain, inv, out, ws, nbytes, null)

    assert far() == _lib.EWORKSPACE and _lib.last_error() == "workspace too small"
    assert far(ws=one, nbytes=lib.nfft_hip_ewald_virial_far_workspace_bytes(8, 1, 1) - 1) == _lib.EWORKSPACE
    nan = np.linalg.inv(eb.T)
    nan[1, 0] = float("nan")
    for kw in (dict(N=7), dict(N=0), dict(B=0), dict(C=-1), dict(band=null), dict(coeffs=null), dict(strain=null), dict(out=null),
               dict(inv=_six(nan)), dict(inv=_six(-np.eye(3))), dict(inv=None)):
        assert far(**kw) == _lib.EINVAL and _lib.last_error().startswith("Input mismatch")
    assert far(C=0) == _lib.OK  # nothing to do


def test_kernel_resource_usage():
    """exactly the six instantiations of the two reduction kernels, each without scratch and without spills (the library's
    own flags; the VGPR, occupancy and LDS figures are recorded in DESIGN.md section 7k, not gated)"""
    from resource_usage import resource_usage
    usage = resource_usage("ewald_disp_virial.hip")
    seen = set()
    for name, u in sorted(usage.items()):
        # (the frames' kernels with this file's policies)
        m = re.search(r"(virial_near_kernel)ILi(\d)E\w*?DispersionVirialWeightE|(virial_far_kernel)ILi(\d)E\w*?TableStrainE", name)
        assert m, name  # (nothing else in that file)
        key = (m.group(1) or m.group(3), int(m.group(2) or m.group(4)))
        seen.add(key)
        print(key, "VGPRs %d AGPRs %d occupancy %d LDS %d" % (u["VGPRs"], u.get("AGPRs", 0), u["Occupancy"], u["LDS Size"]))
        assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (key, u)
    assert seen == {(k, cc) for k in ("virial_near_kernel", "virial_far_kernel") for cc in (1, 2, 4)}
    assert len(usage) == 6
