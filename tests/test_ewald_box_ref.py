"""CPU tests of the Ewald sum in orthorhombic and triclinic boxes: the float64 restatement
tests/ewald_box_ref.py against the fixed points of the lattice sums, against tests/ewald_ref.py on the identity box and
against itself, the host-side pieces of torch_nfft_amd/ewald.py against the restatement, the refusals and the C ABI's
validation."""
import ctypes
import math

import numpy as np
import pytest
import torch

import ewald_box_ref as eb
import ewald_ref as er
from conftest import rel_l2

BOXES = {"T": eb.T, "O": eb.O, "S": eb.S}


@pytest.fixture(scope="module")
def charges():
    """300 float32 fractional positions with neutral float64 charges (those of tests/test_ewald_ref.py)"""
    rng = np.random.default_rng(0)
    s = (rng.random((300, 3)) - 0.5).astype(np.float32)
    q = rng.standard_normal(300)
    q -= q.mean()
    return s, q


def test_sheared_cubic_lattice_and_primitive_rock_salt():
    # the cell S spans the cubic lattice: one charge sees the cubic-lattice constant, wherever it sits.  (alpha = 5 and 6:
    # the longest lattice vector is sqrt(2), so |k|_inf <= 14 reaches |kappa| = 10.6 only, too little for a larger alpha)
    for alpha in (5.0, 6.0):
        for pos in ([0.0, 0.0, 0.0], [0.31, -0.47, 0.123]):
            phi = eb.converged(np.array([1.5]), np.array([pos]), eb.S, alpha=alpha)
            print("sheared cell, alpha %g, s = %s: phi / q = %.10f" % (alpha, pos, phi[0] / 1.5))
            assert abs(phi[0] / 1.5 + 2.8372974795) <= 1e-9
    # two ions in the primitive fcc cell, nearest distance 1/2: phi_i = -2 M q_i
    A, Q = eb.lower_triangular(eb.ROCK_SALT_PRIMITIVE)
    assert np.abs(np.triu(A, 1)).max() == 0 and (np.diag(A) > 0).all()
    assert np.abs(A @ Q.T - eb.ROCK_SALT_PRIMITIVE).max() <= 1e-15 and np.abs(Q @ Q.T - np.eye(3)).max() <= 1e-15
    s = np.array([[0.0, 0.0, 0.0], [-0.5, -0.5, -0.5]])
    q = np.array([1.0, -1.0])
    for alpha in (6.0, 8.0):
        phi = eb.converged(q, s, A, alpha=alpha)
        print("primitive rock salt, alpha %g: phi / q = %s" % (alpha, phi / q))
        assert np.abs(phi / q + 3.4951291892).max() <= 1e-9
        assert np.abs(phi / q + 2.0 * er.MADELUNG_NACL).max() <= 1e-9
    # the same sum in the cell as it was given (not triangular): the restatement does not need the QR
    assert np.abs(eb.converged(q, s, eb.ROCK_SALT_PRIMITIVE) / q + 3.4951291892).max() <= 1e-9


def test_identity_box_is_the_unit_cube(charges):
    s, q = charges
    I = np.eye(3)
    batch = (np.arange(300) >= 130).astype(np.int64)
    q2 = np.stack([q, q[::-1] ** 2], 1)
    assert rel_l2(eb.near_sum(q2, s, I, batch, 12.0, 0.3), er.near_sum(q2, s, batch, 12.0, 0.3)) <= 1e-12
    assert rel_l2(eb.near_field(q2, s, I, batch, 12.0, 0.3), er.near_field(q2, s, batch, 12.0, 0.3)) <= 1e-12
    assert rel_l2(eb.coeffs(I, 12.0, 32), er.coeffs(12.0, 32)) <= 1e-12
    a, b = eb.exact_algorithm(q2, s, I, batch, 12.0, 0.3, 16, field=True), er.exact_algorithm(q2, s, batch, 12.0, 0.3, 16, field=True)
    assert rel_l2(a[0], b[0]) <= 1e-12 and rel_l2(a[1], b[1]) <= 1e-12
    assert rel_l2(eb.exact_algorithm(q, s, I, None, 12.0, 0.3, 16), er.exact_algorithm(q, s, None, 12.0, 0.3, 16)) <= 1e-12
    a, b = eb.converged(q2[:120], s[:120], I, field=True), er.converged(q2[:120], s[:120], field=True)
    assert rel_l2(a[0], b[0]) <= 1e-12 and rel_l2(a[1], b[1]) <= 1e-12


@pytest.mark.parametrize("name,alpha,r_c", [("O", 14.0, 0.25), ("T", 12.0, 0.3), ("T", 14.0, 0.25), ("S", 16.0, 0.22),
                                            ("T", 12.0, None), ("S", 12.0, None)])
def test_componentwise_rint_finds_every_image(charges, name, alpha, r_c):
    """r_c <= min w_a / 3 (None: exactly there): the componentwise rint of ds is the only image within r_c"""
    s, q = charges
    A = BOXES[name]
    r_c = eb.widths(A).min() / 3.0 if r_c is None else r_c
    z, f = eb.near_sum(q, s, A, None, alpha, r_c), eb.near_field(q, s, A, None, alpha, r_c)
    za, fa = eb.near_all_images(q, s, A, None, alpha, r_c)
    print("box %s r_c %.4f: rint vs all images, value %.1e field %.1e" % (name, r_c, rel_l2(z, za), rel_l2(f, fa)))
    assert np.linalg.norm(za) > 0 and rel_l2(z, za) <= 1e-14 and rel_l2(f, fa) <= 1e-14


def test_field_is_the_cartesian_gradient_of_the_energy():
    """E_i q_i = -dU/dx_i in the Cartesian position, by central differences (h = 1e-5), for the converged sum and for the
    algorithm's own field in the triclinic box"""
    rng = np.random.default_rng(2)
    n = 12
    A, inv = eb.T, np.linalg.inv(eb.T)
    x = (rng.random((n, 3)) - 0.5) @ A
    q = rng.standard_normal(n)
    _, E = eb.converged(q, x @ inv, A, field=True)
    h = 1e-5

    def energy(fn, xx):
        return 0.5 * (q * fn(xx @ inv)).sum()

    def conv(s):
        return eb.converged(q, s, A)

    for i, a in ((0, 0), (5, 1), (11, 2)):
        xp, xm = x.copy(), x.copy()
        xp[i, a] += h
        xm[i, a] -= h
        dU = (energy(conv, xp) - energy(conv, xm)) / (2 * h)
        assert abs(-dU - q[i] * E[i, a]) <= 1e-6 * np.abs(q[:, None] * E).max()

    def alg(s):
        return eb.exact_algorithm(q, s, A, None, 7.0, 0.3, 16)

    phi_alg, E_alg = eb.exact_algorithm(q, x @ inv, A, None, 7.0, 0.3, 16, field=True)
    assert rel_l2(phi_alg, alg(x @ inv)) <= 1e-13
    ds = (x[:, None, :] - x[None, :, :]) @ inv
    r = np.sqrt(((((ds - np.rint(ds)) @ A)) ** 2).sum(-1))
    assert np.abs(r - 0.3).min() > 10 * h  # (no pair may cross r_c between the two evaluations)
    for i, a in ((3, 0), (3, 1), (7, 2)):
        xp, xm = x.copy(), x.copy()
        xp[i, a] += h
        xm[i, a] -= h
        dU = (energy(alg, xp) - energy(alg, xm)) / (2 * h)
        assert abs(-dU - q[i] * E_alg[i, a]) <= 1e-6 * np.abs(q[:, None] * E_alg).max()


# box, (alpha, r_c, N), the truncation error of phi and of E (relative l2 on the 300 neutral charges), the cells
TRUNCATION = [("T", (12.0, 0.3, 32), 1.03e-7, 4.67e-7, (3, 3, 3)),
              ("T", (14.0, 0.25, 48), 1.86e-7, 9.93e-7, (3, 4, 3)),
              ("O", (14.0, 0.25, 48), 1.74e-7, 9.27e-7, (4, 5, 3)),
              ("S", (16.0, 0.22, 48), 2.40e-7, 1.05e-6, (3, 4, 4))]


@pytest.mark.parametrize("name,split,phi_err,E_err,cells", TRUNCATION)
def test_exact_algorithm_against_converged(charges, name, split, phi_err, E_err, cells):
    s, q = charges
    A = BOXES[name]
    alpha, r_c, N = split
    conv = eb.converged(q, s, A, field=True)
    alg = eb.exact_algorithm(q, s, A, None, alpha, r_c, N, field=True)
    e_phi, e_E = rel_l2(alg[0], conv[0]), rel_l2(alg[1], conv[1])
    print("box %s (%g, %g, %d): phi %.3e (recorded %.2e), E %.3e (recorded %.2e)" % (name, alpha, r_c, N, e_phi, phi_err,
                                                                                      e_E, E_err))
    assert e_phi <= 1.5 * phi_err and e_E <= 1.5 * E_err
    assert tuple(int(g) for g in np.floor(eb.widths(A) / r_c)) == cells


def test_converged_does_not_depend_on_alpha(charges):
    s, q = charges
    qn = np.random.default_rng(1).standard_normal(120)  # not neutral: the background term carries 1 / V
    for A in (eb.T, eb.O):
        assert rel_l2(eb.converged(qn, s[:120], A, alpha=7.0), eb.converged(qn, s[:120], A)) <= 1e-11


def test_splitting_with_a_box():
    import torch_nfft_amd as tn
    for name, (alpha, r_c, N), cells in (("T", (12.0, 0.3, 32), (3, 3, 3)), ("T", (14.0, 0.25, 16), (3, 4, 3)),
                                         ("T", (30.0, 0.12, 16), (7, 8, 7)), ("O", (14.0, 0.25, 16), (4, 5, 3)),
                                         ("S", (16.0, 0.22, 16), (3, 4, 4))):
        A = BOXES[name]
        sp = tn.EwaldSplitting(alpha, r_c, N, box=A, device="cpu")
        assert sp.cells == cells
        assert sp.box.dtype == torch.float64 and np.array_equal(sp.box.numpy(), A)
        assert abs(sp.volume - np.linalg.det(A)) <= 1e-15 and np.abs(np.array(sp.widths) - eb.widths(A)).max() <= 1e-15
        want = eb.coeffs(A, alpha, N)
        b = sp.coeffs.numpy()
        assert b.shape == (N, N, N) and b.dtype == np.float32
        assert np.abs(b - want).max() <= 6e-8 * np.abs(want).max()  # (float32 rounding of float64 values)
        assert b[N // 2, N // 2, N // 2] == 0 and not b[0].any() and not b[:, 0].any() and not b[:, :, 0].any()
        assert (b[1:, 1:, 1:] == b[1:, 1:, 1:][::-1, ::-1, ::-1]).all()  # even: a real q gives a real phi
        fc = sp.field_coeffs().numpy()
        assert fc.shape == (N, N, N, 4) and fc.dtype == np.complex64
        kappa = eb._kappa(A, N)
        assert rel_l2(fc[..., 0], want) <= 1e-7
        for a in range(3):
            assert rel_l2(fc[..., 1 + a], 2j * math.pi * kappa[..., a] * want) <= 1e-7
    # an orthorhombic box as three edges, a tensor, a list of rows
    sp = tn.EwaldSplitting(14.0, 0.25, 16, box=(1.0, 1.3, 0.8), device="cpu")
    assert np.array_equal(sp.box.numpy(), eb.O) and sp.cells == (4, 5, 3) and np.allclose(sp.widths, (1.0, 1.3, 0.8), rtol=1e-15, atol=0)
    assert torch.equal(tn.EwaldSplitting(14.0, 0.25, 16, box=torch.tensor(eb.T), device="cpu").coeffs,
                       tn.EwaldSplitting(14.0, 0.25, 16, box=eb.T.tolist(), device="cpu").coeffs)
    # the identity box has the unit cube's coefficients (to rounding: kappa = k) and box=None is the old splitting, bit for bit
    old = tn.EwaldSplitting(12.0, 0.3, 32, device="cpu")
    assert old.box is None and old.volume == 1.0 and old.widths == (1.0, 1.0, 1.0) and old.cells == (3, 3, 3)
    ident = tn.EwaldSplitting(12.0, 0.3, 32, box=(1, 1, 1), device="cpu")
    assert np.abs(ident.coeffs.numpy() - old.coeffs.numpy()).max() <= 6e-8 * float(old.coeffs.max())
    assert rel_l2(ident.field_coeffs().numpy(), old.field_coeffs().numpy()) <= 2e-7
    assert tn.EwaldSplitting(12.0, 1.0 / 3.0, 16, box=(1, 1, 1), device="cpu").cells == (3, 3, 3)


def test_box_none_keeps_the_old_coefficients():
    """the coefficients of the unit cube, restated the way EwaldSplitting built them before it knew boxes"""
    import torch_nfft_amd as tn
    for alpha, N in ((12.0, 32), (7.5, 16)):
        k = torch.arange(-(N // 2), N // 2, dtype=torch.float64)
        k2 = (k * k).reshape(N, 1, 1) + (k * k).reshape(1, N, 1) + (k * k).reshape(1, 1, N)
        b = torch.exp(-(math.pi / alpha) ** 2 * k2) / (math.pi * k2.clamp(min=1.0))
        b[N // 2, N // 2, N // 2] = 0.0
        b[0, :, :] = 0.0
        b[:, 0, :] = 0.0
        b[:, :, 0] = 0.0
        b = b.to(torch.float32)
        sp = tn.EwaldSplitting(alpha, 0.3, N, device="cpu")
        assert torch.equal(sp.coeffs, b)
        freq = 2.0 * math.pi * torch.arange(-(N // 2), N // 2, dtype=torch.float32)
        assert torch.equal(sp.field_coeffs()[..., 2], torch.complex(torch.zeros_like(b), b * freq.reshape(1, N, 1)))


def test_from_tolerance_with_a_box():
    import torch_nfft_amd as tn
    s = math.sqrt(-math.log(1e-6))
    for A in (eb.T, eb.O, eb.S):
        sp = tn.EwaldSplitting.from_tolerance(1e-6, 0.22, box=A, device="cpu")
        longest = np.linalg.norm(A, axis=1).max()
        assert sp.r_cut == 0.22 and abs(sp.alpha - s / 0.22) <= 1e-12
        lower = 2 * sp.alpha * s * longest / math.pi
        assert sp.bandwidth % 2 == 0 and lower <= sp.bandwidth < lower + 2
        # the far sum's factor on the planes k_a = N/2, at their distance (N/2) / |a_a| from the origin
        assert math.exp(-(math.pi * (sp.bandwidth / 2) / longest / sp.alpha) ** 2) <= 1e-6
    old = tn.EwaldSplitting.from_tolerance(1e-6, 0.3, device="cpu")
    new = tn.EwaldSplitting.from_tolerance(1e-6, 0.3, box=(1, 1, 1), device="cpu")
    assert (old.alpha, old.bandwidth) == (new.alpha, new.bandwidth)
    with pytest.raises(ValueError):
        tn.EwaldSplitting.from_tolerance(1e-6, 0.31, box=eb.T, device="cpu")


def test_refusals():
    import torch_nfft_amd as tn
    wmin = eb.widths(eb.T).min()
    assert tn.EwaldSplitting(12.0, wmin / 3.0 * (1 - 1e-15), 16, box=eb.T, device="cpu").cells[0] == 3
    upper = eb.T.copy()
    upper[0, 2] = 1e-3
    zero = eb.T.copy()
    zero[1, 1] = 0.0
    for bad in (dict(r_cut=wmin / 3.0 * (1 + 1e-9)), dict(r_cut=0.0), dict(box=upper), dict(box=zero), dict(box=eb.T.T),
                dict(box=(1.0, -1.0, 1.0)), dict(box=(1.0, 1.0)), dict(box=np.ones((3, 2))),
                dict(box=(1.0, float("nan"), 1.0)), dict(bandwidth=31), dict(alpha=0.0)):
        kw = dict(alpha=12.0, r_cut=0.3, bandwidth=16, box=eb.T, device="cpu")
        kw.update(bad)
        with pytest.raises(ValueError):
            tn.EwaldSplitting(**kw)
    with pytest.raises(AssertionError, match="box requires grad"):
        tn.EwaldSplitting(12.0, 0.3, 16, box=torch.tensor(eb.T, requires_grad=True), device="cpu")
    cube = tn.EwaldSplitting(12.0, 0.3, 16, device="cpu")
    sp = tn.EwaldSplitting(12.0, 0.3, 16, box=eb.T, device="cpu")
    q, pos = torch.zeros(5), torch.zeros(5, 3)
    for fn in (tn.nfft_ewald, tn.nfft_ewald_energy):
        with pytest.raises(ValueError, match="fractional"):
            fn(q, pos, splitting=cube, fractional=True)
        for fractional in (False, True):
            with pytest.raises(RuntimeError, match="is currently only implemented for GPU tensors"):
                fn(q, pos, splitting=sp, fractional=fractional)
        with pytest.raises(ValueError, match="three-dimensional"):
            fn(q, torch.zeros(5, 2), splitting=sp)
    s = str(torch.ops.torch_nfft._nfft_ewald_near_box.default._schema)
    assert s == ("torch_nfft::_nfft_ewald_near_box(Tensor pos, Tensor x, Tensor? batch, float[] box, float alpha, "
                 "float r_cut, bool with_field) -> (Tensor, Tensor)")
    with pytest.raises(RuntimeError, match="torch_nfft._nfft_ewald_near_box is currently only implemented for GPU tensors"):
        tn.ops.nfft_ewald_near_box(pos, q, None, sp.box6, 12.0, 0.3, True)


def _six(A):
    A = np.asarray(A, dtype=np.float64)
    return (ctypes.c_double * 6)(A[0, 0], A[1, 0], A[1, 1], A[2, 0], A[2, 1], A[2, 2])


def test_c_abi_validation_without_gpu():
    from torch_nfft_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 7 and lib.nfft_hip_abi_version() == 7
    for name in ("nfft_hip_ewald_box_cells", "nfft_hip_ewald_near_box_workspace_bytes", "nfft_hip_ewald_near_box"):
        assert name in _lib.SYMBOLS

    def cells(A, r_cut, batch=1):
        out = (ctypes.c_int32 * 3)(-7, -7, -7)
        rc = lib.nfft_hip_ewald_box_cells(_six(A), r_cut, batch, out)
        return tuple(out) if rc == 0 else rc

    assert cells(eb.O, 0.25) == (4, 5, 3)
    assert cells(eb.T, 0.3) == (3, 3, 3) and cells(eb.T, 0.25) == (3, 4, 3) and cells(eb.T, 0.12) == (7, 8, 7)
    assert cells(eb.S, 0.22) == (3, 4, 4)
    assert cells(np.eye(3), 1.0 / 3.0) == (3, 3, 3) and cells(np.eye(3), 0.12) == (8, 8, 8)
    assert cells(np.diag([2.0, 2.0, 2.0]), 2.0 / 3.0) == (3, 3, 3)
    # too many cells: the largest count is lowered first, until batch_size G0 G1 G2 <= 2^20
    assert cells(np.eye(3), 0.01, 2) == (80, 80, 81)  # 100^3 -> 2 * 80 * 80 * 81 <= 2^20 < 2 * 80 * 81 * 81
    g = cells(eb.O, 0.005)  # (200, 260, 160) proposed
    assert g[0] * g[1] * g[2] <= 1 << 20 < g[0] * g[1] * g[2] // min(g) * (min(g) + 1) and max(g) - min(g) <= 1
    assert cells(eb.O, 0.25, 20000) == (4, 4, 3)  # 20000 * 60 > 2^20 >= 20000 * 48
    assert cells(eb.O, 0.25, 1 << 15) == (3, 3, 3)
    zero, nan = eb.T.copy(), eb.T.copy()
    zero[2, 2] = 0.0
    nan[1, 0] = float("nan")
    wmin = eb.widths(eb.T).min()
    for A, r_cut, batch in ((eb.T, wmin / 3 * (1 + 1e-9), 1), (eb.T, 0.0, 1), (eb.T, -0.1, 1), (eb.T, float("nan"), 1),
                            (zero, 0.1, 1), (-eb.T, 0.1, 1), (nan, 0.1, 1), (np.tril(np.full((3, 3), np.inf)), 0.1, 1), (eb.T, 0.3, 0),
                            (eb.T, 0.3, 1 << 20), (eb.O, 0.25, 1 << 16)):
        assert cells(A, r_cut, batch) == -1
        assert _lib.last_error().startswith("Input mismatch")

    def problem(A=eb.O, **kw):
        f = dict(cells=(ctypes.c_int32 * 3)(4, 5, 3), with_field=1, num_points=1000, num_columns=2, batch_size=1, alpha=14.0,
                 r_cut=0.25, box=_six(A))
        f.update(kw)
        if isinstance(f["cells"], tuple):
            f["cells"] = (ctypes.c_int32 * 3)(*f["cells"])
        return _lib.EwaldBoxProblem(**f)

    ok = problem()
    need = lib.nfft_hip_ewald_near_box_workspace_bytes(ctypes.byref(ok))
    assert need == (1000 // 128 + 60 + 1) * 8 + 256
    assert lib.nfft_hip_ewald_near_box_workspace_bytes(ctypes.byref(problem(cells=(3, 4, 3)))) > 0  # (coarser cells are valid)
    for bad in (problem(cells=(5, 5, 3)), problem(cells=(4, 6, 3)), problem(cells=(4, 5, 4)), problem(cells=(2, 5, 3)),
                problem(cells=(5, 4, 3)), problem(with_field=2), problem(num_points=-1), problem(num_columns=-1),
                problem(batch_size=0), problem(alpha=0.0), problem(alpha=float("nan")), problem(r_cut=0.27, cells=(3, 4, 3)),
                problem(r_cut=0.0), problem(num_points=1 << 31), problem(batch_size=1 << 15), problem(A=zero), problem(A=nan)):
        assert lib.nfft_hip_ewald_near_box_workspace_bytes(ctypes.byref(bad)) == -1
        assert _lib.last_error().startswith("Input mismatch")
    assert lib.nfft_hip_ewald_near_box_workspace_bytes(None) == -1
    null = ctypes.c_void_p(0)
    one = ctypes.c_void_p(256)  # (never dereferenced: the checks come first)

    def call(q, ws=null, nbytes=0, z=one, field=one, points=one):
        return lib.nfft_hip_ewald_near_box(ctypes.byref(q), points, one, one, one, z, field, ws, nbytes, null)

    assert call(ok) == _lib.EWORKSPACE and _lib.last_error() == "workspace too small"
    assert call(ok, one, need - 1) == _lib.EWORKSPACE
    assert call(problem(with_field=0), field=null) == _lib.EWORKSPACE  # (the field is not asked for: no pointer needed)
    assert call(ok, field=null) == _lib.EINVAL and _lib.last_error().startswith("Input mismatch")
    assert call(ok, z=null) == _lib.EINVAL
    assert call(ok, points=null) == _lib.EINVAL
    assert call(problem(cells=(2, 5, 3))) == _lib.EINVAL
    # nothing to do: no launch, no workspace needed
    assert call(problem(num_points=0)) == _lib.OK
    assert call(problem(num_columns=0)) == _lib.OK


def test_pair_kernel_resource_usage():
    """every instantiation <CC, FIELD, BOX = true> of the Ewald pair kernel: no scratch and no spills (the library's own
    flags; VGPRs are recorded in DESIGN.md section 7h, not gated)"""
    import re
    from resource_usage import resource_usage
    usage = resource_usage("ewald_near.hip")
    by = {}
    for name, u in usage.items():
        m = re.search(r"ewald_near_kernelILi(\d)ELb(\d)ELb1EE", name)
        if m:
            by[(int(m.group(1)), int(m.group(2)))] = u
    assert set(by) == {(cc, f) for cc in (1, 2, 4) for f in (0, 1)}
    for key, u in sorted(by.items()):
        print(key, "VGPRs %d occupancy %d LDS %d" % (u["VGPRs"], u["Occupancy"], u["LDS Size"]))
        assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (key, u)
