"""CPU tests of the bonded-pair exclusions (torch_nfft_amd/exclusions.py): the float64 restatement
tests/exclusions_ref.py against itself (two splittings, continuity at r = 0, finite differences in the positions and in the
strain, the traces), ExclusionList, the exports, schemas and refusals of the Python layer, the C ABI and the registers of the
kernels."""
import ctypes
import math
import re

import numpy as np
import pytest
import torch

import dispersion_ref as dr
import ewald_virial_ref as ev
import exclusions_ref as xr
from conftest import rel_l2
from ewald_box_ref import T

BOXES = {"cube": None, "T": T}
R_MIN = 0.05  # the closest listed pair of `few` that is not coincident


def _few(box, coincident=True, kind=xr.COULOMB):
    """12 fractional points, neutral charges (Coulomb) or positive coefficients, and a list: a chain 0-1-2-3 bonded at 0.05 ..
    0.08 (in the box's metric) at scale 0 with its 1-3 pairs at Coulomb / dispersion scale 0.5 / 0.25, a pair across the face
    x = 1/2 at 1 / 1.2 and 0.5, and, with `coincident`, a fully excluded pair at r = 0"""
    rng = np.random.default_rng(7)
    A = BOXES[box]
    inv = np.linalg.inv(np.eye(3) if A is None else A)
    s = rng.random((12, 3)) - 0.5
    for k, length in ((1, R_MIN), (2, 0.07), (3, 0.08)):
        e = rng.standard_normal(3)
        s[k] = s[k - 1] + (length * e / np.linalg.norm(e)) @ inv
    s[4] = (0.49, 0.1, -0.2)
    s[5] = (-0.48, 0.12, -0.17)
    pairs = [(0, 1), (2, 1), (2, 3), (0, 2), (3, 1), (4, 5)]
    sc = [0.0, 0.0, 0.0, 0.5, 0.5, 1.0 / 1.2]
    sd = [0.0, 0.0, 0.0, 0.25, 0.25, 0.5]
    if coincident:
        s[7] = s[6]
        pairs.append((7, 6))
        sc.append(0.0)
        sd.append(0.0)
    if kind == xr.COULOMB:
        x = rng.standard_normal(12)
        x -= x.mean()
    else:
        x = rng.random(12) + 0.5
    w = 1.0 - np.array(sc if kind == xr.COULOMB else sd)
    return s, x, np.array(pairs), w


@pytest.mark.parametrize("box", ["cube", "T"])
def test_coulomb_does_not_depend_on_alpha(box):
    """the corrected phi and E at alpha = 6 and 7 (tests/test_ewald_box_ref.py: 1e-11 for these two and |k| <= 14).  The r = 0
    pair is fully excluded: what a scale s > 0 leaves of it, s 2 alpha / sqrt(pi), is no physical quantity"""
    s, q, pairs, w = _few(box)
    a, b = (xr.coulomb_converged(q, s, BOXES[box], None, pairs, w, alpha=alpha) for alpha in (6.0, 7.0))
    for what, x, y in zip(("phi", "E"), a, b):
        print("corrected Coulomb %s in %s at alpha 6 and 7: rel_l2 %.3e" % (what, box, rel_l2(x, y)))
        assert rel_l2(x, y) <= 1e-11
    # ... and the correction matters: the r = 0 constant alone moves phi by far more
    without = xr.coulomb_converged(q, s, BOXES[box], None, pairs[:-1], w[:-1], alpha=6.0)[0]
    assert abs(without[6] - a[0][6]) >= 1e-2 * abs(a[0][6])


@pytest.mark.parametrize("box", ["cube", "T"])
def test_dispersion_does_not_depend_on_alpha(box):
    """the corrected psi and G at alpha = 3.2 and 4, N = 30, every image within two cells (tests/test_dispersion_ref.py: 1e-9)"""
    s, c, pairs, w = _few(box, kind=xr.DISPERSION)
    a, b = (xr.dispersion_converged(c, s, BOXES[box], None, pairs, w, alpha=alpha) for alpha in (3.2, 4.0))
    for what, x, y in zip(("psi", "G"), a, b):
        print("corrected dispersion %s in %s at alpha 3.2 and 4: rel_l2 %.3e" % (what, box, rel_l2(x, y)))
        assert rel_l2(x, y) <= 1e-9
    without = xr.dispersion_converged(c, s, BOXES[box], None, pairs[:-1], w[:-1], alpha=3.2)[0]
    assert abs(without[6] - a[0][6]) >= 1e-2 * abs(a[0][6])  # (at the pair itself)


def test_virials_do_not_depend_on_alpha_and_keep_their_traces():
    """U and W of both corrected sums in T at two splittings, to the figures of tests/test_ewald_virial_ref.py (4 x 7e-10
    absolute, alpha 5 and 6) and tests/test_dispersion_virial_ref.py (1e-9 relative, alpha 3.2 and 4); tr W = U (to 4e-9, as
    there) and tr W = 6 U (1e-13 there; here plus the rounding of the listed terms, which are subtracted from sums that hold
    them)"""
    s, q, pairs, w = _few("T")
    U5, W5 = xr.coulomb_virial_converged(q, s, T, None, pairs, w, alpha=5.0)
    U6, W6 = xr.coulomb_virial_converged(q, s, T, None, pairs, w)
    print("Coulomb, alpha 5 vs 6: W %.1e U %.1e; tr W - U = %.1e" % (np.abs(W5 - W6).max(), np.abs(U5 - U6).max(), np.trace(W6[0]) - U6[0]))
    assert np.abs(W5 - W6).max() <= 4 * 7e-10 and np.abs(U5 - U6).max() <= 4 * 7e-10
    # The smooth part of a coincident pair, q_i q_j 2 alpha / sqrt(pi), is a constant that no strain moves: it is in U and not
    # in W, so that pair breaks tr W = U of the sum over every pair, and excluding it fully (as here) mends it.
    assert abs(np.trace(W6[0]) - U6[0]) <= 4 * 1e-9 and np.abs(W6 - W6.transpose(0, 2, 1)).max() <= 1e-12
    Ua, Wa = ev.converged_virial(q, s, T)
    assert abs(np.trace(Wa[0]) - Ua[0] + xr.zero_constant(xr.COULOMB, 6.0) * q[6] * q[7]) <= 4 * 1e-9
    s, c, pairs, w = _few("T", kind=xr.DISPERSION)
    U0, W0 = xr.dispersion_virial_converged(c, s, T, None, pairs, w)
    U1, W1 = xr.dispersion_virial_converged(c, s, T, None, pairs, w, alpha=4.0)
    print("dispersion, alpha 3.2 vs 4: W %.1e U %.1e" % (rel_l2(W1, W0), rel_l2(U1, U0)))
    assert rel_l2(W1, W0) <= 1e-9 and rel_l2(U1, U0) <= 1e-9
    U, W = U0, W0
    listed = xr.listed_virial(xr.DISPERSION, c, s, T, None, pairs, w, 3.2)[0]
    e_tr = abs(np.trace(W[0]) / U[0] - 6.0)
    print("dispersion: tr W / U - 6 = %.1e (U %.3e, listed %.3e)" % (e_tr, U[0], listed[0]))
    assert e_tr <= 1e-13 + 1e-14 * abs(listed[0] / U[0])


def test_listed_pair_is_continuous_at_zero_separation():
    """A fully excluded pair at r and at r = 0.  Coulomb, r = 1e-7: the corrected phi of every point moves by O(r) -- at most
    r |E|_max for a point that sees the pair move, plus the rounding 2^-52 / r of the two singular terms that cancel.
    Dispersion: the same two terms are 1 / r^6 = 1e42 at r = 1e-7 and cancel to nothing that float64 holds, so the pair is put
    at r = 2e-2 and 1e-2 and psi is compared at the end that stays where it is: it moves by the next term of the smooth part,
    alpha^8 r^2 / 8 per unit coefficient (twice that is allowed), plus the rounding 2^-52 / r^6 (2e-4 at 1e-2; 0.2 at 1e-3,
    which is why the pair is not put closer)."""
    s, q, pairs, w = _few("cube")
    e = np.array([0.6, -0.64, 0.48])

    def at(r, kind, x, alpha):
        y = s.copy()
        y[7] = y[6] + r * e
        fn = xr.coulomb_converged if kind == xr.COULOMB else xr.dispersion_converged
        return fn(x, y, None, None, pairs, w, alpha=alpha)

    phi0, E0 = at(0.0, xr.COULOMB, q, 6.0)
    r = 1e-7
    phi1, _ = at(r, xr.COULOMB, q, 6.0)
    bound = r * np.abs(E0).max() * 2 + 2.0 ** -52 / r * np.abs(q).max() * 4
    print("Coulomb pair at r = 1e-7 and 0: |dphi|_max %.3e, bound %.3e" % (np.abs(phi1 - phi0).max(), bound))
    assert np.abs(phi1 - phi0).max() <= bound
    assert xr.zero_constant(xr.COULOMB, 6.0) * abs(q[6]) > 1e4 * bound  # (the constant is not hidden under it)
    c = np.abs(q) + 0.5
    alpha = 3.2
    psi0, G0 = at(0.0, xr.DISPERSION, c, alpha)
    for r in (2e-2, 1e-2):
        psi1, _ = at(r, xr.DISPERSION, c, alpha)
        bound = 2 * alpha ** 8 * r * r / 8 * c[7] + 2.0 ** -52 / r ** 6 * c.max() * 4
        print("dispersion pair at r = %g and 0: |dpsi| %.3e, bound %.3e" % (r, abs(psi1[6] - psi0[6]), bound))
        assert abs(psi1[6] - psi0[6]) <= bound
    assert xr.zero_constant(xr.DISPERSION, alpha) * c[7] > 50 * bound


@pytest.mark.parametrize("kind", [xr.COULOMB, xr.DISPERSION])
def test_fields_are_the_gradient_of_the_corrected_energy(kind):
    """-dU/dx_i = x_i E_i (x_i G_i) of the corrected energy U = 1/2 sum x_i phi_i in T, by central differences (h = 1e-5) at a
    chain end, a chain middle, a point across the face and the coincident pair's end.  A central difference of 1 / r^p is off
    by (h^2 / 6) (p + 1) (p + 2) / r^2 of the derivative -- 9.4 (h / r)^2 for p = 6 -- and r_min is the closest pair of the
    set, listed or not: 10 (h / r_min)^2 of the largest force.  (The coincident pair's end is moved for the Coulomb sum only:
    at r = h = 1e-5 the dispersion sum's two singular terms are 1e30 and cancel to nothing that float64 holds.)"""
    s, x, pairs, w = _few("T", kind=kind)
    inv = np.linalg.inv(T)
    if kind == xr.COULOMB:
        fn = lambda y: xr.coulomb_converged(x, y, T, None, pairs, w, kmax=10)  # noqa: E731
    else:
        fn = lambda y: xr.dispersion_converged(x, y, T, None, pairs, w, N=20, nimg=1)  # noqa: E731
    _, E = fn(s)
    r_min = dr.min_separation(s, T)
    assert 0.01 < r_min <= R_MIN * (1 + 1e-12)
    h = 1e-5
    force = x[:, None] * E
    for i in (0, 2, 5, 6) if kind == xr.COULOMB else (0, 2, 5):
        for b in range(3):
            step = np.zeros(3)
            step[b] = h
            up, um = s.copy(), s.copy()
            up[i] += step @ inv
            um[i] -= step @ inv
            fd = -(xr.energy(x, fn(up)[0])[0] - xr.energy(x, fn(um)[0])[0]) / (2 * h)
            err = abs(fd - force[i, b]) / np.abs(force).max()
            print("kind %d: force[%d, %d] %.6e, differences %.6e (%.1e of the largest)" % (kind, i, b, force[i, b], fd, err))
            assert err <= 10 * (h / r_min) ** 2


@pytest.mark.parametrize("kind", [xr.COULOMB, xr.DISPERSION])
def test_virial_is_the_strain_derivative_of_the_corrected_energy(kind):
    """W_ab = -dU / d eps_ab for A -> A (1 + eps) at fixed fractional coordinates, by central differences (H = 1e-5), to
    10 (H / r_min)^2 ... no: the strain scales every separation, d -> d (1 + eps), so a pair's term r^-p is differentiated in
    ln r and the difference is off by (H^2 / 6) p^2 of it, 6 H^2 for p = 6, whatever r is: 10 H^2 of |W|_max, plus the rounding
    2^-52 |U| / H of the difference of two energies"""
    s, x, pairs, w = _few("T", kind=kind)
    if kind == xr.COULOMB:
        conv = lambda A: xr.coulomb_virial_converged(x, s, A, None, pairs, w, kmax=10)  # noqa: E731
    else:
        conv = lambda A: xr.dispersion_virial_converged(x, s, A, None, pairs, w, N=20, nimg=1)  # noqa: E731
    U, W = conv(T)
    H = 1e-5
    fd = np.zeros((3, 3))
    for a in range(3):
        for b in range(3):
            eps = np.zeros((3, 3))
            eps[a, b] = H
            fd[a, b] = -(conv(T @ (np.eye(3) + eps))[0][0] - conv(T @ (np.eye(3) - eps))[0][0]) / (2 * H)
    err = np.abs(W[0] - fd).max() / np.abs(W).max()
    print("kind %d: |W + dU/d eps|_max / |W|_max = %.2e" % (kind, err))
    floor = 2.0 ** -52 * abs(U[0]) / H / np.abs(W).max()
    assert err <= 10 * H * H + 10 * floor
    # U is the energy of the corrected potential
    phi = (xr.coulomb_converged(x, s, T, None, pairs, w, kmax=10) if kind == xr.COULOMB
           else xr.dispersion_converged(x, s, T, None, pairs, w, N=20, nimg=1))[0]
    assert abs(U[0] - xr.energy(x, phi)[0]) <= 1e-10 * max(abs(U[0]), np.abs(x * phi).max())


# ---- the product ---------------------------------------------------------------------------------------------------------

def test_exclusion_list_csr():
    import torch_nfft_amd as tn
    n = 30
    hub = [(5, k) for k in range(8, 28)]  # a row of length 20
    pairs = [(3, 1), (0, 3)] + hub + [(29, 28)]
    sc = np.linspace(0.0, 1.0, len(pairs))
    sd = np.linspace(1.0, 0.0, len(pairs))
    ex = tn.ExclusionList(torch.tensor(pairs), n, coulomb_scale=torch.from_numpy(sc), dispersion_scale=sd.tolist(), device="cpu")
    assert ex.num_points == n and ex.num_pairs == len(pairs) == len(ex)
    assert ex.row_start.dtype == torch.int32 and ex.col.dtype == torch.int32
    assert ex.coulomb_weight.dtype == ex.dispersion_weight.dtype == torch.float32
    assert ex.row_start.shape == (n + 1,) and ex.col.shape == ex.coulomb_weight.shape == ex.dispersion_weight.shape == (2 * len(pairs),)
    rs, col, wc = xr.csr(pairs, n, 1.0 - sc)
    _, _, wd = xr.csr(pairs, n, 1.0 - sd)
    assert np.array_equal(ex.row_start.numpy(), rs) and np.array_equal(ex.col.numpy(), col)
    assert np.array_equal(ex.coulomb_weight.numpy(), wc.astype(np.float32))
    assert np.array_equal(ex.dispersion_weight.numpy(), wd.astype(np.float32))
    length = np.diff(ex.row_start.numpy())
    assert length[2] == 0 and length[0] == 1 and length[5] == 20 and length[3] == 2 and length.sum() == 2 * len(pairs)
    dense = np.zeros((n, n))
    for i in range(n):
        row = ex.col.numpy()[rs[i]:rs[i + 1]]
        assert (np.diff(row) > 0).all()  # sorted, no duplicates
        dense[i, row] = ex.coulomb_weight.numpy()[rs[i]:rs[i + 1]]
    assert np.array_equal(dense, dense.T) and not np.diag(dense).any()
    assert dense[1, 3] == np.float32(1.0) and dense[28, 29] == 0.0  # scale 0 -> weight 1, scale 1 -> weight 0
    # scalars, the defaults, m = 0
    ex = tn.ExclusionList(pairs, n, coulomb_scale=1 / 1.2, device="cpu")
    assert np.all(ex.coulomb_weight.numpy() == np.float32(1.0 - 1 / 1.2)) and np.all(ex.dispersion_weight.numpy() == 1.0)
    for empty in ([], torch.zeros(0, 2, dtype=torch.int64), np.zeros((0, 2), dtype=np.int32)):
        ex = tn.ExclusionList(empty, 4, device="cpu")
        assert ex.num_pairs == 0 and ex.col.numel() == 0 and ex.row_start.tolist() == [0] * 5
    assert tn.ExclusionList([], 0, device="cpu").row_start.tolist() == [0]
    assert ex.to("cpu") is ex


def test_exclusion_list_refusals():
    import torch_nfft_amd as tn
    ok = [(0, 1), (2, 1)]
    for bad, what in (([(0, 0)], "i == j"), ([(0, 4)], "outside"), ([(-1, 2)], "outside"), (ok + [(1, 0)], "twice"),
                      (ok + [(2, 1)], "twice")):
        with pytest.raises(ValueError, match=what):
            tn.ExclusionList(bad, 4, device="cpu")
    for scale in (-0.1, 1.5, float("nan"), float("inf"), [0.0, 2.0]):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            tn.ExclusionList(ok, 4, coulomb_scale=scale, device="cpu")
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            tn.ExclusionList(ok, 4, dispersion_scale=scale, device="cpu")
    with pytest.raises(ValueError, match="one entry per pair"):
        tn.ExclusionList(ok, 4, coulomb_scale=[0.0, 0.5, 1.0], device="cpu")
    with pytest.raises(ValueError, match="different point sets"):
        tn.ExclusionList(ok, 4, batch=torch.tensor([0, 0, 1, 1]), device="cpu")
    tn.ExclusionList(ok, 4, batch=torch.tensor([0, 0, 0, 1]), device="cpu")
    with pytest.raises(ValueError, match="integer"):
        tn.ExclusionList(torch.zeros(2, 2), 4, device="cpu")
    with pytest.raises(ValueError, match="integer"):
        tn.ExclusionList(torch.zeros(2, 3, dtype=torch.int64), 4, device="cpu")


def test_exports_schemas_and_refusals():
    import torch_nfft
    import torch_nfft_amd as tn
    from torch_nfft_amd import _lib
    assert _lib.ABI_VERSION == 7
    assert "ExclusionList" in tn.__all__ and "ExclusionList" in torch_nfft.__all__ and torch_nfft.ExclusionList is tn.ExclusionList
    assert torch_nfft.exclusions is tn.exclusions
    s = str(torch.ops.torch_nfft._nfft_ewald_excl.default._schema)
    assert s == ("torch_nfft::_nfft_ewald_excl(Tensor pos, Tensor x, Tensor? batch, Tensor row_start, Tensor col, Tensor weight, "
                 "float[] box, float alpha, int kind, bool with_field) -> (Tensor, Tensor)")
    s = str(torch.ops.torch_nfft._nfft_ewald_excl_virial.default._schema)
    assert s == ("torch_nfft::_nfft_ewald_excl_virial(Tensor pos, Tensor x, Tensor? batch, Tensor row_start, Tensor col, "
                 "Tensor weight, float[] box, float alpha, int kind) -> Tensor")
    q, pos = torch.zeros(5), torch.zeros(5, 3)
    ex = tn.ExclusionList([(0, 1), (3, 4)], 5, device="cpu")
    box6 = (1.0, 0.0, 1.3, 0.0, 0.0, 0.8)
    for box in ((), box6):
        with pytest.raises(RuntimeError, match="torch_nfft._nfft_ewald_excl is currently only implemented for GPU tensors"):
            tn.ops.nfft_ewald_excl(pos, q, None, ex.row_start, ex.col, ex.coulomb_weight, box, 6.0, 0, True)
    with pytest.raises(RuntimeError, match="torch_nfft._nfft_ewald_excl_virial is currently only implemented for GPU tensors"):
        tn.ops.nfft_ewald_excl_virial(pos, q, None, ex.row_start, ex.col, ex.dispersion_weight, box6, 6.0, 1)
    es = tn.EwaldSplitting(6.0, 0.3, 16, device="cpu")
    ds = tn.DispersionSplitting(6.0, 0.3, 16, device="cpu")
    for fn, sp in ((tn.nfft_ewald, es), (tn.nfft_ewald_energy, es), (tn.nfft_ewald_virial, es), (tn.nfft_ewald_dispersion, ds),
                   (tn.nfft_ewald_dispersion_energy, ds), (tn.nfft_ewald_dispersion_virial, ds)):
        for bad in ([(0, 1)], torch.tensor([[0, 1]]), "none", 0):
            with pytest.raises(TypeError, match="ExclusionList"):
                fn(q, pos, splitting=sp, exclusions=bad)
        with pytest.raises(ValueError, match="pairs of 4 points, pos has 5"):
            fn(q, pos, splitting=sp, exclusions=tn.ExclusionList([(0, 1)], 4, device="cpu"))
        with pytest.raises(RuntimeError, match="is currently only implemented for GPU tensors"):
            fn(q, pos, splitting=sp, exclusions=ex)


def test_c_abi_validation_without_gpu():
    """the four symbols; they refuse null pointers, negative counts, a kind other than 0 or 1, an alpha that is not finite and
    positive and (where the box is read) a box without a positive diagonal, all before any device access, and the virial
    takes the workspace that its size function reports"""
    from torch_nfft_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 7 and lib.nfft_hip_abi_version() == 7
    for name in ("nfft_hip_ewald_excl", "nfft_hip_ewald_excl_box", "nfft_hip_ewald_excl_virial_workspace_bytes", "nfft_hip_ewald_excl_virial"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(256)  # (never dereferenced: the checks come first)

    def problem(**kw):
        f = dict(kind=0, with_field=1, num_points=1000, num_columns=2, num_entries=4000, batch_size=1, alpha=6.0,
                 box=(ctypes.c_double * 6)(1.0, 0.0, 1.3, 0.0, 0.0, 0.8))
        f.update(kw)
        return _lib.EwaldExclProblem(**f)

    def call(fn, q, points=one, xr_=one, rs=one, col=one, w=one, z=one, field=one):
        return fn(ctypes.byref(q), points, xr_, rs, col, w, z, field, null)

    bad_box = (ctypes.c_double * 6)(1.0, 0.0, -1.3, 0.0, 0.0, 0.8)
    nan_box = (ctypes.c_double * 6)(1.0, float("nan"), 1.3, 0.0, 0.0, 0.8)
    common = (problem(kind=2), problem(kind=-1), problem(with_field=2), problem(num_points=-1), problem(num_columns=-1),
              problem(num_entries=-1), problem(batch_size=0), problem(alpha=0.0), problem(alpha=-1.0), problem(alpha=float("nan")),
              problem(alpha=float("inf")), problem(num_points=2 ** 31), problem(num_entries=2 ** 31))
    for fn in (lib.nfft_hip_ewald_excl, lib.nfft_hip_ewald_excl_box):
        for bad in common:
            assert call(fn, bad) == _lib.EINVAL and _lib.last_error().startswith("Input mismatch"), _lib.last_error()
        for kw in (dict(points=null), dict(xr_=null), dict(rs=null), dict(col=null), dict(w=null), dict(z=null), dict(field=null)):
            assert call(fn, problem(), **kw) == _lib.EINVAL and _lib.last_error().startswith("Input mismatch")
        assert fn(None, one, one, one, one, one, one, one, null) == _lib.EINVAL
        assert call(fn, problem(num_points=0)) == _lib.OK and call(fn, problem(num_columns=0)) == _lib.OK
        assert call(fn, problem(num_points=0, kind=3)) == _lib.EINVAL  # (before the early return too)
    for what, bad in (("kind", problem(kind=2)), ("alpha", problem(alpha=0.0)), ("negative", problem(num_entries=-1))):
        assert call(lib.nfft_hip_ewald_excl, bad) == _lib.EINVAL and what in _lib.last_error()
    for box in (bad_box, nan_box):
        assert call(lib.nfft_hip_ewald_excl_box, problem(box=box)) == _lib.EINVAL and "box" in _lib.last_error()
        assert call(lib.nfft_hip_ewald_excl_box, problem(box=box, num_points=0)) == _lib.EINVAL
        assert lib.nfft_hip_ewald_excl_virial_workspace_bytes(ctypes.byref(problem(box=box))) == -1
    assert call(lib.nfft_hip_ewald_excl, problem(box=bad_box, num_points=0)) == _lib.OK  # (the torus does not read the box)

    def virial(q, ws=null, nbytes=0, out=one, set_start=one, points=one):
        return lib.nfft_hip_ewald_excl_virial(ctypes.byref(q), points, one, one, one, one, set_start, out, ws, nbytes, null)

    ok = problem(batch_size=3)
    need = lib.nfft_hip_ewald_excl_virial_workspace_bytes(ctypes.byref(ok))
    assert need > 0 and lib.nfft_hip_ewald_excl_virial_workspace_bytes(None) == -1
    assert virial(ok) == _lib.EWORKSPACE and _lib.last_error() == "workspace too small"
    assert virial(ok, ws=one, nbytes=need - 1) == _lib.EWORKSPACE
    assert virial(ok, out=null) == _lib.EINVAL and virial(ok, points=null) == _lib.EINVAL
    assert virial(ok, set_start=null) == _lib.EINVAL  # (three point sets need their starts)
    assert virial(problem(), set_start=null) == _lib.EWORKSPACE  # (one does not)
    for bad in common + (problem(num_columns=2 ** 21), problem(batch_size=2 ** 20, num_columns=2)):
        assert virial(bad) == _lib.EINVAL and _lib.last_error().startswith("Input mismatch")
        assert lib.nfft_hip_ewald_excl_virial_workspace_bytes(ctypes.byref(bad)) == -1
    assert virial(problem(num_columns=0)) == _lib.OK


def test_kernel_resource_usage():
    """exactly the 24 instantiations <CC, KIND, FIELD, BOX> of the list kernel and the 6 <CC, KIND> of the virial kernel and
    nothing else in that file, each without scratch and without spills (the library's own flags); the list kernel uses no
    LDS (VGPRs and occupancy are recorded in DESIGN.md section 7o, not gated)"""
    from resource_usage import resource_usage
    usage = resource_usage("ewald_excl.hip")
    lists, virials = {}, {}
    for name, u in usage.items():
        m = re.search(r"ewald_excl_kernelILi(\d)ELi(\d)ELb(\d)ELb(\d)EE", name)
        v = re.search(r"ewald_excl_virial_kernelILi(\d)ELi(\d)EE", name)
        assert m or v, name  # (nothing else in that file)
        (lists if m else virials)[tuple(int(g) for g in (m or v).groups())] = u
        assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
    assert set(lists) == {(cc, k, f, b) for cc in (1, 2, 4) for k in (0, 1) for f in (0, 1) for b in (0, 1)}
    assert set(virials) == {(cc, k) for cc in (1, 2, 4) for k in (0, 1)}
    assert len(usage) == 30
    for key, u in sorted(lists.items()):
        print("list", key, "VGPRs %d SGPRs %d occupancy %d LDS %d" % (u["VGPRs"], u["TotalSGPRs"], u["Occupancy"], u["LDS Size"]))
        assert u["LDS Size"] == 0
    for key, u in sorted(virials.items()):
        print("virial", key, "VGPRs %d SGPRs %d occupancy %d LDS %d" % (u["VGPRs"], u["TotalSGPRs"], u["Occupancy"], u["LDS Size"]))
        assert u["LDS Size"] == 4 * 7 * key[0] * 8
