"""CPU tests of the screened Coulomb (Yukawa) Ewald sum (nfft_ewald_yukawa): the float64 restatement
tests/yukawa_ref.py against the brute-force lattice sum (which converges on its own for lambda > 0 and owes nothing to Ewald),
against central differences of the lattice energy, against the Coulomb restatement as lambda -> 0 and against the mistakes a
pair weight can make; the host-side pieces of torch_nfft_amd/yukawa.py against the restatement, the refusals, the C ABI and
the registers of the two pair kernels."""
import ctypes
import math
import re

import numpy as np
import pytest
import torch

import dispersion_ref as dr
import ewald_ref as er
import yukawa_ref as yr
from conftest import rel_l2
from ewald_box_ref import O, T, widths

BOXES = {"cube": None, "T": T, "O": O}

# alpha r_c = 4.5: erfc(4.5) = 2e-10; the plane k_a = 28 of T's longest lattice vector lies at e^(-pi^2 |kappa|^2 / alpha^2) = 6e-12
SPLIT = (15.0, 0.3, 56)


@pytest.mark.parametrize("box,lam,radius", [("cube", 6.0, 6), ("T", 8.0, 5)])
def test_split_against_lattice_sum(box, lam, radius):
    """The restatement (pairs within r_c, |k_a| < 28, self term) against the sum over the images |n|_inf <= radius, whose own
    truncation is e^(-lam w radius) <= e^-36 = 2e-16.  What is left is the split's truncation of the pair sum at r_c, of the
    size of erfc(alpha r_c) = 2.0e-10.  Seen: 5.1e-11 (potential) and 3.4e-10 (field) in the cube, 6.6e-12 and 5.4e-11 in T.
    The bound is erfc(alpha r_c) itself for the potential and four times that for the field: the field's weight at the cut,
    mg r ~ 2 alpha^2 r_c w, is larger than the potential's by more than the field itself is larger than the potential, so its
    share of the truncation is a small multiple of the potential's."""
    A = BOXES[box]
    w = 1.0 if A is None else widths(A).min()
    assert lam * w * radius >= 35.0
    alpha, r_c, N = SPLIT
    assert alpha * r_c >= 4.5 and r_c <= w / 3 + 1e-12
    rng = np.random.default_rng(5)
    n = 30
    s = rng.random((n, 3)) - 0.5
    q = rng.standard_normal(n)
    want, ewant = yr.lattice_sum(q, s, A, lam, radius)
    got, egot = yr.yukawa(q, s, A, None, alpha, lam, r_c, N)
    e, ee = rel_l2(got, want), rel_l2(egot, ewant)
    bound = math.erfc(alpha * r_c)
    print("yukawa split in %s (lambda %g): potential rel_l2 %.3e, field rel_l2 %.3e (erfc(alpha r_c) = %.3e)" % (box, lam, e, ee, bound))
    assert e <= bound and ee <= 4 * bound
    # with the background: the same sum less the mean potential
    gotb, egotb = yr.yukawa(q, s, A, None, alpha, lam, r_c, N, background=True)
    wantb, _ = yr.lattice_sum(q, s, A, lam, radius, background=True)
    assert rel_l2(gotb, wantb) <= bound and rel_l2(egotb, egot) <= 1e-13  # (k = 0 carries no field)


@pytest.mark.parametrize("background", [False, True])
def test_forces_and_virial_are_derivatives_of_the_lattice_energy(background):
    """q_i E_i = -dU/dx_i and W_ab = -dU/d eps_ab (A -> A (1 + eps) at fixed s and lambda) of the restatement against central
    differences (h = 1e-5) of the brute-force lattice energy, in T: the differences are good to h^2 and to 1e-16 U / h ~ 1e-10
    (seen: 1.7e-10 of max |W| without and 1.6e-10 with the background)."""
    lam, radius = 8.0, 5
    alpha, r_c, N = SPLIT
    rng = np.random.default_rng(11)
    n = 12
    s = rng.random((n, 3)) - 0.5
    q = rng.standard_normal(n) + 0.3  # (not neutral: the background term is there)
    _, E = yr.yukawa(q, s, T, None, alpha, lam, r_c, N, background=background)
    U, W = yr.virial(q, s, T, None, alpha, lam, r_c, N, background=background)
    U0 = yr.lattice_energy(q, s, T, lam, radius, background=background)
    assert abs(U[0] - U0) <= 1e-9 * abs(U0)
    h = 1e-5
    inv = np.linalg.inv(T)
    scale = np.abs(q[:, None] * E).max()
    for i, a in ((0, 0), (5, 1), (11, 2)):
        e = np.zeros(3)
        e[a] = h
        sp, sm = s.copy(), s.copy()
        sp[i] += e @ inv
        sm[i] -= e @ inv
        up, um = (yr.lattice_energy(q, x, T, lam, radius, background=background) for x in (sp, sm))
        assert abs(-(up - um) / (2 * h) - q[i] * E[i, a]) <= 1e-6 * scale
    num = np.zeros((3, 3))
    for a in range(3):
        for b in range(3):
            eps = np.zeros((3, 3))
            eps[a, b] = h
            up, um = (yr.lattice_energy(q, s, T @ (np.eye(3) + sg * eps), lam, radius, background=background) for sg in (1, -1))
            num[a, b] = -(up - um) / (2 * h)
    err = np.abs(W[0] - num).max() / np.abs(num).max()
    print("yukawa virial, background=%d: U %.6f, tr W %.6f, max |W - dU/d eps| / max |W| %.3e" % (background, U[0], np.trace(W[0]), err))
    assert err <= 1e-6
    # W is symmetric: the restatement's to rounding, and so is the derivative of the lattice energy that owes it nothing
    assert np.abs(W[0] - W[0].T).max() <= 1e-13 * np.abs(W[0]).max()
    assert np.abs(num - num.T).max() <= 1e-6 * np.abs(num).max()
    assert abs(np.trace(W[0]) - U[0]) > 1e-3 * abs(U[0])  # (lambda carries a length: tr W is not U)


def test_coulomb_limit():
    """With the background, phi - lambda q tends to the Coulomb restatement's phi like lambda^2 (the same alpha, r_c, N on both
    sides): the remainders seen are 1.35e-3, 1.50e-4 and 1.35e-5 of |phi|, ratios 9.0 and 11.1 as the squares of 3 and 10/3"""
    alpha, r_c, N = 12.0, 0.3, 32
    rng = np.random.default_rng(2)
    x = rng.random((20, 3)) - 0.5
    q = rng.standard_normal(20) + 0.2
    coul = er.exact_algorithm(q, x, None, alpha, r_c, N)
    lams = (0.3, 0.1, 0.03)
    rem = [rel_l2(yr.yukawa(q, x, None, None, alpha, lam, r_c, N, background=True)[0] - lam * q, coul) for lam in lams]
    print("phi^Y - lambda q against the Coulomb sum at lambda = 0.3, 0.1, 0.03: rel_l2 %.3e %.3e %.3e" % tuple(rem))
    for k in (0, 1):
        ratio, want = rem[k] / rem[k + 1], (lams[k] / lams[k + 1]) ** 2
        assert want / 2 <= ratio <= want * 2
    # without the lambda q the limit is missed at first order
    assert rel_l2(yr.yukawa(q, x, None, None, alpha, 0.03, r_c, N, background=True)[0], coul) > 10 * rem[2]


def test_near_sum_is_sensitive_to_mistakes():
    """On the 8^3 jittered lattice at lambda = 10, (alpha, r_c) = (6, 0.25), every mistake of the pair weight or of the sweep
    moves the near value or the near field by 1e-2 at least, far above a device run's tolerance.  Seen: beta's sign 1.8e1 /
    1.7e0 (value / field), e^(lambda r) term dropped 2.3e-1 / 2.1e-2, e^(-beta^2) missing in g 0 / 3.2e-1, the Coulomb
    weights 4.8e-1 / 2.3e-1, no wrap 2.6e-1 / 9.1e-1, a cut at 0.95 r_c 2.2e-2 / 5.7e-2."""
    alpha, r_c, lam = 6.0, 0.25, 10.0
    x = dr.jittered_lattice(np.random.default_rng(0), 8, 1.0 / 8, 0.03).reshape(-1, 3)
    q = (np.random.default_rng(1).random(512) + 0.5).astype(np.float32)
    z, f = yr.near_sum(q, x, None, None, alpha, lam, r_c), yr.near_field(q, x, None, None, alpha, lam, r_c)
    assert np.linalg.norm(z) > 0 and np.linalg.norm(f) > 0
    cases = [(m, dict(mutant=m), r_c) for m in yr.MUTANTS] + [("no wrap", dict(wrap=False), r_c), ("0.95 r_c", {}, 0.95 * r_c)]
    for what, kw, rc in cases:
        ez = rel_l2(yr.near_sum(q, x, None, None, alpha, lam, rc, **kw), z)
        ef = rel_l2(yr.near_field(q, x, None, None, alpha, lam, rc, **kw), f)
        print("lambda %g (%g, %g) %s: value moves by %.3e, field by %.3e" % (lam, alpha, r_c, what, ez, ef))
        assert max(ez, ef) >= 1e-2


def _virial_before_the_factoring(q, s, A, batch, alpha, lam, r_c, N, background):
    """yukawa_ref.virial as it stood before near_virial was factored out of it: the pair part inline, W by one einsum"""
    qc = dr._columns(np.asarray(q))
    s = np.asarray(s, dtype=np.float64)
    Am = dr._box(A)
    V = abs(np.linalg.det(Am))
    b, t = yr.coeffs(A, alpha, lam, N, background).reshape(-1), yr.strain_coeffs(A, alpha, lam, N, background).reshape(-1)
    K, kap = dr.kappa(A, N)
    K, kap, t, b = K.reshape(-1, 3)[b != 0], kap.reshape(-1, 3)[b != 0], t[b != 0], b[b != 0]
    sets = dr._sets(batch, s.shape[0])
    U, W = np.zeros((len(sets), qc.shape[1])), np.zeros((len(sets), 3, 3, qc.shape[1]))
    for n, sel in enumerate(sets):
        if sel.size == 0:
            continue
        qs = qc[sel]
        ds = s[sel][:, None, :] - s[sel][None, :, :]
        d = (ds - np.rint(ds)) @ Am
        w, mg = yr.pair_weights(d, alpha, lam, r_c)
        U[n] = 0.5 * np.einsum("ic,ij,jc->c", qs, w, qs)
        W[n] = 0.5 * np.einsum("ic,ij,ija,ijb,jc->abc", qs, mg, d, d, qs)
        S = np.exp(-2j * math.pi * K @ s[sel].T) @ qs
        p = (S * np.conj(S)).real
        U[n] += 0.5 * (b[:, None] * p).sum(0)
        W[n] += 0.5 * (np.einsum("k,kc->c", b, p)[None, None] * np.eye(3)[:, :, None] + np.einsum("k,ka,kb,kc->abc", t, kap, kap, p))
        U[n] -= 0.5 * yr.self_term(alpha, lam) * (qs * qs).sum(0)
        if background:
            bg = 0.5 * yr.background_term(alpha, lam, V) * qs.sum(0) ** 2
            U[n] += bg
            W[n] += bg[None, None] * np.eye(3)[:, :, None]
    return U, W


@pytest.mark.parametrize("box,background", [("cube", False), ("T", True), ("O", False)])
def test_factored_pair_part_leaves_the_virial_unchanged(box, background):
    """virial() with its pair part taken from near_virial against the function as it stood, to float64 rounding, three point
    sets with an empty one and two columns; and near_virial is that pair part in the order energy, xx, yy, zz, yz, xz, xy"""
    A = BOXES[box]
    rng = np.random.default_rng(17)
    n = 90
    s = rng.random((n, 3)) - 0.5
    q = rng.standard_normal((n, 2)) + 0.2
    batch = np.concatenate([np.zeros(40, np.int64), np.full(50, 2, np.int64)])
    alpha, r_c, N, lam = 6.0, 0.25, 8, 10.0
    U, W = yr.virial(q, s, A, batch, alpha, lam, r_c, N, background=background)
    U0, W0 = _virial_before_the_factoring(q, s, A, batch, alpha, lam, r_c, N, background)
    assert U.shape == (3, 2) and W.shape == (3, 3, 3, 2) and not U[1].any() and not W[1].any()
    eu, ew = np.abs(U - U0).max() / np.abs(U0).max(), np.abs(W - W0).max() / np.abs(W0).max()
    print("yukawa virial in %s, factored against before: U %.3e, W %.3e" % (box, eu, ew))
    assert eu <= 1e-14 and ew <= 1e-14
    seven = yr.near_virial(q, s, A, batch, alpha, lam, r_c)
    assert seven.shape == (3, 7, 2) and not seven[1].any() and seven[0].all() and seven[2].all()
    for sel, b in ((np.arange(40), 0), (np.arange(40, 90), 2)):
        ds = s[sel][:, None, :] - s[sel][None, :, :]
        d = (ds - np.rint(ds)) @ dr._box(A)
        w, mg = yr.pair_weights(d, alpha, lam, r_c)
        want = [0.5 * np.einsum("ic,ij,jc->c", q[sel], w, q[sel])]
        want += [0.5 * np.einsum("ic,ij,jc->c", q[sel], mg * d[..., i] * d[..., j], q[sel]) for i, j in
                 ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))]
        assert np.abs(seven[b] - np.array(want)).max() <= 1e-13 * np.abs(seven[b]).max()
    assert yr.near_virial(q[:, 0], s, A, None, alpha, lam, r_c).shape == (1, 7)


def test_near_virial_is_sensitive_to_the_pair_weight_mutants():
    """on the counted 3^3 layout in T (tests/pair_frame_ref.py) at lambda = 10, (5, 0.3), every mutant of the pair weight
    moves the pair part of the virial by at least ten times the gate that tests/test_gpu_pair_frame_edges.py holds the
    native pair reduction to (seen: beta's sign 1.5e1, the e^(lambda r) term dropped 6.6e-2, e^(-beta^2) missing in g 4.8e-1,
    the Coulomb weights 4.5e-1)"""
    import pair_frame_ref as pf
    from ewald_virial_ref import rel_fro
    from test_gpu_pair_frame_edges import GATES
    gate = GATES[("yukawa_virial_near", "seven")]
    L = pf.layout("grid3")
    q = np.random.default_rng(1).standard_normal(L.n).astype(np.float32)
    ref = yr.near_virial(q, L.points, T, None, 5.0, 10.0, 0.3)
    for m in yr.MUTANTS:
        moved = rel_fro(yr.near_virial(q, L.points, T, None, 5.0, 10.0, 0.3, mutant=m), ref)
        print("near_virial on the counted layout, mutant %s: moves by %.3e (gate %.1e)" % (m, moved, gate))
        assert moved >= 10 * gate


def test_weights_at_zero_screening_are_the_coulomb_weights():
    d = np.random.default_rng(4).random((50, 3)) * 0.2
    for a, b in zip(yr.pair_weights(d, 6.0, 0.0), yr.pair_weights(d, 6.0, 0.0, mutant="coulomb")):
        assert np.abs(a - b).max() <= 1e-15 * np.abs(b).max()
    w, _ = yr.pair_weights(d, 6.0, 10.0)
    assert (w <= yr.pair_weights(d, 6.0, 0.0)[0]).all()  # w <= erfc(alpha r) / r


@pytest.mark.parametrize("box", ["cube", "T", "O"])
@pytest.mark.parametrize("background", [False, True])
def test_splitting_coefficients(box, background):
    import torch_nfft
    import torch_nfft_amd as tn
    A = BOXES[box]
    V = 1.0 if A is None else float(np.linalg.det(A))
    for alpha, lam, N in ((11.5, 3.0, 32), (6.0, 10.0, 16)):
        sp = tn.YukawaSplitting(alpha, 0.25, N, lam, box=None if A is None else torch.from_numpy(A), background=background,
                                device="cpu")
        assert isinstance(sp, torch_nfft.YukawaSplitting)
        assert sp.coeffs.shape == (N, N, N) and sp.coeffs.dtype == torch.float32
        assert sp.volume == pytest.approx(V, rel=1e-14) and sp.bandwidth == N and sp.alpha == alpha and sp.r_cut == 0.25
        assert sp.screening == lam and sp.background is background
        want = yr.coeffs(A, alpha, lam, N, background)
        b = sp.coeffs.numpy()
        assert np.abs(b - want).max() <= 6e-8 * np.abs(want).max()  # (float32 rounding of float64 values)
        h, beta = N // 2, lam / (2 * alpha)
        b0 = 4 * math.pi * math.exp(-beta * beta) / (V * lam * lam)
        if background:
            assert b[h, h, h] == 0.0
            assert sp.background_term == pytest.approx(4 * math.pi / (V * lam * lam) * math.expm1(-beta * beta), rel=1e-14)
        else:
            assert abs(b[h, h, h] - b0) <= 6e-8 * b0 and b[h, h, h] == b.max() and sp.background_term == 0.0
        assert not b[0].any() and not b[:, 0].any() and not b[:, :, 0].any()
        assert (b[1:, 1:, 1:] == b[1:, 1:, 1:][::-1, ::-1, ::-1]).all() and (b >= 0).all()
        assert sp.self_term == pytest.approx(yr.self_term(alpha, lam), rel=1e-14)
        t = sp.strain_coeffs()
        assert t.shape == (N, N, N) and t.dtype == torch.float32
        assert ((t.numpy() == 0) == (b == 0)).all() and (t.numpy() <= 0).all()
        tw = yr.strain_coeffs(A, alpha, lam, N, background)
        tw[b == 0] = 0.0
        assert np.abs(t.numpy() - tw).max() <= 6e-8 * np.abs(tw).max()
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
    A = None if BOXES[box] is None else torch.from_numpy(BOXES[box])
    sp = tn.YukawaSplitting.from_tolerance(tol, 0.25, 5.0, box=A, background=True, device="cpu")
    ew = tn.EwaldSplitting.from_tolerance(tol, 0.25, box=A, device="cpu")
    assert (sp.alpha, sp.bandwidth, sp.r_cut) == (ew.alpha, ew.bandwidth, 0.25) and sp.screening == 5.0 and sp.background
    assert (sp.coeffs <= ew.coeffs)[ew.coeffs > 0].all()  # b^Y <= b^C: the bandwidth is an upper bound
    with pytest.raises(ValueError):
        tn.YukawaSplitting.from_tolerance(1.5, 0.25, 5.0, device="cpu")
    with pytest.raises(ValueError):
        tn.YukawaSplitting.from_tolerance(tol, 0.34, 5.0, device="cpu")
    with pytest.raises(ValueError, match="screening"):
        tn.YukawaSplitting.from_tolerance(tol, 0.25, 0.0, device="cpu")


def test_exports_symbols_and_schemas():
    import torch_nfft
    import torch_nfft_amd as tn
    from torch_nfft_amd import _lib
    for name in ("YukawaSplitting", "nfft_ewald_yukawa", "nfft_ewald_yukawa_energy", "NfftEwaldYukawaFunction",
                 "nfft_ewald_yukawa_virial"):
        assert name in tn.__all__ and name in torch_nfft.__all__ and getattr(torch_nfft, name) is getattr(tn, name)
    assert torch_nfft.yukawa is tn.yukawa
    lib = _lib.load()
    assert _lib.ABI_VERSION == 7 and lib.nfft_hip_abi_version() == 7
    for name in ("nfft_hip_ewald_yukawa_near", "nfft_hip_ewald_yukawa_near_box", "nfft_hip_ewald_yukawa_virial_near"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    s = str(torch.ops.torch_nfft._nfft_ewald_yukawa_near.default._schema)
    assert s == ("torch_nfft::_nfft_ewald_yukawa_near(Tensor pos, Tensor x, Tensor? batch, float[] box, float alpha, float r_cut, "
                 "float screening, bool with_field) -> (Tensor, Tensor)")
    s = str(torch.ops.torch_nfft._nfft_ewald_yukawa_virial_near.default._schema)
    assert s == ("torch_nfft::_nfft_ewald_yukawa_virial_near(Tensor pos, Tensor x, Tensor? batch, float[] box, float alpha, "
                 "float r_cut, float screening) -> Tensor")
    q, pos = torch.zeros(5), torch.zeros(5, 3)
    six = (1.0, 0.0, 1.3, 0.0, 0.0, 0.8)
    with pytest.raises(RuntimeError, match="torch_nfft._nfft_ewald_yukawa_near is currently only implemented for GPU tensors"):
        tn.ops.nfft_ewald_yukawa_near(pos, q, None, (), 5.0, 0.3, 2.0, True)
    with pytest.raises(RuntimeError, match="torch_nfft._nfft_ewald_yukawa_near is currently only implemented for GPU tensors"):
        tn.ops.nfft_ewald_yukawa_near(pos, q, None, six, 5.0, 0.25, 2.0, False)
    with pytest.raises(RuntimeError, match="torch_nfft._nfft_ewald_yukawa_virial_near is currently only implemented for GPU tensors"):
        tn.ops.nfft_ewald_yukawa_virial_near(pos, q, None, six, 5.0, 0.25, 2.0)


def test_refusals():
    import torch_nfft_amd as tn
    for bad in (dict(screening=0.0), dict(screening=-1.0), dict(screening=float("nan")), dict(screening=float("inf")),
                dict(screening=50.0001 / 0.3), dict(r_cut=0.34), dict(bandwidth=31), dict(alpha=0.0),
                dict(box=[1.0, 1.0, 0.8])):  # (r_cut = 0.3 > 0.8 / 3)
        kw = dict(alpha=6.0, r_cut=0.3, bandwidth=16, screening=2.0, device="cpu")
        kw.update(bad)
        with pytest.raises(ValueError, match="YukawaSplitting"):
            tn.YukawaSplitting(**kw)
    with pytest.raises(ValueError, match="EwaldSplitting"):  # zero screening: the message names the class to use
        tn.YukawaSplitting(6.0, 0.3, 16, 0.0, device="cpu")
    assert tn.YukawaSplitting(6.0, 0.3, 16, 50.0 / 0.3 * (1 - 1e-15), device="cpu").cells == (3, 3, 3)
    with pytest.raises(AssertionError, match="box requires grad"):
        tn.YukawaSplitting(6.0, 0.3, 16, 2.0, box=torch.ones(3, requires_grad=True), device="cpu")
    spb = tn.YukawaSplitting(6.0, 0.25, 16, 2.0, box=[1.0, 1.3, 0.8], device="cpu")
    assert spb.cells == (4, 5, 3) and spb.box6 == (1.0, 0.0, 1.3, 0.0, 0.0, 0.8)
    sp = tn.YukawaSplitting(6.0, 0.3, 16, 2.0, device="cpu")
    q, pos = torch.zeros(5), torch.zeros(5, 3)
    for fn in (tn.nfft_ewald_yukawa, tn.nfft_ewald_yukawa_energy, tn.nfft_ewald_yukawa_virial):
        with pytest.raises(ValueError, match="three-dimensional"):
            fn(q, torch.zeros(5, 2), splitting=sp)
        with pytest.raises(AssertionError, match="batch"):
            fn(q, pos, torch.zeros(5, requires_grad=True), splitting=sp)
        with pytest.raises(RuntimeError, match="is currently only implemented for GPU tensors"):
            fn(q, pos, splitting=sp)
        with pytest.raises(RuntimeError, match="is currently only implemented for GPU tensors"):
            fn(q, pos, splitting=spb)
        with pytest.raises(TypeError, match="YukawaSplitting"):
            fn(q, pos)
        with pytest.raises(TypeError, match="YukawaSplitting"):  # the Coulomb splitting is the wrong class
            fn(q, pos, splitting=tn.EwaldSplitting(6.0, 0.3, 16, device="cpu"))
        with pytest.raises(ValueError, match="fractional"):
            fn(q, pos, splitting=sp, fractional=True)
    with pytest.raises(TypeError):  # ... and the other way round
        tn.nfft_ewald(q, pos, splitting=sp)
    with pytest.raises(ValueError, match="real"):
        tn.nfft_ewald_yukawa_virial(torch.zeros(5, dtype=torch.complex64), pos, splitting=sp)


def test_c_abi_validation_without_gpu():
    """the three entry points validate as their Coulomb twins do, take the workspace that the shared functions report, and
    check the screening before anything else"""
    from torch_nfft_amd import _lib
    lib = _lib.load()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(256)  # (never dereferenced: the checks come first)

    def problem(**kw):
        f = dict(cells_per_axis=4, with_field=1, num_points=1000, num_columns=2, batch_size=1, alpha=6.0, r_cut=0.25)
        f.update(kw)
        return _lib.EwaldProblem(**f)

    def call(q, ws=null, nbytes=0, z=one, field=one, points=one, lam=3.0):
        return lib.nfft_hip_ewald_yukawa_near(ctypes.byref(q), points, one, one, one, lam, z, field, ws, nbytes, null)

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
    assert call(problem(num_points=0), lam=0.0) == _lib.OK and call(ok, lam=0.0) == _lib.EWORKSPACE
    assert call(ok, lam=50.0 / 0.25) == _lib.EWORKSPACE  # (the bound itself is allowed)

    def box_problem(**kw):
        f = dict(cells=(ctypes.c_int32 * 3)(4, 5, 3), with_field=1, num_points=1000, num_columns=2, batch_size=1, alpha=6.0,
                 r_cut=0.25, box=(ctypes.c_double * 6)(1.0, 0.0, 1.3, 0.0, 0.0, 0.8))
        f.update(kw)
        return _lib.EwaldBoxProblem(**f)

    def box_call(q, ws=null, nbytes=0, z=one, field=one, lam=3.0):
        return lib.nfft_hip_ewald_yukawa_near_box(ctypes.byref(q), one, one, one, one, lam, z, field, ws, nbytes, null)

    def virial_call(q, ws=null, nbytes=0, out=one, points=one, lam=3.0):
        return lib.nfft_hip_ewald_yukawa_virial_near(ctypes.byref(q), points, one, one, lam, out, ws, nbytes, null)

    okb = box_problem()
    needb = lib.nfft_hip_ewald_near_box_workspace_bytes(ctypes.byref(okb))
    needv = lib.nfft_hip_ewald_virial_near_workspace_bytes(ctypes.byref(okb))
    assert needb > 0 and needv > 0
    assert box_call(okb) == _lib.EWORKSPACE and box_call(okb, one, needb - 1) == _lib.EWORKSPACE
    assert box_call(okb, field=null) == _lib.EINVAL and box_call(okb, z=null) == _lib.EINVAL
    assert virial_call(okb) == _lib.EWORKSPACE and virial_call(okb, one, needv - 1) == _lib.EWORKSPACE
    assert virial_call(okb, out=null) == _lib.EINVAL and virial_call(okb, points=null) == _lib.EINVAL
    for bad in (box_problem(cells=(ctypes.c_int32 * 3)(4, 6, 3)), box_problem(r_cut=0.3), box_problem(alpha=float("nan")),
                box_problem(box=(ctypes.c_double * 6)(1.0, 0.0, -1.3, 0.0, 0.0, 0.8))):
        assert box_call(bad) == _lib.EINVAL and _lib.last_error().startswith("Input mismatch")
        assert virial_call(bad) == _lib.EINVAL and _lib.last_error().startswith("Input mismatch")
    assert virial_call(box_problem(num_columns=1 << 21)) == _lib.EINVAL
    assert box_call(box_problem(num_points=0)) == _lib.OK and virial_call(box_problem(num_columns=0)) == _lib.OK
    # the screening: refused before the empty-problem return, with its name in the message
    for lam in (-1.0, float("nan"), float("inf"), 50.0001 / 0.25):
        for q, qb in ((ok, okb), (problem(num_points=0), box_problem(num_points=0))):
            for rc in (call(q, lam=lam), box_call(qb, lam=lam), virial_call(qb, lam=lam)):
                assert rc == _lib.EINVAL
                assert _lib.last_error().startswith("Input mismatch") and "screening" in _lib.last_error()
    assert box_call(box_problem(num_points=0), lam=0.0) == _lib.OK


def test_pair_kernel_resource_usage():
    """exactly the twelve instantiations <CC, FIELD, BOX> of the sweep and the three <CC> of the pair reduction, each without
    scratch and without spills, with the LDS of their dispersion twins (the library's own flags; VGPRs and occupancy are
    recorded in DESIGN.md section 7p, not gated)"""
    from resource_usage import resource_usage
    usage = resource_usage("ewald_yukawa.hip")
    sweep, red = {}, {}
    for name, u in usage.items():
        m = re.search(r"ewald_yukawa_near_kernelILi(\d)ELb(\d)ELb(\d)EE", name)
        v = re.search(r"virial_near_kernelILi(\d)E\w*?YukawaVirialWeightE", name)  # (virial_frame.h)
        assert m or v, name  # (nothing else in that file)
        if m:
            sweep[(int(m.group(1)), int(m.group(2)), int(m.group(3)))] = u
        else:
            red[int(v.group(1))] = u
    assert set(sweep) == {(cc, f, box) for cc in (1, 2, 4) for f in (0, 1) for box in (0, 1)} and set(red) == {1, 2, 4}
    assert len(usage) == 15
    twin_sweep, twin_red = {}, {}
    for name, u in resource_usage("ewald_disp.hip").items():
        m = re.search(r"ewald_disp_near_kernelILi(\d)ELb(\d)ELb(\d)EE", name)
        twin_sweep[(int(m.group(1)), int(m.group(2)), int(m.group(3)))] = u
    for name, u in resource_usage("ewald_disp_virial.hip").items():
        v = re.search(r"virial_near_kernelILi(\d)E\w*?DispersionVirialWeightE", name)
        if v:
            twin_red[int(v.group(1))] = u
    for kind, by, twin in (("sweep", sweep, twin_sweep), ("virial", red, twin_red)):
        for key, u in sorted(by.items()):
            print(kind, key, "VGPRs %d occupancy %d LDS %d (twin: VGPRs %d occupancy %d)"
                  % (u["VGPRs"], u["Occupancy"], u["LDS Size"], twin[key]["VGPRs"], twin[key]["Occupancy"]))
            assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (key, u)
            assert u["LDS Size"] == twin[key]["LDS Size"]
