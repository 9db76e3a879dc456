"""Float64 restatement of the Ewald sum for point charges and point dipoles -- TEST INFRASTRUCTURE ONLY.

Written independently of ``torch_nfft_amd/dipole.py`` and of the kernels, dense numpy in float64 (``torch.special.erfc`` for
erfc, as in ``tests/ewald_ref.py``), straight from the formulas of DESIGN.md section 7l.  The box is the matrix ``A`` ``[3, 3]``
whose rows are the lattice vectors (``None``: the unit cube), the positions are FRACTIONAL, ``x = s A``, ``kappa = A^-1 k``,
``V = det A``; ``q`` ``[n, *cols]`` and the Cartesian ``mu`` ``[n, 3, *cols]`` (either may be ``None``).  Every function returns
``(phi [n, *cols], E [n, 3, *cols], T [n, 3, 3, *cols] or None)``, ``T`` at ``order = 2``.

``smith``            ``B_0 .. B_3`` of the distances r
``near``             the pair sums over the wrapped minimum image with ``0 < r < r_c``
``near_f32``         the same image and recurrences in numpy float32 arithmetic: what float32 does to these points
``far``              the dense sum over ``k in [-N/2, N/2)^3``, the unpaired planes ``k_a = -N/2`` zeroed (``kmax``: over
                     ``|k|_inf <= kmax`` instead)
``terms``            the self and background terms
``exact_algorithm``  near + far + terms: the algorithm in exact arithmetic
``converged``        5^3 images without a cut, ``|k|_inf <= 14``
``energy`` / ``force``   ``U = 1/2 sum (q phi - mu . E)`` per point set, and ``q E + T mu``
"""
import itertools
import math

import numpy as np
import torch

from dispersion_ref import kappa

VOIGT = ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))


def erfc(a):
    return torch.special.erfc(torch.from_numpy(np.ascontiguousarray(a))).numpy()


def _box(A):
    return np.eye(3) if A is None else np.asarray(A, dtype=np.float64)


def _sets(batch, n):
    if batch is None:
        return [np.arange(n)]
    batch = np.asarray(batch)
    return [np.nonzero(batch == b)[0] for b in range(int(batch.max()) + 1 if batch.size else 0)]


def _sources(q, mu, n, dtype=np.float64):
    """(q [n, C], mu [n, 3, C], cols)"""
    cols = tuple(np.shape(q)[1:]) if q is not None else tuple(np.shape(mu)[2:])
    C = int(np.prod(cols, dtype=np.int64))
    qc = np.zeros((n, C), dtype) if q is None else np.asarray(q, dtype=dtype).reshape(n, C)
    mc = np.zeros((n, 3, C), dtype) if mu is None else np.asarray(mu, dtype=dtype).reshape(n, 3, C)
    return qc, mc, cols


def _shaped(phi, E, T, cols, order):
    n = phi.shape[0]
    return phi.reshape((n,) + cols), E.reshape((n, 3) + cols), T.reshape((n, 3, 3) + cols) if order == 2 else None


def smith(r, alpha):
    """[B_0, B_1, B_2, B_3] of r > 0: B_0 = erfc(alpha r) / r, B_l = ((2l - 1) B_(l-1) + (2 alpha^2)^l / (alpha sqrt(pi))
    e^(-alpha^2 r^2)) / r^2, in the arithmetic of r"""
    one = r.dtype.type
    g = np.exp(-(one(alpha) * r) ** 2) / one(alpha * math.sqrt(math.pi))
    B = [erfc(one(alpha) * r) / r]
    for l in (1, 2, 3):
        B.append((one(2 * l - 1) * B[-1] + one((2.0 * alpha * alpha) ** l) * g) / (r * r))
    return B


def _pair_sums(d, ok, qs, ms, alpha, order, b3=True, mdelta=True):
    """the sums of one block of rows: d [rows, n, 3] (Cartesian), ok [rows, n], sources qs [n, C], ms [n, 3, C]"""
    r = np.sqrt((d * d).sum(-1))
    B = [np.where(ok, b, 0) for b in smith(np.where(ok, r, 1).astype(d.dtype), alpha)]
    rows, n, C = d.shape[0], d.shape[1], qs.shape[1]
    m = sum(d[..., a, None] * ms[None, :, a, :] for a in range(3))  # mu_j . d: [rows, n, C]
    phi = B[0] @ qs + (B[1][..., None] * m).sum(1)
    # (q_j B_1 + m B_2) d_a - mu_j,a B_1        (sums over j as matrix products)
    dt = d.transpose(0, 2, 1)  # [rows, 3, n]
    E = dt @ (B[1][..., None] * qs[None] + B[2][..., None] * m) - (B[1] @ ms.reshape(n, 3 * C)).reshape(rows, 3, C)
    if order != 2:
        return phi, E, None
    eye = np.eye(3, dtype=d.dtype)
    # q_j (delta_ab B_1 - d_a d_b B_2)
    T = eye[None, :, :, None] * (B[1] @ qs)[:, None, None, :]
    ddt = (d[..., :, None] * d[..., None, :]).reshape(rows, n, 9).transpose(0, 2, 1)  # d_a d_b: [rows, 9, n]
    T = T - (ddt @ (B[2][..., None] * qs[None])).reshape(rows, 3, 3, C)
    # (mu_j,a d_b + mu_j,b d_a + m delta_ab) B_2
    md = np.stack([(B[2] * d[..., b]) @ ms.reshape(n, 3 * C) for b in range(3)], 1).reshape(rows, 3, 3, C)  # [rows, b, a, C]
    T = T + md + md.transpose(0, 2, 1, 3)
    if mdelta:
        T = T + eye[None, :, :, None] * (B[2][..., None] * m).sum(1)[:, None, None, :]
    # - m d_a d_b B_3
    if b3:
        T = T - (ddt @ (B[3][..., None] * m)).reshape(rows, 3, 3, C)
    return phi, E, T


def near(q, mu, s, A, batch, alpha, r_c, order=2, nimg=0, wrap=True, b3=True, mdelta=True):
    """the pair sums over d = (ds - rint(ds)) A with 0 < |d| < r_c (r_c = None with nimg = 2: every image within two cells, no
    cut).  The mistakes of the sensitivity test: wrap=False, b3=False (the B_3 term dropped), mdelta=False (the m delta_ab B_2
    term dropped)."""
    s = np.asarray(s, dtype=np.float64)
    n = s.shape[0]
    A = _box(A)
    qc, mc, cols = _sources(q, mu, n)
    C = qc.shape[1]
    phi, E, T = np.zeros((n, C)), np.zeros((n, 3, C)), np.zeros((n, 3, 3, C))
    for sel in _sets(batch, n):
        for r0 in range(0, sel.size, 256):  # (rows in blocks: the pair arrays stay small)
            rows = sel[r0:r0 + 256]
            ds = s[rows][:, None, :] - s[sel][None, :, :]
            if wrap:
                ds = ds - np.rint(ds)
            for sh in itertools.product(range(-nimg, nimg + 1), repeat=3):
                d = (ds + np.array(sh, dtype=np.float64)) @ A
                rr = (d * d).sum(-1)
                ok = rr > 0 if r_c is None else (rr > 0) & (rr < r_c * r_c)
                p, e, t = _pair_sums(d, ok, qc[sel], mc[sel], alpha, order, b3, mdelta)
                phi[rows] += p
                E[rows] += e
                if order == 2:
                    T[rows] += t
    return _shaped(phi, E, T, cols, order)


def near_f32(q, mu, s, A, batch, alpha, r_c, order=2):
    """``near`` in numpy float32 arithmetic: the positions reduced to [-1/2, 1/2), their differences wrapped and multiplied
    with the float32 box, r^2 compared with the float32 r_c^2, the Smith recurrence and every product and sum in float32 (erfc
    and exp as torch and numpy round them in float32).  Not the device's bits: the same number format on the same points."""
    f = np.float32
    s = np.asarray(s, dtype=f)
    s = s - np.rint(s)
    n = s.shape[0]
    A = _box(A).astype(f)
    qc, mc, cols = _sources(q, mu, n, f)
    C = qc.shape[1]
    phi, E, T = np.zeros((n, C), f), np.zeros((n, 3, C), f), np.zeros((n, 3, 3, C), f)
    rc2 = f(r_c * r_c)
    for sel in _sets(batch, n):
        for r0 in range(0, sel.size, 256):
            rows = sel[r0:r0 + 256]
            ds = s[rows][:, None, :] - s[sel][None, :, :]
            ds = ds - np.rint(ds)
            d = np.stack([ds[..., 0] * A[0, 0] + ds[..., 1] * A[1, 0] + ds[..., 2] * A[2, 0],
                          ds[..., 1] * A[1, 1] + ds[..., 2] * A[2, 1], ds[..., 2] * A[2, 2]], -1)
            rr = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
            ok = (rr > 0) & (rr < rc2)
            p, e, t = _pair_sums(d, ok, qc[sel], mc[sel], alpha, order)
            assert p.dtype == f and e.dtype == f
            phi[rows], E[rows] = p, e
            if order == 2:
                assert t.dtype == f
                T[rows] = t
    return _shaped(phi, E, T, cols, order)


def coeffs(A, alpha, N=None, kmax=None):
    """(K [nk, 3] integer frequencies, kappa [nk, 3], b [nk]) with b != 0: b_k = exp(-pi^2 |kappa|^2 / alpha^2) / (pi V |kappa|^2)
    on [-N/2, N/2)^3 without k = 0 and the unpaired planes k_a = -N/2, or on 0 < |k|_inf <= kmax"""
    if kmax is None:
        K, kap = kappa(A, N)
        keep = (K > -(N // 2)).all(-1) & (K != 0).any(-1)
    else:
        K, kap = kappa(A, 2 * kmax + 2)
        keep = (np.abs(K) <= kmax).all(-1) & (K != 0).any(-1)
    K, kap = K[keep], kap[keep]
    k2 = (kap * kap).sum(-1)
    V = abs(np.linalg.det(_box(A)))
    return K, kap, np.exp(-math.pi ** 2 * k2 / alpha ** 2) / (math.pi * V * k2)


def far(q, mu, s, A, batch, alpha, N=None, order=2, kmax=None, chunk=4096):
    """phi = sum_k b_k rho_k e^{2 pi i k.s}, rho_k = sum_j (q_j - 2 pi i kappa . mu_j) e^{-2 pi i k.s_j}; E_a with the factor
    (-2 pi i kappa_a), T_ab with 4 pi^2 kappa_a kappa_b"""
    s = np.asarray(s, dtype=np.float64)
    n = s.shape[0]
    qc, mc, cols = _sources(q, mu, n)
    C = qc.shape[1]
    K, kap, b = coeffs(A, alpha, N, kmax)
    phi, E, T = np.zeros((n, C)), np.zeros((n, 3, C)), np.zeros((n, 3, 3, C))
    for sel in _sets(batch, n):
        if sel.size == 0:
            continue
        for c0 in range(0, K.shape[0], chunk):
            Kc, kc, bc = K[c0:c0 + chunk], kap[c0:c0 + chunk], b[c0:c0 + chunk]
            ph = np.exp(2j * math.pi * s[sel] @ Kc.T)  # [n, nk]: e^{+2 pi i k.s_i}
            nk = Kc.shape[0]
            hat = np.conj(ph).T @ np.concatenate([qc[sel], mc[sel].reshape(sel.size, 3 * C)], 1)  # [nk, 4 C]: of q and of mu
            S = bc[:, None] * (hat[:, :C] - 2j * math.pi * (kc[:, :, None] * hat[:, C:].reshape(nk, 3, C)).sum(1))
            phi[sel] += (ph @ S).real
            E[sel] += (ph @ (-2j * math.pi * kc[:, :, None] * S[:, None, :]).reshape(nk, 3 * C)).real.reshape(sel.size, 3, C)
            if order == 2:
                kk = 4.0 * math.pi ** 2 * (kc[:, :, None] * kc[:, None, :]).reshape(nk, 9)
                T[sel] += (ph @ (kk[:, :, None] * S[:, None, :]).reshape(nk, 9 * C)).real.reshape(sel.size, 3, 3, C)
    return _shaped(phi, E, T, cols, order)


def terms(q, mu, n, A, batch, alpha, order=2):
    """the self and background terms: -(2 alpha / sqrt(pi)) q_i - pi Q / (alpha^2 V) in phi, +(4 alpha^3 / (3 sqrt(pi))) mu_i in E,
    -(4 alpha^3 / (3 sqrt(pi))) q_i delta_ab in T"""
    qc, mc, cols = _sources(q, mu, n)
    V = abs(np.linalg.det(_box(A)))
    total = np.zeros_like(qc)
    for sel in _sets(batch, n):
        total[sel] = qc[sel].sum(0, keepdims=True)
    c3 = 4.0 * alpha ** 3 / (3.0 * math.sqrt(math.pi))
    phi = -2.0 * alpha / math.sqrt(math.pi) * qc - math.pi / (alpha ** 2 * V) * total
    T = -c3 * np.eye(3)[None, :, :, None] * qc[:, None, None, :]
    return _shaped(phi, c3 * mc, T, cols, order)


def _add(*parts):
    return tuple(None if p[0] is None else sum(p) for p in zip(*parts))


def exact_algorithm(q, mu, s, A, batch, alpha, r_c, N, order=2):
    """the algorithm in exact arithmetic: near + far over [-N/2, N/2)^3 + self and background"""
    n = np.shape(s)[0]
    return _add(near(q, mu, s, A, batch, alpha, r_c, order), far(q, mu, s, A, batch, alpha, N, order),
                terms(q, mu, n, A, batch, alpha, order))


def converged(q, mu, s, A, batch=None, alpha=6.0, order=2, nimg=2, kmax=14):
    """the sum carried to convergence: 5^3 images without a cut, |k|_inf <= 14"""
    n = np.shape(s)[0]
    return _add(near(q, mu, s, A, batch, alpha, None, order, nimg=nimg), far(q, mu, s, A, batch, alpha, None, order, kmax=kmax),
                terms(q, mu, n, A, batch, alpha, order))


def energy(q, mu, phi, E, batch=None):
    """U_b = 1/2 sum_{i in set b} (q_i phi_i - mu_i . E_i): [B, *cols]"""
    n = phi.shape[0]
    u = np.zeros_like(phi) if q is None else np.asarray(q, dtype=np.float64) * phi
    if mu is not None:
        u = u - (np.asarray(mu, dtype=np.float64) * E).sum(1)
    return np.stack([0.5 * u[sel].sum(0) for sel in _sets(batch, n)])


def force(q, mu, E, T):
    """q_i E_i + T_i mu_i: [n, 3, *cols]"""
    f = np.zeros_like(E)
    if q is not None:
        f = f + np.asarray(q, dtype=np.float64)[:, None] * E
    if mu is not None:
        f = f + (T * np.asarray(mu, dtype=np.float64)[:, None]).sum(2)
    return f


def spectral_table(A, alpha, N, order=2):
    """[N, N, N, 4 or 10, 4] complex128: what turns the adjoint transform of the packed sources (q, mu) into the spectra of
    (phi, E, T) in the sign convention of the transforms (the adjoint sums e^{+2 pi i k.s}, the forward e^{-2 pi i k.s}:
    k -> -k against ``far``): row 0 is b_k (1, 2 pi i kappa), row 1 + a is 2 pi i kappa_a times row 0, row 4 + e is
    4 pi^2 kappa_a kappa_b times row 0 (e in the order of VOIGT); b_0 = 0 and the unpaired planes zeroed"""
    K, kap = kappa(A, N)
    k2 = (kap * kap).sum(-1)
    V = abs(np.linalg.det(_box(A)))
    b = np.exp(-math.pi ** 2 * k2 / alpha ** 2) / (math.pi * V * np.where(k2 > 0, k2, 1.0))
    b[~((K > -(N // 2)).all(-1) & (K != 0).any(-1))] = 0.0
    tau = 2.0 * math.pi * kap
    row0 = b[..., None] * np.concatenate([np.ones(k2.shape + (1,)), 1j * tau], -1)  # [N, N, N, 4]
    rows = [row0] + [1j * tau[..., a, None] * row0 for a in range(3)]
    if order == 2:
        rows += [(tau[..., a] * tau[..., c])[..., None] * row0 for a, c in VOIGT]
    return np.stack(rows, 3)


def near_points():
    """The 8^3 jittered lattice (spacing 1/8, jitter 0.03) of the dispersion sum's near-sweep tests with the same edge cases of
    the wrap written over 29 of its nodes, those first: points exactly on the lower faces, just below the upper faces and in
    the upper corner, points given outside the box, exact duplicates, a pair 0.04 apart through each face.  float32 [512, 3]"""
    from dispersion_ref import jittered_lattice
    rng = np.random.default_rng(0)
    x = jittered_lattice(rng, 8, 1.0 / 8, 0.03)
    below = np.nextafter(np.float32(0.5), np.float32(0))  # the largest float32 below 1/2
    special = []

    def node(i, j, k):
        special.append((i, j, k))
        return (i, j, k)

    for a, idx in enumerate(((0, 2, 3), (3, 0, 2), (2, 3, 0))):
        x[node(*idx)][a] = -0.5
    for a, idx in enumerate(((7, 5, 4), (4, 7, 5), (5, 4, 7))):
        x[node(*idx)][a] = below
    x[node(7, 7, 7)][:] = below
    for idx in ((1, 1, 1), (6, 1, 2), (2, 6, 1), (1, 2, 6)):
        x[node(*idx)] += np.float32(0.7)
    for idx in ((5, 5, 1), (1, 5, 5), (5, 1, 5), (6, 6, 2)):
        x[node(*idx)] -= np.float32(1.2)
    for dst, src in (((3, 3, 3), (3, 3, 4)), ((4, 4, 4), (4, 4, 3)), ((3, 4, 3), (3, 4, 4)), ((4, 3, 4), (4, 3, 3))):
        x[node(*dst)] = x[node(*src)]
    for a, (p, q) in enumerate((((0, 6, 5), (7, 6, 5)), ((6, 0, 6), (6, 7, 6)), ((2, 5, 0), (2, 5, 7)))):
        x[node(*q)] = x[node(*p)] + np.float32(0.01)
        x[p][a], x[q][a] = -0.48, 0.48
    flat = [(i * 8 + j) * 8 + k for i, j, k in special]
    rest = np.setdiff1d(np.arange(512), flat)
    return x.reshape(-1, 3)[np.concatenate([flat, rng.permutation(rest)])]


def near_sources(seed, n, cols):
    """signed (q [n, *cols], mu [n, 3, *cols]) float32 from a seeded normal distribution"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n,) + cols).astype(np.float32), rng.standard_normal((n, 3) + cols).astype(np.float32)


def near_gate(what, got_f32, ref, committed):
    """The gate of a device pair sweep for one quantity: max(4 x rel_l2(float32 emulation, float64), the committed figure of the
    Coulomb pair loop).  The emulation is the number format's own rounding on these points, the committed figure what the
    erfcf / __expf pair loop measured on the hardware, 4 x the project's margin.  Returns (gate, emulation term)."""
    emu = float(np.linalg.norm(got_f32.astype(np.float64) - ref) / np.linalg.norm(ref))
    return max(4.0 * emu, committed), emu


def voigt(T):
    """[n, 3, 3, *cols] as [n, 6, *cols] in the order xx, yy, zz, yz, xz, xy"""
    return np.stack([T[:, a, b] for a, b in VOIGT], 1)
