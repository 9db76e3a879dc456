"""Float64 restatement of the Ewald sum for the periodic screened Coulomb (Yukawa) potential e^(-lambda r) / r -- TEST
INFRASTRUCTURE ONLY.

Written independently of ``torch_nfft_amd/yukawa.py``, dense numpy in float64 (``torch.special.erfc`` for erfc, as in
``tests/ewald_ref.py``).  The box is the matrix ``A`` ``[3, 3]`` whose rows are the lattice vectors (``None``: the unit cube),
the positions are FRACTIONAL, ``x = s A``, ``kappa = A^-1 k``, ``V = det A``; ``lam`` is the screening parameter,
``beta = lam / (2 alpha)`` and ``K = 4 pi^2 |kappa|^2 + lam^2``:

``lattice_sum``            brute force: every image ``|n|_inf <= radius`` of every pair, ``q_j e^(-lam |d|) / |d|`` (the sum converges
                           like ``e^(-lam w radius)`` for the smallest perpendicular width ``w``); ``background``: minus the mean
                           potential ``4 pi Q / (V lam^2)`` of the one-component plasma
``lattice_energy``         ``1/2 sum q_i phi_i`` of that, per column
``pair_weights``           ``w = (P + M) / (2 r)`` and ``mg = -w'/r = (w - lam D + g) / r^2``, ``P = e^(lam r) erfc(alpha r + beta)``,
                           ``M = e^(-lam r) erfc(alpha r - beta)``, ``D = (P - M) / 2``, ``g = (2 alpha / sqrt(pi)) e^(-alpha^2 r^2 - beta^2)``;
                           ``mutant`` names one mistake of a pair weight (the sensitivity test)
``near_sum`` / ``near_field``  the pair sums over the wrapped minimum image with ``0 < r < r_c`` (duplicates skipped)
``coeffs`` / ``strain_coeffs``  ``b_k = 4 pi e^(-K / (4 alpha^2)) / (V K)`` and ``t_k = -8 pi^2 b_k (1 / (4 alpha^2) + 1 / K)`` on
                           ``[-N/2, N/2)^3``, the unpaired planes ``k_a = -N/2`` zeroed, ``b_0`` zeroed with ``background``
``yukawa``                 near + far - self (+ background): the algorithm in exact arithmetic, per point set
``near_virial``            the pair part of the next alone, ``[B, 7, *cols]`` in the order of the native pair reduction
``virial``                 ``(U, W)`` of the same: pairs (``near_virial``), frequencies, self and background terms
``near_points``            the 512 points of the GPU near-sweep tests
"""
import itertools
import math

import numpy as np

import dispersion_ref as dr
from dispersion_ref import _box, _columns, _sets, _shaped, erfc

MUTANTS = ("beta_sign", "no_plus", "no_ebeta", "coulomb")


def self_term(alpha, lam):
    beta = lam / (2.0 * alpha)
    return 2.0 * alpha / math.sqrt(math.pi) * math.exp(-beta * beta) - lam * math.erfc(beta)


def background_term(alpha, lam, V):
    """what ``background=True`` adds to phi_i per unit of total charge: b_0 - 4 pi / (V lam^2)"""
    beta = lam / (2.0 * alpha)
    return 4.0 * math.pi / (V * lam * lam) * math.expm1(-beta * beta)


def lattice_sum(q, s, A, lam, radius, batch=None, background=False, reach=None):
    """(phi [n, *cols], E = -grad_x phi [n, 3, *cols]): q_j e^(-lam |d|) / |d| over all pairs and the images |n|_inf <= radius,
    the self pair's images n != 0 included.  reach: the differences are wrapped first and the images that lie further than
    reach from every wrapped difference are skipped (each of their terms is below e^(-lam reach) / reach)"""
    q0 = np.asarray(q)
    s = np.asarray(s, dtype=np.float64)
    A = _box(A)
    V = abs(np.linalg.det(A))
    qc = _columns(q0)
    phi = np.zeros_like(qc)
    E = np.zeros((qc.shape[0], 3, qc.shape[1]), dtype=qc.dtype)
    shifts = np.array(list(itertools.product(range(-radius, radius + 1), repeat=3)), dtype=np.float64)
    if reach is not None:  # (a wrapped difference is shorter than half the sum of the lattice vectors' lengths)
        shifts = shifts[np.linalg.norm(shifts @ A, axis=1) < reach + 0.5 * np.linalg.norm(A, axis=1).sum()]
    for sel in _sets(batch, s.shape[0]):
        if sel.size == 0:
            continue
        ds = s[sel][:, None, :] - s[sel][None, :, :]
        if reach is not None:
            ds = ds - np.rint(ds)
        p = np.zeros_like(qc[sel])
        e = np.zeros((sel.size, 3, qc.shape[1]), dtype=qc.dtype)
        step = max(1, 200000 // (sel.size * sel.size))
        for m0 in range(0, shifts.shape[0], step):
            d = (ds[None] + shifts[m0:m0 + step, None, None, :]) @ A  # [images, n, n, 3]
            r = np.sqrt((d * d).sum(-1))
            ok = r > 0
            rs = np.where(ok, r, 1.0)
            k0 = np.where(ok, np.exp(-lam * rs) / rs, 0.0)
            k1 = k0 * (lam + 1.0 / rs) / rs  # -K'(r) / r
            p += k0.sum(0) @ qc[sel]
            e += np.einsum("ija,jc->iac", (k1[..., None] * d).sum(0), qc[sel])
        if background:
            p -= 4.0 * math.pi / (V * lam * lam) * qc[sel].sum(0, keepdims=True)
        phi[sel] = p
        E[sel] = e
    return _shaped(q0, phi, E)


def lattice_energy(q, s, A, lam, radius, background=False):
    """1/2 sum_i q_i phi_i of one point set: [*cols]"""
    q0 = np.asarray(q, dtype=np.float64)
    return 0.5 * (q0 * lattice_sum(q0, s, A, lam, radius, background=background)[0]).sum(0)


def pair_weights(d, alpha, lam, r_c=None, mutant=None):
    """(w, mg) for the difference vectors d [.., 3]; zero where r = 0 or r >= r_c"""
    assert mutant is None or mutant in MUTANTS
    rr = (d * d).sum(-1)
    ok = rr > 0 if r_c is None else (rr > 0) & (rr < r_c * r_c)
    r = np.sqrt(np.where(ok, rr, 1.0))
    beta = lam / (2.0 * alpha)
    bs = -beta if mutant == "beta_sign" else beta
    P = np.exp(lam * r) * erfc(alpha * r + bs)
    M = np.exp(-lam * r) * erfc(alpha * r - bs)
    if mutant == "no_plus":
        P = np.zeros_like(P)
    g = 2.0 * alpha / math.sqrt(math.pi) * np.exp(-alpha * alpha * r * r - (0.0 if mutant == "no_ebeta" else beta * beta))
    w = (P + M) / (2.0 * r)
    mg = (w - lam * (P - M) / 2.0 + g) / (r * r)
    if mutant == "coulomb":
        w = erfc(alpha * r) / r
        mg = (w + 2.0 * alpha / math.sqrt(math.pi) * np.exp(-alpha * alpha * r * r)) / (r * r)
    return np.where(ok, w, 0.0), np.where(ok, mg, 0.0)


def _near(q, s, A, batch, alpha, lam, r_c, wrap=True, mutant=None):
    q0 = np.asarray(q)
    s = np.asarray(s, dtype=np.float64)
    A = _box(A)
    qc = _columns(q0)
    z = np.zeros_like(qc)
    f = np.zeros((qc.shape[0], 3, qc.shape[1]), dtype=qc.dtype)
    for sel in _sets(batch, s.shape[0]):
        for r0 in range(0, sel.size, 512):  # (rows in blocks: the pair arrays stay small)
            rows = sel[r0:r0 + 512]
            ds = s[rows][:, None, :] - s[sel][None, :, :]
            if wrap:
                ds = ds - np.rint(ds)
            d = ds @ A
            w, mg = pair_weights(d, alpha, lam, r_c, mutant)
            z[rows] += w @ qc[sel]
            f[rows] += np.einsum("ija,jc->iac", mg[..., None] * d, qc[sel])
    return _shaped(q0, z, f)


def near_sum(q, s, A, batch, alpha, lam, r_c, **kw):
    """z_i = sum_{j: 0 < r_ij < r_c, same set} w(r_ij) q_j, r_ij = |(ds - rint(ds)) A|"""
    return _near(q, s, A, batch, alpha, lam, r_c, **kw)[0]


def near_field(q, s, A, batch, alpha, lam, r_c, **kw):
    """f_i = sum_j mg(r_ij) d_ij q_j (Cartesian; minus the gradient of near_sum): [n, 3, *cols]"""
    return _near(q, s, A, batch, alpha, lam, r_c, **kw)[1]


def _K(A, lam, N):
    _, kap = dr.kappa(A, N)
    return 4.0 * math.pi ** 2 * (kap * kap).sum(-1) + lam * lam


def coeffs(A, alpha, lam, N, background=False):
    K = _K(A, lam, N)
    b = 4.0 * math.pi * np.exp(-K / (4.0 * alpha * alpha)) / (abs(np.linalg.det(_box(A))) * K)
    b[0, :, :] = 0.0
    b[:, 0, :] = 0.0
    b[:, :, 0] = 0.0
    if background:
        b[N // 2, N // 2, N // 2] = 0.0
    return b


def strain_coeffs(A, alpha, lam, N, background=False):
    return -8.0 * math.pi ** 2 * coeffs(A, alpha, lam, N, background) * (1.0 / (4.0 * alpha * alpha) + 1.0 / _K(A, lam, N))


def _far(q, s, A, batch, b, chunk=4096):
    """the direct sum over the frequencies of the grid b [N, N, N]: (z, f = minus the Cartesian gradient)"""
    q0 = np.asarray(q)
    s = np.asarray(s, dtype=np.float64)
    qc = _columns(q0)
    real = not np.iscomplexobj(qc)
    K, kap = dr.kappa(A, b.shape[0])
    b = b.reshape(-1)
    K, kap, b = K.reshape(-1, 3)[b != 0], kap.reshape(-1, 3)[b != 0], b[b != 0]
    z = np.zeros_like(qc)
    f = np.zeros((qc.shape[0], 3, qc.shape[1]), dtype=qc.dtype)
    for sel in _sets(batch, s.shape[0]):
        if sel.size == 0:
            continue
        p = np.zeros((sel.size, qc.shape[1]), dtype=np.complex128)
        g = np.zeros((sel.size, 3, qc.shape[1]), dtype=np.complex128)
        for c0 in range(0, K.shape[0], chunk):
            Kc, kc, bc = K[c0:c0 + chunk], kap[c0:c0 + chunk], b[c0:c0 + chunk]
            ph = np.exp(2j * math.pi * s[sel] @ Kc.T)      # [n, nk]: e^{+2 pi i k.s_i}
            Sk = (np.conj(ph).T @ qc[sel]) * bc[:, None]   # b_k sum_j q_j e^{-2 pi i k.s_j}
            p += ph @ Sk
            g -= np.einsum("ik,ka,kc->iac", ph, 2j * math.pi * kc, Sk)
        z[sel] = p.real if real else p
        f[sel] = g.real if real else g
    return _shaped(q0, z, f)


def _set_totals(q0, batch):
    """the total charge of i's point set, per column: the shape of q"""
    qc = _columns(q0)
    tot = np.zeros_like(qc)
    for sel in _sets(batch, qc.shape[0]):
        tot[sel] = qc[sel].sum(0, keepdims=True)
    return tot.reshape(q0.shape)


def yukawa(q, s, A, batch, alpha, lam, r_c, N, background=False):
    """(phi, E) of the split sum in exact arithmetic: near + far - self (+ background)"""
    q0 = np.asarray(q)
    z, f = _near(q0, s, A, batch, alpha, lam, r_c)
    zf, ff = _far(q0, s, A, batch, coeffs(A, alpha, lam, N, background))
    phi = z + zf - self_term(alpha, lam) * _columns(q0).reshape(q0.shape)
    if background:
        phi = phi + background_term(alpha, lam, abs(np.linalg.det(_box(A)))) * _set_totals(q0, batch)
    return phi, f + ff


def near_virial(q, s, A, batch, alpha, lam, r_c, mutant=None):
    """the pair part of ``virial`` alone, in the layout of the native pair reduction: [B, 7, *cols] -- energy, xx, yy, zz, yz, xz,
    xy of 1/2 sum_ij q_i q_j (w, mg d_a d_b) over the wrapped minimum images with 0 < r < r_c, real q; an empty point set
    gives zeros.  ``mutant``: one mistake of ``pair_weights``"""
    q0 = np.asarray(q)
    s = np.asarray(s, dtype=np.float64)
    Am = _box(A)
    qc = _columns(q0)
    assert not np.iscomplexobj(qc)
    sets = _sets(batch, s.shape[0])
    out = np.zeros((len(sets), 7, qc.shape[1]))
    for n, sel in enumerate(sets):
        if sel.size == 0:
            continue
        qs = qc[sel]
        ds = s[sel][:, None, :] - s[sel][None, :, :]
        d = (ds - np.rint(ds)) @ Am
        w, mg = pair_weights(d, alpha, lam, r_c, mutant)
        out[n, 0] = 0.5 * np.einsum("ic,ij,jc->c", qs, w, qs)
        for e, (a, b) in enumerate(((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))):
            out[n, 1 + e] = 0.5 * np.einsum("ic,ij,jc->c", qs, mg * d[..., a] * d[..., b], qs)
    return out.reshape((len(sets), 7) + q0.shape[1:])


def virial(q, s, A, batch, alpha, lam, r_c, N, background=False):
    """(U [B, *cols], W [B, 3, 3, *cols]) of the split sum in exact arithmetic, real q: W_ab = -dU / d eps_ab for
    A -> A (1 + eps) at fixed s and fixed lam"""
    q0 = np.asarray(q)
    s = np.asarray(s, dtype=np.float64)
    Am = _box(A)
    V = abs(np.linalg.det(Am))
    qc = _columns(q0)
    assert not np.iscomplexobj(qc)
    b, t = coeffs(A, alpha, lam, N, background).reshape(-1), strain_coeffs(A, alpha, lam, N, background).reshape(-1)
    K, kap = dr.kappa(A, N)
    K, kap, t, b = K.reshape(-1, 3)[b != 0], kap.reshape(-1, 3)[b != 0], t[b != 0], b[b != 0]
    sets = _sets(batch, s.shape[0])
    pairs = near_virial(qc, s, A, batch, alpha, lam, r_c)  # [B, 7, C]
    U = pairs[:, 0].copy()
    W = np.zeros((len(sets), 3, 3, qc.shape[1]))
    for e, (i, j) in enumerate(((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))):
        W[:, i, j] = W[:, j, i] = pairs[:, 1 + e]
    for n, sel in enumerate(sets):
        if sel.size == 0:
            continue
        qs = qc[sel]
        for c0 in range(0, K.shape[0], 4096):
            Kc, kc, bc, tc = K[c0:c0 + 4096], kap[c0:c0 + 4096], b[c0:c0 + 4096], t[c0:c0 + 4096]
            S = np.exp(-2j * math.pi * Kc @ s[sel].T) @ qs  # [nk, C]
            p = (S * np.conj(S)).real
            U[n] += 0.5 * (bc[:, None] * p).sum(0)
            W[n] += 0.5 * (np.einsum("k,kc->c", bc, p)[None, None] * np.eye(3)[:, :, None] + np.einsum("k,ka,kb,kc->abc", tc, kc, kc, p))
        U[n] -= 0.5 * self_term(alpha, lam) * (qs * qs).sum(0)
        if background:
            bg = 0.5 * background_term(alpha, lam, V) * qs.sum(0) ** 2
            U[n] += bg
            W[n] += bg[None, None] * np.eye(3)[:, :, None]
    cols = q0.shape[1:]
    return U.reshape((len(sets),) + cols), W.reshape((len(sets), 3, 3) + cols)


def near_points():
    """The 8^3 jittered lattice (spacing 1/8, jitter 0.03) with the edge cases of the wrap written over 29 of its nodes, those
    first -- the construction of tests/test_gpu_dispersion.py: points exactly on the lower faces and just below the upper
    ones, points given outside the box, exact duplicates, and a pair 0.04 apart through each face.  float32 [512, 3]"""
    rng = np.random.default_rng(0)
    x = dr.jittered_lattice(rng, 8, 1.0 / 8, 0.03)
    below = np.nextafter(np.float32(0.5), np.float32(0))  # the largest float32 below 1/2
    special = []

    def node(i, j, k):
        special.append((i, j, k))
        return (i, j, k)

    for a, idx in enumerate(((0, 2, 3), (3, 0, 2), (2, 3, 0))):      # exactly on the lower faces
        x[node(*idx)][a] = -0.5
    for a, idx in enumerate(((7, 5, 4), (4, 7, 5), (5, 4, 7))):      # just below the upper faces
        x[node(*idx)][a] = below
    x[node(7, 7, 7)][:] = below                                      # ... and in the upper corner
    for idx in ((1, 1, 1), (6, 1, 2), (2, 6, 1), (1, 2, 6)):         # given outside the box: must act as their images
        x[node(*idx)] += np.float32(0.7)
    for idx in ((5, 5, 1), (1, 5, 5), (5, 1, 5), (6, 6, 2)):
        x[node(*idx)] -= np.float32(1.2)
    for dst, src in (((3, 3, 3), (3, 3, 4)), ((4, 4, 4), (4, 4, 3)), ((3, 4, 3), (3, 4, 4)), ((4, 3, 4), (4, 3, 3))):
        x[node(*dst)] = x[node(*src)]                                # exact duplicates: r = 0
    for a, (p, q) in enumerate((((0, 6, 5), (7, 6, 5)), ((6, 0, 6), (6, 7, 6)), ((2, 5, 0), (2, 5, 7)))):
        x[node(*q)] = x[node(*p)] + np.float32(0.01)                 # a pair 0.04 apart through each face
        x[p][a], x[q][a] = -0.48, 0.48
    flat = [(i * 8 + j) * 8 + k for i, j, k in special]
    rest = np.setdiff1d(np.arange(512), flat)
    return x.reshape(-1, 3)[np.concatenate([flat, rng.permutation(rest)])]
