"""Float64 restatement of the periodic Stokeslet sum (Hasimoto's Ewald sum) -- TEST INFRASTRUCTURE ONLY.

Written independently of ``torch_nfft_amd/stokeslet.py`` and of the kernels, dense numpy in float64 (``torch.special.erfc`` for
erfc, as in ``tests/dipole_ref.py``), straight from the formulas of DESIGN.md section 7m.  The box is the matrix ``A`` ``[3, 3]``
whose rows are the lattice vectors (``None``: the unit cube), the positions are FRACTIONAL, ``x = s A``, ``kappa = A^-1 k``,
``V = det A``; the Cartesian forces ``f`` are ``[n, 3, *cols]``.  Every function returns ``(u [n, 3, *cols], G [n, 3, 3, *cols] or
None)``, ``G_ab = d u_a / d x_b`` at ``order = 2``.

``weights``          ``B_0 - g``, ``B_1``, ``2 alpha^2 g - B_1`` and ``B_2`` of the distances r
``near``             the pair sums over the wrapped minimum image with ``0 < r < r_c``
``near_f32``         the same image and weights in numpy float32 arithmetic: what float32 does to these points
``far``              the dense sum over ``k in [-N/2, N/2)^3``, the unpaired planes ``k_a = -N/2`` zeroed (``kmax``: over
                     ``|k|_inf <= kmax`` instead)
``terms``            the self term
``exact_algorithm``  near + far + terms: the algorithm in exact arithmetic
``converged``        the sum at a second ``alpha`` with wide cutoffs: 5^3 images without a cut, ``|k|_inf <= 14``
``power``            ``P = 1/2 sum f . u`` per point set
``spectral_table``   what the spectral kernel multiplies with, in the transforms' sign convention
"""
import itertools
import math

import numpy as np

from dipole_ref import _box, _sets, erfc, near_gate, near_points  # noqa: F401  (the points and the gate of the dipole tests)
from dispersion_ref import kappa


def _forces(f, n, dtype=np.float64):
    """(f [n, 3, C], cols)"""
    cols = tuple(np.shape(f)[2:])
    return np.asarray(f, dtype=dtype).reshape(n, 3, int(np.prod(cols, dtype=np.int64))), cols


def _shaped(u, G, cols, order):
    n = u.shape[0]
    return u.reshape((n, 3) + cols), G.reshape((n, 3, 3) + cols) if order == 2 else None


def weights(r, alpha, minus_g=True):
    """(B_0 - g, B_1, 2 alpha^2 g - B_1, B_2) of r > 0 in the arithmetic of r: B_0 = erfc(alpha r) / r, g = (2 alpha / sqrt(pi))
    e^(-alpha^2 r^2), B_1 = (B_0 + g) / r^2, B_2 = (3 B_1 + 2 alpha^2 g) / r^2.  minus_g=False: the mistake of weighing f with B_0
    alone"""
    one = r.dtype.type
    g = one(2.0 * alpha / math.sqrt(math.pi)) * np.exp(-(one(alpha) * r) ** 2)
    B0 = erfc(one(alpha) * r) / r
    B1 = (B0 + g) / (r * r)
    g2 = one(2.0 * alpha * alpha) * g
    return (B0 - g if minus_g else B0), B1, g2 - B1, (one(3) * B1 + g2) / (r * r)


def _pair_sums(d, ok, fs, alpha, order, minus_g=True, mdelta=True, b2=True):
    """the sums of one block of rows: d [rows, n, 3] (Cartesian), ok [rows, n], forces fs [n, 3, C]"""
    r = np.sqrt((d * d).sum(-1))
    a, B1, c, B2 = (np.where(ok, w, 0) for w in weights(np.where(ok, r, 1).astype(d.dtype), alpha, minus_g))
    rows, n, C = d.shape[0], d.shape[1], fs.shape[2]
    flat = fs.reshape(n, 3 * C)
    m = sum(d[..., e, None] * fs[None, :, e, :] for e in range(3))  # d . f_j: [rows, n, C]
    dt = d.transpose(0, 2, 1)  # [rows, 3, n]
    u = (a @ flat).reshape(rows, 3, C) + dt @ (B1[..., None] * m)
    if order != 2:
        return u, None
    eye = np.eye(3, dtype=d.dtype)
    # (2 alpha^2 g - B_1) f_a d_b: [rows, a, b, C]
    G = np.stack([((c * d[..., b]) @ flat).reshape(rows, 3, C) for b in range(3)], 2)
    # B_1 d_a f_b
    G = G + np.stack([((B1 * d[..., e]) @ flat).reshape(rows, 3, C) for e in range(3)], 1)
    if mdelta:  # B_1 m delta_ab
        G = G + eye[None, :, :, None] * (B1[..., None] * m).sum(1)[:, None, None, :]
    if b2:  # - B_2 m d_a d_b
        ddt = (d[..., :, None] * d[..., None, :]).reshape(rows, n, 9).transpose(0, 2, 1)  # [rows, 9, n]
        G = G - (ddt @ (B2[..., None] * m)).reshape(rows, 3, 3, C)
    return u, G


def near(f, s, A, batch, alpha, r_c, order=2, nimg=0, wrap=True, **mistakes):
    """the pair sums over d = (ds - rint(ds)) A with 0 < |d| < r_c (r_c = None with nimg = 2: every image within two cells, no
    cut).  The mistakes of the sensitivity test: wrap=False, minus_g=False (the -g term dropped), mdelta=False (the m delta_ab
    term dropped), b2=False (the B_2 term dropped)."""
    s = np.asarray(s, dtype=np.float64)
    n = s.shape[0]
    A = _box(A)
    fs, cols = _forces(f, n)
    C = fs.shape[2]
    u, G = np.zeros((n, 3, C)), np.zeros((n, 3, 3, C))
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
                uu, gg = _pair_sums(d, ok, fs[sel], alpha, order, **mistakes)
                u[rows] += uu
                if order == 2:
                    G[rows] += gg
    return _shaped(u, G, cols, order)


def near_f32(f, s, A, batch, alpha, r_c, order=2):
    """``near`` in numpy float32 arithmetic: the positions reduced to [-1/2, 1/2), their differences wrapped and multiplied
    with the float32 box, r^2 compared with the float32 r_c^2, the weights and every product and sum in float32 (erfc and exp
    as torch and numpy round them in float32).  Not the device's bits: the same number format on the same points."""
    t = np.float32
    s = np.asarray(s, dtype=t)
    s = s - np.rint(s)
    n = s.shape[0]
    A = _box(A).astype(t)
    fs, cols = _forces(f, n, t)
    C = fs.shape[2]
    u, G = np.zeros((n, 3, C), t), np.zeros((n, 3, 3, C), t)
    rc2 = t(r_c * r_c)
    for sel in _sets(batch, n):
        for r0 in range(0, sel.size, 256):
            rows = sel[r0:r0 + 256]
            ds = s[rows][:, None, :] - s[sel][None, :, :]
            ds = ds - np.rint(ds)
            d = np.stack([ds[..., 0] * A[0, 0] + ds[..., 1] * A[1, 0] + ds[..., 2] * A[2, 0],
                          ds[..., 1] * A[1, 1] + ds[..., 2] * A[2, 1], ds[..., 2] * A[2, 2]], -1)
            rr = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
            ok = (rr > 0) & (rr < rc2)
            uu, gg = _pair_sums(d, ok, fs[sel], alpha, order)
            assert uu.dtype == t
            u[rows] = uu
            if order == 2:
                assert gg.dtype == t
                G[rows] = gg
    return _shaped(u, G, cols, order)


def coeffs(A, alpha, N=None, kmax=None):
    """(K [nk, 3] integer frequencies, kappa [nk, 3], c [nk]): c_k = 2 exp(-x) (1 + x) / (pi V |kappa|^2), x = pi^2 |kappa|^2 / alpha^2,
    on [-N/2, N/2)^3 without k = 0 and the unpaired planes k_a = -N/2, or on 0 < |k|_inf <= kmax"""
    if kmax is None:
        K, kap = kappa(A, N)
        keep = (K > -(N // 2)).all(-1) & (K != 0).any(-1)
    else:
        K, kap = kappa(A, 2 * kmax + 2)
        keep = (np.abs(K) <= kmax).all(-1) & (K != 0).any(-1)
    K, kap = K[keep], kap[keep]
    k2 = (kap * kap).sum(-1)
    x = math.pi ** 2 * k2 / alpha ** 2
    V = abs(np.linalg.det(_box(A)))
    return K, kap, 2.0 * np.exp(-x) * (1.0 + x) / (math.pi * V * k2)


def far(f, s, A, batch, alpha, N=None, order=2, kmax=None, chunk=4096):
    """u = sum_k c_k (I - kappa kappa^T / |kappa|^2) rho_k e^{2 pi i k.s}, rho_k = sum_j f_j e^{-2 pi i k.s_j}; G_ab with the
    further factor 2 pi i kappa_b"""
    s = np.asarray(s, dtype=np.float64)
    n = s.shape[0]
    fs, cols = _forces(f, n)
    C = fs.shape[2]
    K, kap, c = coeffs(A, alpha, N, kmax)
    u, G = np.zeros((n, 3, C)), np.zeros((n, 3, 3, C))
    for sel in _sets(batch, n):
        if sel.size == 0:
            continue
        for c0 in range(0, K.shape[0], chunk):
            Kc, kc, cc = K[c0:c0 + chunk], kap[c0:c0 + chunk], c[c0:c0 + chunk]
            ph = np.exp(2j * math.pi * s[sel] @ Kc.T)  # [n, nk]: e^{+2 pi i k.s_i}
            nk = Kc.shape[0]
            rho = (np.conj(ph).T @ fs[sel].reshape(sel.size, 3 * C)).reshape(nk, 3, C)
            along = (kc[:, :, None] * rho).sum(1) / (kc * kc).sum(-1)[:, None]  # kappa . rho / |kappa|^2
            U = cc[:, None, None] * (rho - kc[:, :, None] * along[:, None, :])  # [nk, 3, C]
            u[sel] += (ph @ U.reshape(nk, 3 * C)).real.reshape(sel.size, 3, C)
            if order == 2:
                W = 2j * math.pi * U[:, :, None, :] * kc[:, None, :, None]  # [nk, a, b, C]
                G[sel] += (ph @ W.reshape(nk, 9 * C)).real.reshape(sel.size, 3, 3, C)
    return _shaped(u, G, cols, order)


def terms(f, n, alpha, order=2):
    """the self term: -(4 alpha / sqrt(pi)) f_i in u, nothing in G"""
    fs, cols = _forces(f, n)
    return _shaped(-4.0 * alpha / math.sqrt(math.pi) * fs, np.zeros((n, 3, 3, fs.shape[2])), cols, order)


def _add(*parts):
    return tuple(None if p[0] is None else sum(p) for p in zip(*parts))


def exact_algorithm(f, s, A, batch, alpha, r_c, N, order=2):
    """the algorithm in exact arithmetic: near + far over [-N/2, N/2)^3 + the self term"""
    return _add(near(f, s, A, batch, alpha, r_c, order), far(f, s, A, batch, alpha, N, order),
                terms(f, np.shape(s)[0], alpha, order))


def converged(f, s, A, batch=None, alpha=6.0, order=2, nimg=2, kmax=14):
    """the sum carried to convergence at a splitting of its own: 5^3 images without a cut, |k|_inf <= 14"""
    return _add(near(f, s, A, batch, alpha, None, order, nimg=nimg), far(f, s, A, batch, alpha, None, order, kmax=kmax),
                terms(f, np.shape(s)[0], alpha, order))


def power(f, u, batch=None):
    """P_b = 1/2 sum_{i in set b} f_i . u_i: [B, *cols]"""
    w = (np.asarray(f, dtype=np.float64) * u).sum(1)
    return np.stack([0.5 * w[sel].sum(0) for sel in _sets(batch, w.shape[0])])


def position_gradient(f, g, Gf, Gg):
    """dL/dx_i,b of L = sum_i g_i . u_i[f] from G[f] and G[g]: sum over the columns and a of g_i,a G[f]_i,ab + f_i,a G[g]_i,ab:
    [n, 3]"""
    f, g = np.asarray(f, dtype=np.float64), np.asarray(g, dtype=np.float64)
    w = (g[:, :, None] * Gf + f[:, :, None] * Gg).sum(1)  # [n, 3 (b), *cols]
    return w.reshape(w.shape[0], 3, -1).sum(2)


def spectral_table(A, alpha, N, order=2):
    """[N, N, N, 3 or 12, 3] complex128: what turns the adjoint transform of the forces into the spectra of (u, G) in the sign
    convention of the transforms (the adjoint sums e^{+2 pi i k.s}, the forward e^{-2 pi i k.s}: k -> -k against ``far``): row a
    is c_k (delta_ar - kappa_a kappa_r / |kappa|^2), row 3 + 3 a + b is -2 pi i kappa_b times row a; c_0 = 0 and the unpaired
    planes zeroed"""
    K, kap = kappa(A, N)
    k2 = (kap * kap).sum(-1)
    safe = np.where(k2 > 0, k2, 1.0)
    x = math.pi ** 2 * k2 / alpha ** 2
    V = abs(np.linalg.det(_box(A)))
    c = 2.0 * np.exp(-x) * (1.0 + x) / (math.pi * V * safe)
    c[~((K > -(N // 2)).all(-1) & (K != 0).any(-1))] = 0.0
    P = c[..., None, None] * (np.eye(3) - kap[..., :, None] * kap[..., None, :] / safe[..., None, None])  # [N, N, N, 3, 3]
    rows = [P.astype(np.complex128)]
    if order == 2:
        rows.append((-2j * math.pi * P[..., :, None, :] * kap[..., None, :, None]).reshape(N, N, N, 9, 3))
    return np.concatenate(rows, 3)


def near_forces(seed, n, cols):
    """signed forces [n, 3, *cols] float32 from a seeded normal distribution"""
    return np.random.default_rng(seed).standard_normal((n, 3) + cols).astype(np.float32)
