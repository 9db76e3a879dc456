"""Float64 restatement of the periodic Rotne-Prager-Yamakawa sum (the Ewald sum of Beenakker) -- TEST INFRASTRUCTURE ONLY.

Written independently of ``torch_nfft_amd/rpy.py`` and of the kernel, dense numpy in float64, straight from the formulas of
DESIGN.md section 7n, in the style and with the conventions of ``tests/stokeslet_ref.py``: the box is the matrix ``A`` ``[3, 3]``
whose rows are the lattice vectors (``None``: the unit cube), the positions are FRACTIONAL, the Cartesian forces ``f`` are
``[n, 3, *cols]``, ``a`` is the sphere radius.  Every function returns ``(u [n, 3, *cols], G [n, 3, 3, *cols] or None)``,
``G_ab = d u_a / d x_b`` at ``order = 2``.

``weights``            ``W1, W2, D1, D2`` of the distances r, the overlap branch ``r < 2 a`` included
``near``               the pair sums over the wrapped minimum image with ``0 < r < r_c``
``near_f32``           the same image and the weights as the kernel forms them, in numpy float32 arithmetic
``far``                the dense sum over ``k in [-N/2, N/2)^3`` with ``c_k (1 - a^2 |tau|^2 / 3)`` (``kmax``: over ``|k|_inf <= kmax``)
``terms``              the self term
``exact_algorithm``    near + far + terms: the algorithm in exact arithmetic
``converged``          the sum at a second ``alpha`` with wide cutoffs: 5^3 images without a cut, ``|k|_inf <= 14``
``mobility``           the ``3 n x 3 n`` matrix of the converged sum
``spectral_table``     what the spectral kernel multiplies with, in the transforms' sign convention
``dimers``             256 pairs of spheres from deep overlap to beyond contact
``position_gradient``, ``power``, ``near_points``, ``near_forces``, ``near_gate``: those of ``stokeslet_ref``
"""
import itertools
import math

import numpy as np

import stokeslet_ref as sr
from stokeslet_ref import _add, _box, _forces, _sets, _shaped, erfc
from stokeslet_ref import near_forces, near_gate, near_points, position_gradient, power  # noqa: F401

FORMS = ("direct", "far")  # how the overlap branch is written, see weights; the kernel uses "far"


def weights(r, alpha, a, overlap=True, a2_term=True, form="direct"):
    """(W1, W2, D1, D2) of r > 0 in the arithmetic of r.  With B_0 = erfc(alpha r) / r, g = (2 alpha / sqrt(pi)) e^(-alpha^2 r^2),
    B_l = ((2l - 1) B_(l-1) + (2 alpha^2)^(l-1) g) / r^2 and q = a^2 / 3:

        W1 = (B_0 - g) + q (2 B_1 + (8 alpha^2 - 4 alpha^4 r^2) g)          W2 = B_1 + q (4 alpha^4 g - 2 B_2)
        D1 = (2 alpha^2 g - B_1) + q (-2 B_2 + (8 alpha^6 r^2 - 24 alpha^4) g)    D2 = -B_2 + q (2 B_3 - 8 alpha^6 g)

    and for r < 2 a the difference of the overlap form and the unscreened tensor.  form="direct" adds that difference as the
    powers of 1 / r it is; form="far" writes the weight as the overlap form minus the far kernel, whose Smith functions
    E_0 = (1 - erfc(alpha r)) / r, E_l = ((2l - 1) E_(l-1) - (2 alpha^2)^(l-1) g) / r^2 stand for (2l - 1)!! / r^(2l+1) - B_l.  The two
    are the same numbers in exact arithmetic.  The mistakes of the sensitivity test: overlap=False (no branch), a2_term=False
    (the a^2 term of W2 and D2 dropped)."""
    one = r.dtype.type
    rr = r * r
    ir = one(1) / r
    ir2 = ir * ir
    two_alpha2 = one(2.0 * alpha * alpha)
    g = one(2.0 * alpha / math.sqrt(math.pi)) * np.exp(-(one(alpha) * r) ** 2)
    g2 = two_alpha2 * g
    g4 = two_alpha2 * g2
    g6 = two_alpha2 * g4
    q = one(a * a / 3.0)
    q2 = q if a2_term else one(0)
    ec = erfc(one(alpha) * r)
    B0 = ec * ir
    B1 = (B0 + g) * ir2
    B2 = (one(3) * B1 + g2) * ir2
    B3 = (one(5) * B2 + g4) * ir2
    W1 = (B0 - g) + q * (one(2) * B1 + (one(4) * g2 - g4 * rr))
    W2 = B1 + q2 * (g4 - one(2) * B2)
    D1 = (g2 - B1) + q * ((g6 * rr - one(6) * g4) - one(2) * B2)
    D2 = q2 * (one(2) * B3 - g6) - B2
    if not overlap:
        return W1, W2, D1, D2
    ov = rr < one(4.0 * a * a)
    h = one(1.0 / (8.0 * a * a))
    lead = one(4.0 / (3.0 * a))
    if form == "direct":
        ir3 = ir * ir2
        ir5 = ir3 * ir2
        ir7 = ir5 * ir2
        o1 = (lead - one(3) * h * r) - (ir + one(2) * q * ir3)
        o2 = h * ir - (ir3 - one(6) * q * ir5)
        p1 = (ir3 + one(6) * q * ir5) - one(3) * h * ir
        p2 = (one(3) * ir5 - one(30) * q * ir7) - h * ir3
        return tuple(np.where(ov, w + o, w) for w, o in zip((W1, W2, D1, D2), (o1, o2, p1, p2)))
    assert form == "far"
    E0 = (one(1) - ec) * ir
    E1 = (E0 - g) * ir2
    E2 = (one(3) * E1 - g2) * ir2
    E3 = (one(5) * E2 - g4) * ir2
    V1 = (lead - one(3) * h * r) - ((E0 + g) + q * (one(2) * E1 - (one(4) * g2 - g4 * rr)))
    V2 = h * ir - (E1 - q * (one(2) * E2 + g4))
    C1 = (E1 + g2) + q * (one(2) * E2 + (g6 * rr - one(6) * g4)) - one(3) * h * ir
    C2 = (E2 - q * (one(2) * E3 + g6)) - h * ir * ir2
    return tuple(np.where(ov, v, w) for w, v in zip((W1, W2, D1, D2), (V1, V2, C1, C2)))


def _pair_sums(d, ok, fs, alpha, a, order, **kw):
    """the sums of one block of rows: d [rows, n, 3] (Cartesian), ok [rows, n], forces fs [n, 3, C]:
    u_a += W1 f_a + W2 m d_a,   G_ab += D1 f_a d_b + D2 m d_a d_b + W2 (m delta_ab + d_a f_b)"""
    r = np.sqrt((d * d).sum(-1))
    W1, W2, D1, D2 = (np.where(ok, w, 0) for w in weights(np.where(ok, r, 1).astype(d.dtype), alpha, a, **kw))
    rows, n, C = d.shape[0], d.shape[1], fs.shape[2]
    flat = fs.reshape(n, 3 * C)
    m = sum(d[..., e, None] * fs[None, :, e, :] for e in range(3))  # d . f_j: [rows, n, C]
    dt = d.transpose(0, 2, 1)  # [rows, 3, n]
    u = (W1 @ flat).reshape(rows, 3, C) + dt @ (W2[..., None] * m)
    if order != 2:
        return u, None
    eye = np.eye(3, dtype=d.dtype)
    G = np.stack([((D1 * d[..., b]) @ flat).reshape(rows, 3, C) for b in range(3)], 2)  # D1 f_a d_b: [rows, a, b, C]
    G = G + np.stack([((W2 * d[..., e]) @ flat).reshape(rows, 3, C) for e in range(3)], 1)  # W2 d_a f_b
    G = G + eye[None, :, :, None] * (W2[..., None] * m).sum(1)[:, None, None, :]  # W2 m delta_ab
    ddt = (d[..., :, None] * d[..., None, :]).reshape(rows, n, 9).transpose(0, 2, 1)  # [rows, 9, n]
    G = G + (ddt @ (D2[..., None] * m)).reshape(rows, 3, 3, C)  # D2 m d_a d_b
    return u, G


def near(f, s, A, batch, alpha, r_c, a, order=2, nimg=0, wrap=True, **mistakes):
    """the pair sums over d = (ds - rint(ds)) A with 0 < |d| < r_c (r_c = None with nimg = 2: every image within two cells, no
    cut; the overlap branch belongs to the minimum image alone, 2 a is below every other image's distance).  The mistakes of
    the sensitivity test: wrap=False, and overlap=False, a2_term=False of ``weights``."""
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
                uu, gg = _pair_sums(d, ok, fs[sel], alpha, a, order, **mistakes)
                u[rows] += uu
                if order == 2:
                    G[rows] += gg
    return _shaped(u, G, cols, order)


def near_f32(f, s, A, batch, alpha, r_c, a, order=2, form="far"):
    """``near`` in numpy float32 arithmetic, as ``stokeslet_ref.near_f32``: the positions reduced to [-1/2, 1/2), their
    differences wrapped and multiplied with the float32 box, r^2 compared with the float32 r_c^2 and (2 a)^2, the weights in the
    form the kernel uses and every product and sum in float32.  Not the device's bits: the same number format on the same
    points."""
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
            uu, gg = _pair_sums(d, ok, fs[sel], alpha, a, order, form=form)
            assert uu.dtype == t
            u[rows] = uu
            if order == 2:
                assert gg.dtype == t
                G[rows] = gg
    return _shaped(u, G, cols, order)


def coeffs(A, alpha, a, N=None, kmax=None):
    """(K, kappa, c) of ``stokeslet_ref.coeffs`` with c_k (1 - a^2 |tau|^2 / 3), tau = 2 pi kappa"""
    K, kap, c = sr.coeffs(A, alpha, N, kmax)
    return K, kap, c * (1.0 - a * a / 3.0 * 4.0 * math.pi ** 2 * (kap * kap).sum(-1))


def far(f, s, A, batch, alpha, a, N=None, order=2, kmax=None, chunk=4096):
    """u = sum_k c_k (1 - a^2 |tau|^2 / 3) (I - kappa kappa^T / |kappa|^2) rho_k e^{2 pi i k.s}, rho_k = sum_j f_j e^{-2 pi i k.s_j};
    G_ab with the further factor 2 pi i kappa_b"""
    s = np.asarray(s, dtype=np.float64)
    n = s.shape[0]
    fs, cols = _forces(f, n)
    C = fs.shape[2]
    K, kap, c = coeffs(A, alpha, a, N, kmax)
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


def self_coefficient(alpha, a, a2_term=True):
    """4 / (3 a) - 4 alpha / sqrt(pi) + 40 a^2 alpha^3 / (9 sqrt(pi)): the sphere's own mobility less what the far sum holds of
    it.  a2_term=False: the mistake of keeping the Stokeslet's self term beside 4 / (3 a)."""
    c = 4.0 / (3.0 * a) - 4.0 * alpha / math.sqrt(math.pi)
    return c + 40.0 * a * a * alpha ** 3 / (9.0 * math.sqrt(math.pi)) if a2_term else c


def terms(f, n, alpha, a, order=2, a2_term=True):
    """the self term: self_coefficient f_i in u, nothing in G"""
    fs, cols = _forces(f, n)
    return _shaped(self_coefficient(alpha, a, a2_term) * fs, np.zeros((n, 3, 3, fs.shape[2])), cols, order)


def exact_algorithm(f, s, A, batch, alpha, r_c, N, a, order=2):
    """the algorithm in exact arithmetic: near + far over [-N/2, N/2)^3 + the self term"""
    return _add(near(f, s, A, batch, alpha, r_c, a, order), far(f, s, A, batch, alpha, a, N, order),
                terms(f, np.shape(s)[0], alpha, a, order))


def converged(f, s, A, a, batch=None, alpha=6.0, order=2, nimg=2, kmax=14):
    """the sum carried to convergence at a splitting of its own: 5^3 images without a cut, |k|_inf <= 14"""
    return _add(near(f, s, A, batch, alpha, None, a, order, nimg=nimg), far(f, s, A, batch, alpha, a, None, order, kmax=kmax),
                terms(f, np.shape(s)[0], alpha, a, order))


def mobility(s, A, a, **kw):
    """[3 n, 3 n]: column 3 j + b is the velocity of all spheres for the unit force e_b on sphere j (the converged sum)"""
    n = np.shape(s)[0]
    f = np.eye(3 * n).reshape(n, 3, 3 * n)
    return converged(f, s, A, a, order=1, **kw)[0].reshape(3 * n, 3 * n)


def spectral_table(A, alpha, N, a, order=2):
    """``stokeslet_ref.spectral_table`` with every row times 1 - a^2 |tau|^2 / 3: [N, N, N, 3 or 12, 3] complex128"""
    _, kap = sr.kappa(A, N)
    factor = 1.0 - a * a / 3.0 * 4.0 * math.pi ** 2 * (kap * kap).sum(-1)
    return sr.spectral_table(A, alpha, N, order) * factor[..., None, None]


def dimers(A=None, radius=0.02, seed=11):
    """256 dimers (512 fractional float32 points, the partners interleaved) on a jittered 8 x 8 x 4 lattice of centres, their
    separations spread uniformly over [a / 2, 2.5 a] (in the metric of the box A) in random directions: each pair's
    contribution dominates its two points.  (points, Cartesian separations)"""
    rng = np.random.default_rng(seed)
    g = [(np.arange(m) + 0.5) / m - 0.5 for m in (8, 8, 4)]
    c = np.stack(np.meshgrid(*g, indexing="ij"), -1).reshape(-1, 3)
    c = c + (rng.random(c.shape) * 2.0 - 1.0) * 0.02
    sep = rng.permutation(np.linspace(0.5 * radius, 2.5 * radius, 256))
    e = rng.standard_normal((256, 3))
    half = 0.5 * sep[:, None] * e / np.linalg.norm(e, axis=1, keepdims=True) @ np.linalg.inv(_box(A))
    x = np.stack([c - half, c + half], 1).reshape(512, 3).astype(np.float32)
    ds = x[0::2].astype(np.float64) - x[1::2]
    return x, np.linalg.norm((ds - np.rint(ds)) @ _box(A), axis=1)
