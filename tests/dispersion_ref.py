"""Float64 restatement of the Ewald sum for the periodic 1/r^6 (the dispersion sum) -- TEST INFRASTRUCTURE ONLY.

Written independently of ``torch_nfft_amd/dispersion.py``, dense numpy in float64 (``torch.special.erfc`` for erfc, as in
``tests/ewald_ref.py``).  The box is the matrix ``A`` ``[3, 3]`` whose rows are the lattice vectors (``None``: the unit cube),
the positions are FRACTIONAL, ``x = s A``, ``kappa = A^-1 k``, ``V = det A``; with ``a = alpha r`` and ``b = pi |kappa| / alpha``:

``lattice_sum``            brute force: every image with ``0 < |d| < R`` plus the continuum tail ``4 pi sum(c) / (3 V R^3)``
``near_sum`` / ``near_field``  the pair sums over the wrapped minimum image with ``0 < r < r_c`` (duplicates skipped), weights
                           ``w = e^(-a^2) (1 + a^2 + a^4/2) / r^6`` and ``mg = -w'/r = e^(-a^2) (6 + 6a^2 + 3a^4 + a^6) / r^8``
``coeffs``                 ``b_k = pi^(3/2) alpha^3 f(b) / (3 V)``, ``f(b) = (1 - 2b^2) e^(-b^2) + 2 sqrt(pi) b^3 erfc(b)``, on
                           ``[-N/2, N/2)^3``, ``b_0`` kept, the unpaired planes ``k_a = -N/2`` zeroed
``far_sum`` / ``far_field``    the direct sum over those frequencies
``dispersion``             near + far - (alpha^6 / 6) c: the algorithm in exact arithmetic, per point set
"""
import itertools
import math

import numpy as np
import torch


def erfc(a):
    return torch.special.erfc(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))).numpy()


def _box(A):
    return np.eye(3) if A is None else np.asarray(A, dtype=np.float64)


def _columns(c):
    c = np.asarray(c)
    return c.reshape(c.shape[0], -1).astype(np.complex128 if np.iscomplexobj(c) else np.float64)


def _sets(batch, n):
    if batch is None:
        return [np.arange(n)]
    batch = np.asarray(batch)
    return [np.nonzero(batch == b)[0] for b in range(int(batch.max()) + 1 if batch.size else 0)]


def _shaped(c0, z, f):
    return z.reshape(c0.shape), f.reshape((c0.shape[0], 3) + c0.shape[1:])


def lattice_sum(c, s, A, R, batch=None):
    """(psi [n, *cols], G = -grad_x psi [n, 3, *cols]): sum of c_j / |d|^6 over all pairs and images with 0 < |d| < R, plus
    the tail of a uniform density sum(c) / V beyond R (which has no field)"""
    c0 = np.asarray(c)
    s = np.asarray(s, dtype=np.float64)
    A = _box(A)
    V = abs(np.linalg.det(A))
    cc = _columns(c0)
    psi = np.zeros_like(cc)
    G = np.zeros((cc.shape[0], 3, cc.shape[1]), dtype=cc.dtype)
    w = 1.0 / np.linalg.norm(np.linalg.inv(A), axis=0)  # perpendicular widths
    reach = [int(math.ceil(R / w[a])) + 1 for a in range(3)]
    shifts = np.array(list(itertools.product(*(range(-m, m + 1) for m in reach))), dtype=np.float64)
    # (a wrapped difference is shorter than the cell's diagonal: images further than R + that are out of reach)
    shifts = shifts[np.linalg.norm(shifts @ A, axis=1) < R + np.linalg.norm(np.abs(A).sum(0))]
    for sel in _sets(batch, s.shape[0]):
        if sel.size == 0:
            continue
        ds = s[sel][:, None, :] - s[sel][None, :, :]
        ds = ds - np.rint(ds)
        p = np.zeros_like(cc[sel])
        g = np.zeros((sel.size, 3, cc.shape[1]), dtype=cc.dtype)
        step = max(1, 200000 // (sel.size * sel.size))
        for m0 in range(0, shifts.shape[0], step):
            d = (ds[None] + shifts[m0:m0 + step, None, None, :]) @ A  # [images, n, n, 3]
            rr = (d * d).sum(-1)
            ok = (rr > 0) & (rr < R * R)
            ir2 = np.where(ok, 1.0 / np.where(ok, rr, 1.0), 0.0)
            p += (ir2 ** 3).sum(0) @ cc[sel]
            g += np.einsum("ija,jc->iac", (6.0 * (ir2 ** 4)[..., None] * d).sum(0), cc[sel])
        psi[sel] = p + 4.0 * math.pi * cc[sel].sum(0, keepdims=True) / (3.0 * V * R ** 3)
        G[sel] = g
    return _shaped(c0, psi, G)


def pair_weights(d, alpha, r_c=None, top_term=True):
    """(w, mg) for the difference vectors d [.., 3]; zero where r = 0 or r >= r_c.  top_term=False drops a^4/2 from w and
    a^6 from mg (a mistake for the sensitivity test)."""
    rr = (d * d).sum(-1)
    ok = rr > 0 if r_c is None else (rr > 0) & (rr < r_c * r_c)
    rs = np.where(ok, rr, 1.0)
    a2 = alpha * alpha * rs
    e = np.exp(-a2)
    top = 1.0 if top_term else 0.0
    w = e * (1.0 + a2 + top * a2 ** 2 / 2.0) / rs ** 3
    mg = e * (6.0 + 6.0 * a2 + 3.0 * a2 ** 2 + top * a2 ** 3) / rs ** 4
    return np.where(ok, w, 0.0), np.where(ok, mg, 0.0)


def _near(c, s, A, batch, alpha, r_c, nimg=0, wrap=True, top_term=True):
    c0 = np.asarray(c)
    s = np.asarray(s, dtype=np.float64)
    A = _box(A)
    cc = _columns(c0)
    z = np.zeros_like(cc)
    f = np.zeros((cc.shape[0], 3, cc.shape[1]), dtype=cc.dtype)
    for sel in _sets(batch, s.shape[0]):
        if sel.size == 0:
            continue
        for r0 in range(0, sel.size, 512):  # (rows in blocks: the pair arrays stay small)
            rows = sel[r0:r0 + 512]
            ds = s[rows][:, None, :] - s[sel][None, :, :]
            if wrap:
                ds = ds - np.rint(ds)
            for sh in itertools.product(range(-nimg, nimg + 1), repeat=3):
                d = (ds + np.array(sh, dtype=np.float64)) @ A
                w, mg = pair_weights(d, alpha, r_c, top_term)
                z[rows] += w @ cc[sel]
                f[rows] += np.einsum("ija,jc->iac", mg[..., None] * d, cc[sel])
    return _shaped(c0, z, f)


def jittered_lattice(rng, m, spacing, jitter, centre=0.0):
    """m^3 float32 points on a cubic lattice of the given spacing around `centre`, each coordinate moved by at most
    `jitter`: [m, m, m, 3] (no two closer than spacing - 2 jitter)"""
    g = (np.arange(m) + 0.5 - m / 2.0) * spacing + centre
    x = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1)
    return (x + (rng.random((m, m, m, 3)) * 2.0 - 1.0) * jitter).astype(np.float32)


def min_separation(s, A=None):
    """the smallest non-zero wrapped distance of the set"""
    s = np.asarray(s, dtype=np.float64)
    best = np.inf
    for r0 in range(0, s.shape[0], 512):
        ds = s[r0:r0 + 512, None, :] - s[None, :, :]
        d = (ds - np.rint(ds)) @ _box(A)
        rr = (d * d).sum(-1)
        best = min(best, np.sqrt(rr[rr > 0].min()))
    return best


def near_sum(c, s, A, batch, alpha, r_c, **kw):
    """z_i = sum_{j: 0 < r_ij < r_c, same set} w(r_ij) c_j, r_ij = |(ds - rint(ds)) A|.  r_c=None with nimg=2: every image
    within two cells, no cut."""
    return _near(c, s, A, batch, alpha, r_c, **kw)[0]


def near_field(c, s, A, batch, alpha, r_c, **kw):
    """f_i = sum_j mg(r_ij) d_ij c_j (Cartesian; minus the gradient of near_sum): [n, 3, *cols]"""
    return _near(c, s, A, batch, alpha, r_c, **kw)[1]


def far_factor(b):
    """f(b), clamped at 0"""
    b = np.asarray(b, dtype=np.float64)
    return np.maximum((1.0 - 2.0 * b * b) * np.exp(-b * b) + 2.0 * math.sqrt(math.pi) * b ** 3 * erfc(b), 0.0)


def pair_factor(a):
    """e^(-a^2) (1 + a^2 + a^4 / 2)"""
    return math.exp(-a * a) * (1.0 + a * a + a ** 4 / 2.0)


def kappa(A, N):
    k = np.arange(-(N // 2), N // 2, dtype=np.float64)
    K = np.stack(np.meshgrid(k, k, k, indexing="ij"), -1)  # [N, N, N, 3]
    return K, K @ np.linalg.inv(_box(A)).T  # kappa_b = sum_a (A^-1)_ba k_a


def coeffs(A, alpha, N):
    _, kap = kappa(A, N)
    V = abs(np.linalg.det(_box(A)))
    b = math.pi ** 1.5 * alpha ** 3 / (3.0 * V) * far_factor(math.pi * np.sqrt((kap * kap).sum(-1)) / alpha)
    b[0, :, :] = 0.0
    b[:, 0, :] = 0.0
    b[:, :, 0] = 0.0
    return b


def _far(c, s, A, batch, alpha, N, chunk=4096):
    c0 = np.asarray(c)
    s = np.asarray(s, dtype=np.float64)
    cc = _columns(c0)
    real = not np.iscomplexobj(cc)
    K, kap = kappa(A, N)
    b = coeffs(A, alpha, N).reshape(-1)
    K, kap = K.reshape(-1, 3)[b != 0], kap.reshape(-1, 3)[b != 0]
    b = b[b != 0]
    z = np.zeros_like(cc)
    f = np.zeros((cc.shape[0], 3, cc.shape[1]), dtype=cc.dtype)
    for sel in _sets(batch, s.shape[0]):
        if sel.size == 0:
            continue
        p = np.zeros((sel.size, cc.shape[1]), dtype=np.complex128)
        g = np.zeros((sel.size, 3, cc.shape[1]), dtype=np.complex128)
        for c0_ in range(0, K.shape[0], chunk):
            Kc, kc, bc = K[c0_:c0_ + chunk], kap[c0_:c0_ + chunk], b[c0_:c0_ + chunk]
            ph = np.exp(2j * math.pi * s[sel] @ Kc.T)      # [n, nk]: e^{+2 pi i k.s_i}
            Sk = (np.conj(ph).T @ cc[sel]) * bc[:, None]   # b_k sum_j c_j e^{-2 pi i k.s_j}
            p += ph @ Sk
            g -= np.einsum("ik,ka,kc->iac", ph, 2j * math.pi * kc, Sk)
        z[sel] = p.real if real else p
        f[sel] = g.real if real else g
    return _shaped(c0, z, f)


def far_sum(c, s, A, batch, alpha, N):
    """sum_k b_k e^{2 pi i k.s_i} sum_j c_j e^{-2 pi i k.s_j} over k in [-N/2, N/2)^3, the unpaired planes zeroed"""
    return _far(c, s, A, batch, alpha, N)[0]


def far_field(c, s, A, batch, alpha, N):
    """minus the Cartesian gradient of far_sum: [n, 3, *cols]"""
    return _far(c, s, A, batch, alpha, N)[1]


def dispersion(c, s, A, batch, alpha, r_c, N, nimg=0):
    """(psi, G) of the split sum in exact arithmetic: near + far - (alpha^6 / 6) c"""
    c0 = np.asarray(c)
    z, f = _near(c0, s, A, batch, alpha, r_c, nimg=nimg)
    zf, ff = _far(c0, s, A, batch, alpha, N)
    self_term = alpha ** 6 / 6.0 * _columns(c0).reshape(c0.shape)
    return z + zf - self_term, f + ff
