"""Float64 restatement of the Ewald sum for the periodic 1/r in the unit box -- TEST INFRASTRUCTURE ONLY.

Written independently of ``torch_nfft_amd/ewald.py``, dense and in float64 (``torch.special.erfc`` for erfc):

``converged``        the Ewald sum carried to convergence (images ``|n|_inf <= 2``, ``|k|_inf <= 14``, ``alpha = 6``), with
                     the self and background terms: the potential and the analytic field ``E = -grad phi``
``near_sum`` / ``near_field``  the pair sums over the minimum images with ``0 < r < r_c``
``coeffs``           ``b_k`` on ``[-N/2, N/2)^3``, ``b_0 = 0``, the unpaired planes zeroed
``exact_algorithm``  the algorithm in exact arithmetic: the trigonometric sum with those coefficients
                     (``oracle.ndft``) plus near, self and background
"""
import itertools
import math

import numpy as np
import torch

from oracle import ndft

MADELUNG_NACL = 1.7475645946331826
CUBIC_LATTICE = -2.8372974794806  # potential of one unit charge in the unit box at its own place


def erfc(a):
    return torch.special.erfc(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))).numpy()


def _columns(q):
    q = np.asarray(q)
    return q.reshape(q.shape[0], -1).astype(np.complex128 if np.iscomplexobj(q) else np.float64)


def _sets(batch, n):
    if batch is None:
        return [np.arange(n)]
    batch = np.asarray(batch)
    return [np.nonzero(batch == b)[0] for b in range(int(batch.max()) + 1 if batch.size else 0)]


def _pair_weights(d, alpha, r_c=None):
    """(erfc(alpha r) / r, -K'(r) / r) for the difference vectors d [.., 3]; zero where r = 0 or r >= r_c"""
    r = np.sqrt((d * d).sum(-1))
    ok = r > 0 if r_c is None else (r > 0) & (r < r_c)
    rs = np.where(ok, r, 1.0)
    k = erfc(alpha * rs) / rs
    mg = (k + 2.0 * alpha / math.sqrt(math.pi) * np.exp(-(alpha * rs) ** 2)) / (rs * rs)
    return np.where(ok, k, 0.0), np.where(ok, mg, 0.0)


def _terms(q, total, alpha):
    return -2.0 * alpha / math.sqrt(math.pi) * q - math.pi / alpha ** 2 * total


def converged(q, x, batch=None, alpha=6.0, nimg=2, kmax=14, field=False):
    """phi [n, *cols] (and E [n, 3, *cols]) of the converged Ewald sum, per point set"""
    q0 = np.asarray(q)
    x = np.asarray(x, dtype=np.float64)
    qc = _columns(q0)
    phi = np.zeros_like(qc)
    E = np.zeros((qc.shape[0], 3, qc.shape[1]), dtype=qc.dtype)
    ks = np.arange(-kmax, kmax + 1)
    K = np.stack(np.meshgrid(ks, ks, ks, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    k2 = (K * K).sum(-1)
    K, k2 = K[k2 > 0], k2[k2 > 0]
    b = np.exp(-math.pi ** 2 * k2 / alpha ** 2) / (math.pi * k2)
    for sel in _sets(batch, x.shape[0]):
        if sel.size == 0:
            continue
        xs, qs = x[sel], qc[sel]
        p, e = np.zeros_like(qs), np.zeros((sel.size, 3, qs.shape[1]), dtype=qs.dtype)
        for sh in itertools.product(range(-nimg, nimg + 1), repeat=3):
            d = xs[:, None, :] - xs[None, :, :] + np.array(sh, dtype=np.float64)
            w, mg = _pair_weights(d, alpha)
            p += w @ qs
            if field:
                e += np.einsum("ij,ija,jc->iac", mg, d, qs)
        for s in range(0, K.shape[0], 4096):
            Kc, bc = K[s:s + 4096], b[s:s + 4096]
            ph = np.exp(2j * math.pi * xs @ Kc.T)  # [n, nk]: e^{+2 pi i k.x_i}
            S = (np.conj(ph).T @ qs) * bc[:, None]  # b_k sum_j q_j e^{-2 pi i k.x_j}
            far = ph @ S
            p += far if np.iscomplexobj(qs) else far.real
            if field:
                fe = -np.einsum("ik,ka,kc->iac", ph, 2j * math.pi * Kc, S)
                e += fe if np.iscomplexobj(qs) else fe.real
        phi[sel] = p + _terms(qs, qs.sum(0, keepdims=True), alpha)
        E[sel] = e
    phi = phi.reshape(q0.shape)
    return (phi, E.reshape((q0.shape[0], 3) + q0.shape[1:])) if field else phi


def _near(q, x, batch, alpha, r_c):
    q0 = np.asarray(q)
    x = np.asarray(x, dtype=np.float64)
    qc = _columns(q0)
    z = np.zeros_like(qc)
    f = np.zeros((qc.shape[0], 3, qc.shape[1]), dtype=qc.dtype)
    for sel in _sets(batch, x.shape[0]):
        if sel.size == 0:
            continue
        d = x[sel][:, None, :] - x[sel][None, :, :]
        d = d - np.rint(d)
        w, mg = _pair_weights(d, alpha, r_c)
        z[sel] = w @ qc[sel]
        f[sel] = np.einsum("ij,ija,jc->iac", mg, d, qc[sel])
    return z.reshape(q0.shape), f.reshape((q0.shape[0], 3) + q0.shape[1:])


def near_sum(q, x, batch, alpha, r_c):
    """z_i = sum_{j: 0 < r_ij < r_c, same set} erfc(alpha r_ij) / r_ij q_j over the minimum images"""
    return _near(q, x, batch, alpha, r_c)[0]


def near_field(q, x, batch, alpha, r_c):
    """f_i = -sum_j g(r_ij^2) d_ij q_j, g = K'(r) / r of K = erfc(alpha r) / r: [n, 3, *cols]"""
    return _near(q, x, batch, alpha, r_c)[1]


def coeffs(alpha, N):
    k = np.arange(-(N // 2), N // 2, dtype=np.float64)
    k2 = (k * k)[:, None, None] + (k * k)[None, :, None] + (k * k)[None, None, :]
    b = np.exp(-math.pi ** 2 * k2 / alpha ** 2) / (math.pi * np.where(k2 > 0, k2, 1.0))
    b[k2 == 0] = 0.0
    b[0, :, :] = 0.0
    b[:, 0, :] = 0.0
    b[:, :, 0] = 0.0
    return b


def exact_algorithm(q, x, batch, alpha, r_c, N, field=False):
    """The algorithm in exact arithmetic: the trigonometric sum with the float64 coefficients + near, self, background"""
    q0 = np.asarray(q)
    x = np.asarray(x, dtype=np.float64)
    qc = _columns(q0)
    b = coeffs(alpha, N)
    z, f = _near(qc, x, batch, alpha, r_c)
    total = np.zeros_like(qc)
    for sel in _sets(batch, x.shape[0]):
        total[sel] = qc[sel].sum(0, keepdims=True)
    real = not np.iscomplexobj(qc)
    if not field:
        phi = ndft.ndft_fastsum(qc, b, x, None, batch, batch) + z + _terms(qc, total, alpha)
        return phi.reshape(q0.shape)
    k = 2j * math.pi * np.arange(-(N // 2), N // 2, dtype=np.float64)
    four = np.stack([b.astype(np.complex128), b * k[:, None, None], b * k[None, :, None], b * k[None, None, :]], -1)
    band = ndft.ndft_adjoint(qc, x, batch, N=N)  # [B, N, N, N, C]
    far = ndft.ndft_forward(band[..., None, :] * four[None, ..., None], x, batch)  # [n, 4, C]
    far = far.real if real else far
    phi = far[:, 0] + z + _terms(qc, total, alpha)
    E = far[:, 1:] + f
    return phi.reshape(q0.shape), E.reshape((q0.shape[0], 3) + q0.shape[1:])


def nacl():
    """the 8 ions of the rock-salt cell in the unit box (nearest distance 1/2; the ions sit on cell faces): x, q"""
    pts, qs = [], []
    for i, j, k in itertools.product(range(2), repeat=3):
        pts.append([i / 2 - 0.5, j / 2 - 0.5, k / 2 - 0.5])
        qs.append((-1.0) ** (i + j + k))
    return np.array(pts), np.array(qs)
