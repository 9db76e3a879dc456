"""Float64 restatement of the Ewald sum for the periodic 1/r in an orthorhombic or triclinic box -- TEST INFRASTRUCTURE ONLY.

Written independently of ``torch_nfft_amd/ewald.py``, dense and in float64, in the style of ``tests/ewald_ref.py`` (whose
helpers for columns, point sets and pair weights it shares).  The box is the matrix ``A`` ``[3, 3]`` whose rows are the
lattice vectors (lower triangular for the library; nothing here needs that), the positions are FRACTIONAL, ``x = s A``,
the wave vector of the integer frequency ``k`` is ``kappa = A^-1 k`` and ``V = det A``:

``converged``        the Ewald sum carried to convergence (images ``|n|_inf <= 2`` around the wrapped difference,
                     ``|k|_inf <= 14``, ``alpha = 6``), with the self and background terms: the potential and the analytic
                     Cartesian field ``E = -grad_x phi``
``near_sum`` / ``near_field``  the pair sums over ``d = (ds - rint(ds)) A`` with ``0 < |d| < r_c``
``near_all_images``  the same pair sums over every image ``|n|_inf <= 2`` within ``r_c``: no componentwise shortcut
``coeffs``           ``b_k = exp(-pi^2 |kappa|^2 / alpha^2) / (pi V |kappa|^2)`` on ``[-N/2, N/2)^3``, ``b_0 = 0``, the unpaired
                     planes zeroed
``exact_algorithm``  the algorithm in exact arithmetic: the trigonometric sum with those coefficients on the fractional
                     positions (``oracle.ndft``) plus near, self and background
"""
import itertools
import math

import numpy as np

from ewald_ref import _columns, _pair_weights, _sets
from oracle import ndft

T = np.array([[1.0, 0.0, 0.0], [0.35, 1.1, 0.0], [-0.25, 0.3, 0.95]])  # triclinic: widths 0.900, 1.049, 0.95
O = np.diag([1.0, 1.3, 0.8])                                            # orthorhombic
S = np.array([[1.0, 0.0, 0.0], [1.0, 1.0, 0.0], [0.0, 0.0, 1.0]])       # the cubic lattice in a cell sheared by a full edge
ROCK_SALT_PRIMITIVE = np.array([[0.0, 0.5, 0.5], [0.5, 0.0, 0.5], [0.5, 0.5, 0.0]])  # fcc; ions at s = 0 and (1/2, 1/2, 1/2)


def widths(A):
    """the perpendicular widths w_a = 1 / |column a of A^-1|"""
    return 1.0 / np.linalg.norm(np.linalg.inv(np.asarray(A, dtype=np.float64)), axis=0)


def lower_triangular(M):
    """(A, Q): the cell M (rows = lattice vectors) as A = M Q, lower triangular with a positive diagonal, Q orthogonal
    (QR of M^T); fractional coordinates are the same in both"""
    Q, R = np.linalg.qr(np.asarray(M, dtype=np.float64).T)
    D = np.sign(np.diag(R))
    return np.tril((R * D[:, None]).T), Q * D[None, :]


def _terms(q, total, alpha, V):
    return -2.0 * alpha / math.sqrt(math.pi) * q - math.pi / (alpha ** 2 * V) * total


def converged(q, s, A, batch=None, alpha=6.0, nimg=2, kmax=14, field=False):
    """phi [n, *cols] (and the Cartesian E [n, 3, *cols]) of the converged Ewald sum, per point set"""
    q0 = np.asarray(q)
    s = np.asarray(s, dtype=np.float64)
    A = np.asarray(A, dtype=np.float64)
    V = abs(np.linalg.det(A))
    qc = _columns(q0)
    phi = np.zeros_like(qc)
    E = np.zeros((qc.shape[0], 3, qc.shape[1]), dtype=qc.dtype)
    ks = np.arange(-kmax, kmax + 1)
    K = np.stack(np.meshgrid(ks, ks, ks, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    K = K[(K * K).sum(-1) > 0]
    kappa = K @ np.linalg.inv(A).T  # kappa_b = sum_a (A^-1)_ba k_a
    k2 = (kappa * kappa).sum(-1)
    b = np.exp(-math.pi ** 2 * k2 / alpha ** 2) / (math.pi * V * k2)
    for sel in _sets(batch, s.shape[0]):
        if sel.size == 0:
            continue
        ss, qs = s[sel], qc[sel]
        p, e = np.zeros_like(qs), np.zeros((sel.size, 3, qs.shape[1]), dtype=qs.dtype)
        ds = ss[:, None, :] - ss[None, :, :]
        ds = ds - np.rint(ds)  # (any representative: the images below are summed around it)
        for sh in itertools.product(range(-nimg, nimg + 1), repeat=3):
            d = (ds + np.array(sh, dtype=np.float64)) @ A
            w, mg = _pair_weights(d, alpha)
            p += w @ qs
            if field:
                e += np.einsum("ij,ija,jc->iac", mg, d, qs)
        for c0 in range(0, K.shape[0], 4096):
            Kc, kc, bc = K[c0:c0 + 4096], kappa[c0:c0 + 4096], b[c0:c0 + 4096]
            ph = np.exp(2j * math.pi * ss @ Kc.T)  # [n, nk]: e^{+2 pi i k.s_i}
            Sk = (np.conj(ph).T @ qs) * bc[:, None]
            far = ph @ Sk
            p += far if np.iscomplexobj(qs) else far.real
            if field:
                fe = -np.einsum("ik,ka,kc->iac", ph, 2j * math.pi * kc, Sk)
                e += fe if np.iscomplexobj(qs) else fe.real
        phi[sel] = p + _terms(qs, qs.sum(0, keepdims=True), alpha, V)
        E[sel] = e
    phi = phi.reshape(q0.shape)
    return (phi, E.reshape((q0.shape[0], 3) + q0.shape[1:])) if field else phi


def _near(q, s, A, batch, alpha, r_c, shifts=((0, 0, 0),)):
    q0 = np.asarray(q)
    s = np.asarray(s, dtype=np.float64)
    A = np.asarray(A, dtype=np.float64)
    qc = _columns(q0)
    z = np.zeros_like(qc)
    f = np.zeros((qc.shape[0], 3, qc.shape[1]), dtype=qc.dtype)
    for sel in _sets(batch, s.shape[0]):
        if sel.size == 0:
            continue
        ds = s[sel][:, None, :] - s[sel][None, :, :]
        ds = ds - np.rint(ds)
        for sh in shifts:
            d = (ds + np.array(sh, dtype=np.float64)) @ A
            w, mg = _pair_weights(d, alpha, r_c)
            z[sel] += w @ qc[sel]
            f[sel] += np.einsum("ij,ija,jc->iac", mg, d, qc[sel])
    return z.reshape(q0.shape), f.reshape((q0.shape[0], 3) + q0.shape[1:])


def near_sum(q, s, A, batch, alpha, r_c):
    """z_i = sum_{j: 0 < r_ij < r_c, same set} erfc(alpha r_ij) / r_ij q_j, r_ij = |(ds - rint(ds)) A|"""
    return _near(q, s, A, batch, alpha, r_c)[0]


def near_field(q, s, A, batch, alpha, r_c):
    """f_i = -sum_j g(r_ij^2) d_ij q_j (Cartesian), g = K'(r) / r of K = erfc(alpha r) / r: [n, 3, *cols]"""
    return _near(q, s, A, batch, alpha, r_c)[1]


def near_all_images(q, s, A, batch, alpha, r_c, nimg=2):
    """(z, f) over EVERY image |n|_inf <= nimg with 0 < |d| < r_c"""
    return _near(q, s, A, batch, alpha, r_c, tuple(itertools.product(range(-nimg, nimg + 1), repeat=3)))


def _kappa(A, N):
    k = np.arange(-(N // 2), N // 2, dtype=np.float64)
    K = np.stack(np.meshgrid(k, k, k, indexing="ij"), -1)  # [N, N, N, 3]
    return K @ np.linalg.inv(np.asarray(A, dtype=np.float64)).T


def coeffs(A, alpha, N):
    kappa = _kappa(A, N)
    V = abs(np.linalg.det(np.asarray(A, dtype=np.float64)))
    k2 = (kappa * kappa).sum(-1)
    b = np.exp(-math.pi ** 2 * k2 / alpha ** 2) / (math.pi * V * np.where(k2 > 0, k2, 1.0))
    b[N // 2, N // 2, N // 2] = 0.0
    b[0, :, :] = 0.0
    b[:, 0, :] = 0.0
    b[:, :, 0] = 0.0
    return b


def exact_algorithm(q, s, A, batch, alpha, r_c, N, field=False):
    """The algorithm in exact arithmetic: the trigonometric sum with the float64 coefficients + near, self, background"""
    q0 = np.asarray(q)
    s = np.asarray(s, dtype=np.float64)
    A = np.asarray(A, dtype=np.float64)
    V = abs(np.linalg.det(A))
    qc = _columns(q0)
    b = coeffs(A, alpha, N)
    z, f = _near(qc, s, A, batch, alpha, r_c)
    total = np.zeros_like(qc)
    for sel in _sets(batch, s.shape[0]):
        total[sel] = qc[sel].sum(0, keepdims=True)
    real = not np.iscomplexobj(qc)
    if not field:
        phi = ndft.ndft_fastsum(qc, b, s, None, batch, batch) + z + _terms(qc, total, alpha, V)
        return phi.reshape(q0.shape)
    kappa = 2j * math.pi * _kappa(A, N)
    four = np.stack([b.astype(np.complex128), b * kappa[..., 0], b * kappa[..., 1], b * kappa[..., 2]], -1)
    band = ndft.ndft_adjoint(qc, s, batch, N=N)  # [B, N, N, N, C]
    far = ndft.ndft_forward(band[..., None, :] * four[None, ..., None], s, batch)  # [n, 4, C]
    far = far.real if real else far
    phi = far[:, 0] + z + _terms(qc, total, alpha, V)
    E = far[:, 1:] + f
    return phi.reshape(q0.shape), E.reshape((q0.shape[0], 3) + q0.shape[1:])
