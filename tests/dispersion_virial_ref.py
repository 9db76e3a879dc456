"""Float64 restatement of the virial tensor of the dispersion Ewald sum, the periodic 1/r^6 -- TEST
INFRASTRUCTURE ONLY.

Written independently of ``torch_nfft_amd/dispersion.py`` and of ``csrc/ewald_disp_virial.hip``, dense numpy in float64, on
``tests/dispersion_ref.py`` (its boxes, wave vectors, pair weights, coefficients and lattice sum) in the layout of
``tests/ewald_virial_ref.py``.  The box is the matrix ``A`` whose rows are the lattice vectors (``None``: the unit cube), the
positions are FRACTIONAL, ``x = s A``, ``kappa = A^-1 k``, ``V = det A``, ``a = alpha r``, ``b = pi |kappa| / alpha``.  For the
homogeneous strain ``A -> A (1 + eps)`` at fixed ``s`` the virial is ``W_ab = -dU / d eps_ab`` of ``U = 1/2 sum_i c_i psi_i``
(the sign convention of ``nfft_ewald_dispersion_energy``: the physical energy and virial are ``-U`` and ``-W``).  Everything
returns ``(U, W)`` with ``U`` ``[B, *cols]`` and ``W`` ``[B, 3, 3, *cols]``, one row per point set (an empty set: zeros):

``near_virial``             ``1/2 sum_ij c_i c_j (w, mg d_a d_b)`` over ``d = (ds - rint(ds) + n) A`` with ``0 < |d| < r_c``
                            (``nimg`` shells of images ``n``; ``r_c=None``: no cut)
``strain_coeffs``           ``t_k = (d b_k / d |kappa|) / |kappa| = (2 pi^(7/2) alpha / V) (sqrt(pi) b erfc(b) - e^(-b^2))`` on
                            ``[-N/2, N/2)^3``, clamped at ``<= 0``, the unpaired planes ``k_a = -N/2`` zeroed
``far_virial``              ``1/2 sum_k |S_k|^2 (b_k, b_k delta_ab + t_k kappa_a kappa_b)`` from a given ``band`` (``S_k`` at index
                            ``k + N/2``), ``b`` and ``t``; cells with ``b_k = 0`` are skipped, the ``k = 0`` term is kept
``exact_algorithm_virial``  the algorithm in exact arithmetic: ``oracle.ndft.ndft_adjoint`` for the band, ``dr.coeffs`` and
                            ``strain_coeffs``, plus near and the self term ``-(alpha^6 / 12) sum c_i^2`` (in ``U`` only)
``converged_virial``        the split carried to convergence (``alpha = 3.2``, ``N = 30``, two shells of images, no cut): its
                            analytic ``W``, and for ``U`` either the same split or, with ``R``, the energy of the brute-force
                            ``dr.lattice_sum`` over every image within ``R`` -- in the box that is passed, strained or not

``mutant`` evaluates a deliberately wrong formula (tests/test_dispersion_virial_ref.py measures how far off each is, so that
the tolerances of the GPU tests are shown not to hide them): ``"ds"`` the outer product of the fractional difference in
place of ``d``, ``"AT"`` ``A^T`` in place of ``A``, ``"top_term"`` ``a^6`` dropped from ``mg``, ``"k"`` ``k_a k_b`` in place of
``kappa_a kappa_b``, ``"no_t"`` ``t_k`` left out, ``"no_k0"`` the ``k = 0`` term left out.
"""
import itertools
import math

import numpy as np

import dispersion_ref as dr
from oracle import ndft


def _num_sets(batch):
    if batch is None:
        return 1
    batch = np.asarray(batch)
    return int(batch.max()) + 1 if batch.size else 0


def _shape(U, W, c0):
    cols = np.asarray(c0).shape[1:]
    return U.reshape((U.shape[0],) + cols), W.reshape((W.shape[0], 3, 3) + cols)


def _pairs(cs, ss, A, alpha, r_c, shifts, mutant=None):
    """(U, W) [C], [3, 3, C] of one point set: 1/2 sum_ij c_i c_j (w, mg d_a d_b) over the images ds - rint(ds) + shift"""
    U = np.zeros(cs.shape[1])
    W = np.zeros((3, 3, cs.shape[1]))
    M = A.T if mutant == "AT" else A
    for r0 in range(0, ss.shape[0], 512):  # (rows in blocks: the pair arrays stay small)
        ds = ss[r0:r0 + 512, None, :] - ss[None, :, :]
        ds = ds - np.rint(ds)
        ci = cs[r0:r0 + 512]
        for sh in shifts:
            dsn = ds + np.array(sh, dtype=np.float64)
            d = dsn @ M
            w, mg = dr.pair_weights(d, alpha, r_c)
            if mutant == "top_term":
                mg = dr.pair_weights(d, alpha, r_c, top_term=False)[1]
            o = dsn if mutant == "ds" else d
            U += 0.5 * np.einsum("ic,ij,jc->c", ci, w, cs, optimize=True)
            for a in range(3):
                for b in range(a, 3):
                    W[a, b] += 0.5 * np.einsum("ic,ij,jc->c", ci, mg * o[..., a] * o[..., b], cs, optimize=True)
    for a in range(3):
        for b in range(a):
            W[a, b] = W[b, a]
    return U, W


def near_virial(c, s, A, batch, alpha, r_c, mutant=None, nimg=0):
    c0 = np.asarray(c)
    s = np.asarray(s, dtype=np.float64)
    A = dr._box(A)
    cc = dr._columns(c0)
    B = _num_sets(batch)
    U, W = np.zeros((B, cc.shape[1])), np.zeros((B, 3, 3, cc.shape[1]))
    shifts = tuple(itertools.product(range(-nimg, nimg + 1), repeat=3))
    for i, sel in enumerate(dr._sets(batch, s.shape[0])):
        if sel.size == 0:
            continue
        U[i], W[i] = _pairs(cc[sel], s[sel], A, alpha, r_c, shifts, mutant)
    return _shape(U, W, c0)


def strain_factor(b):
    """f'(b) / (6 b) = sqrt(pi) b erfc(b) - e^(-b^2), clamped at 0 from above (-1 at b = 0, ~ -e^(-b^2) / (2 b^2) for large b)"""
    b = np.asarray(b, dtype=np.float64)
    return np.minimum(math.sqrt(math.pi) * b * dr.erfc(b) - np.exp(-b * b), 0.0)


def strain_coeffs(A, alpha, N):
    _, kap = dr.kappa(A, N)
    V = abs(np.linalg.det(dr._box(A)))
    t = 2.0 * math.pi ** 3.5 * alpha / V * strain_factor(math.pi * np.sqrt((kap * kap).sum(-1)) / alpha)
    t[0, :, :] = 0.0
    t[:, 0, :] = 0.0
    t[:, :, 0] = 0.0
    return t


def far_virial(band, b, t, A, mutant=None):
    """band [B, N, N, N, *cols] complex (index k + N/2), b and t [N, N, N]"""
    band = np.asarray(band)
    N = band.shape[1]
    cols = band.shape[4:]
    p = (band.real.astype(np.float64) ** 2 + band.imag.astype(np.float64) ** 2).reshape(band.shape[0], N ** 3, -1)
    k_int, kap = dr.kappa(A, N)
    k_int, kap = k_int.reshape(-1, 3), kap.reshape(-1, 3)
    bb = np.asarray(b, dtype=np.float64).reshape(-1).copy()
    tt = np.where(bb != 0, np.asarray(t, dtype=np.float64).reshape(-1), 0.0)
    if mutant == "no_t":
        tt = np.zeros_like(tt)
    if mutant == "no_k0":
        bb[(k_int == 0).all(1)] = 0.0
    kk = k_int if mutant == "k" else kap
    U = 0.5 * np.einsum("k,nkc->nc", bb, p)
    W = np.eye(3)[None, :, :, None] * U[:, None, None, :] + 0.5 * np.einsum("k,ka,kb,nkc->nabc", tt, kk, kk, p, optimize=True)
    return U.reshape((U.shape[0],) + cols), W.reshape((W.shape[0], 3, 3) + cols)


def _self_energy(c, batch, alpha):
    """-(alpha^6 / 12) sum_{i in set} c_i^2, [B, C]"""
    cc = dr._columns(c)
    return np.stack([-(alpha ** 6 / 12.0) * (cc[sel] * cc[sel]).sum(0) for sel in dr._sets(batch, cc.shape[0])]) \
        if _num_sets(batch) else np.zeros((0, cc.shape[1]))


def exact_algorithm_virial(c, s, A, batch, alpha, r_c, N, mutant=None, nimg=0):
    c0 = np.asarray(c)
    s = np.asarray(s, dtype=np.float64)
    cc = dr._columns(c0)
    Un, Wn = near_virial(cc, s, A, batch, alpha, r_c, mutant, nimg)
    band = ndft.ndft_adjoint(cc, s, batch, N=N)  # [B, N, N, N, C]
    Uf, Wf = far_virial(band, dr.coeffs(A, alpha, N), strain_coeffs(A, alpha, N), A, mutant)
    return _shape(Un + Uf + _self_energy(cc, batch, alpha), Wn + Wf, c0)


def converged_virial(c, s, A, batch=None, R=None, alpha=3.2, N=30, nimg=2):
    U, W = exact_algorithm_virial(c, s, A, batch, alpha, None, N, nimg=nimg)
    if R is not None:  # the energy of the brute-force sum in place of the split's own
        c0 = np.asarray(c)
        cc = dr._columns(c0)
        psi = dr._columns(dr.lattice_sum(cc, s, A, R, batch)[0])
        U = np.stack([0.5 * (cc[sel] * psi[sel]).sum(0) for sel in dr._sets(batch, cc.shape[0])]).reshape(U.shape)
    return U, W


# ---- the point sets and bands of tests/test_gpu_dispersion_virial.py (here, so that tests/test_dispersion_virial_ref.py can
# measure the wrong formulas on the very same inputs without a device) ---------------------------------------------------

def near_points():
    """700 float32 FRACTIONAL points: a 9^3 jittered lattice (spacing 1/9, jitter 0.025: no two closer than 0.06 before the
    box's metric) in random order, with the edge cases of the wrap of tests/test_gpu_ewald_virial.py written over the first
    hundred.  The exact duplicates (r = 0) stay; every other pair made on purpose is 0.04 .. 0.07 apart in fractional
    terms, because with 1/r^8 one pair at 1e-3 would be the whole sum."""
    rng = np.random.default_rng(0)
    x = rng.permutation(dr.jittered_lattice(rng, 9, 1.0 / 9, 0.025).reshape(-1, 3))[:700].copy()
    x[40:60] = x[0:20]                                    # exact duplicates: r = 0
    below = np.nextafter(np.float32(0.5), np.float32(0))  # the largest float32 below 1/2
    for a in range(3):
        x[60 + a, a] = -0.5                               # exactly on the lower face
        x[63 + a, a] = below
    x[63, :] = below                                      # (the upper corner)
    for a in range(3):                                    # ... each with a neighbour 0.04 .. 0.06 away
        x[66 + a] = x[60 + a] + (np.float32(0.025) + np.float32(0.01) * rng.random(3).astype(np.float32))
        x[69 + a] = x[63 + a] - (np.float32(0.025) + np.float32(0.01) * rng.random(3).astype(np.float32))
    x[72:80] += np.float32(0.7)                           # given outside the box: must act as their images
    x[80:88] -= np.float32(1.2)
    for a in range(3):                                    # a pair 0.04 apart through each face, beside its lattice node
        y = x[88 + 2 * a].copy()
        x[89 + 2 * a] = y + np.float32(0.01)
        x[88 + 2 * a, a] = -0.48
        x[89 + 2 * a, a] = 0.48
    return x


def crowded_points():
    """3000 float32 fractional points of a 15^3 jittered lattice (spacing 0.004, jitter 20 %: no two closer than 0.0024) in a
    cube of edge 0.06 centred on the corner (1/2, 1/2, 1/2): ~375 in each of the eight corner cells of a 3^3 grid -- three
    work items per cell, the last with idle lanes, two LDS tiles per cell, every pair inside r_c = 0.3 and most through a wrap"""
    rng = np.random.default_rng(7)
    x = dr.jittered_lattice(rng, 15, 0.004, 0.2 * 0.004, centre=0.5).reshape(-1, 3)
    return rng.permutation(x)[:3000].copy()


def ragged_batch(n=700):
    """three point sets, the middle one empty; the edge cases share the first"""
    return np.concatenate([np.zeros(330, np.int64), np.full(n - 330, 2, np.int64)])


def values(rng, n, cols):
    """coefficients in [0.5, 1.5): dispersion coefficients are positive (as tests/test_gpu_dispersion.py)"""
    return (rng.random((n,) + cols) + 0.5).astype(np.float32)


def far_alpha(N):
    """alpha of the far tests: b = pi |kappa| / alpha is about 2 on the plane k_a = N/2 of a unit edge, where f(b) = 4e-3 and
    the strain factor is -6e-3: b_k and t_k count out to the grid's edge"""
    return 0.8 * N


def far_band(N, name, cols):
    """a complex64 band [2, N, N, N, *cols] of standard normals whose k = 0 cell is raised by 8: the S_0 = sum c of positive
    coefficients stands far above the other cells, and with all cells alike the k = 0 term would be lost among N^3"""
    rng = np.random.default_rng(N + len(cols) + ord(name))
    shape = (2, N, N, N) + cols
    band = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)
    band[:, N // 2, N // 2, N // 2] *= 8
    return band


WHOLE = (14.0, 0.25, 32)  # alpha, r_c, N of the whole-function tests (those of tests/test_gpu_dispersion.py)


def whole_points():
    """(s, c, batch): 7^3 float32 fractional points on a jittered lattice (spacing 1/7, jitter 0.03) in two point sets, one
    column of coefficients -- dense enough that U is not what is left of the self term (tests/test_gpu_dispersion.py)"""
    rng = np.random.default_rng(3)
    s = rng.permutation(dr.jittered_lattice(rng, 7, 1.0 / 7, 0.03).reshape(-1, 3))
    return s, values(rng, s.shape[0], ()), (np.arange(s.shape[0]) >= 160).astype(np.int64)


def rel_fro(a, b):
    """relative Frobenius / l2 error of a against b"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel()))
