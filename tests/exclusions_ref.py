"""Float64 restatement of the bonded-pair exclusions (torch_nfft_amd/exclusions.py): the references of
tests/ewald_ref.py, ewald_box_ref.py, dispersion_ref.py and the two virial references, minus the listed terms, which are
written here directly from their formulas with numpy -- the r = 0 branch included.  A plain module like ewald_ref.py.

A list is `pairs` [m, 2] (unordered, each once) with one weight w = 1 - scale per pair; s holds FRACTIONAL positions and A the
box (None: the unit cube); d_ij = (ds - rint(ds)) A is the one image that a listed pair refers to."""
import math

import numpy as np

import dispersion_ref as dr
import dispersion_virial_ref as dv
import ewald_box_ref as eb
import ewald_ref as er
import ewald_virial_ref as ev

COULOMB, DISPERSION = 0, 1


def zero_constant(kind, alpha):
    """the limit at r = 0 of the smooth part that the far field sums: erf(alpha r) / r -> 2 alpha / sqrt(pi), and
    (1 - e^(-a^2) (1 + a^2 + a^4 / 2)) / r^6 -> alpha^6 / 6"""
    return 2.0 * alpha / math.sqrt(math.pi) if kind == COULOMB else alpha ** 6 / 6.0


def images(s, A, pairs):
    """d_ij [m, 3] of the listed pairs: the minimum image of x_i - x_j, wrapped in fractional coordinates"""
    s = np.asarray(s, dtype=np.float64)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    ds = s[pairs[:, 0]] - s[pairs[:, 1]]
    return (ds - np.rint(ds)) @ dr._box(A)


def kernels(kind, d, alpha):
    """(K0, K1) [m] of the separations d [m, 3]: 1 / r and 1 / r^3, or 1 / r^6 and 6 / r^8; at r = 0 the constant and 0"""
    r = np.sqrt((d * d).sum(-1))
    ok = r > 0
    rs = np.where(ok, r, 1.0)
    if kind == COULOMB:
        k0, k1 = 1.0 / rs, 1.0 / rs ** 3
    else:
        k0, k1 = 1.0 / rs ** 6, 6.0 / rs ** 8
    return np.where(ok, k0, zero_constant(kind, alpha)), np.where(ok, k1, 0.0)


def _weights(weights, m):
    return np.broadcast_to(np.asarray(weights, dtype=np.float64), (m,))


def listed_terms(kind, x, s, A, pairs, weights, alpha):
    """(z [n, *cols], f [n, 3, *cols]): what the listed pairs take out of the potential and of the field,
    z_i = sum_{j in ex(i)} w_ij K0(r) x_j and f_i = sum w_ij K1(r) d_ij x_j"""
    x0 = np.asarray(x)
    xc = dr._columns(x0)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    w = _weights(weights, pairs.shape[0])
    d = images(s, A, pairs)
    k0, k1 = kernels(kind, d, alpha)
    z = np.zeros_like(xc)
    f = np.zeros((xc.shape[0], 3, xc.shape[1]), dtype=xc.dtype)
    i, j = pairs[:, 0], pairs[:, 1]
    np.add.at(z, i, (w * k0)[:, None] * xc[j])
    np.add.at(z, j, (w * k0)[:, None] * xc[i])
    g = (w * k1)[:, None] * d  # [m, 3]
    np.add.at(f, i, g[:, :, None] * xc[j][:, None, :])
    np.add.at(f, j, -g[:, :, None] * xc[i][:, None, :])
    return dr._shaped(x0, z, f)


def listed_virial(kind, x, s, A, batch, pairs, weights, alpha):
    """(U [B, *cols], W [B, 3, 3, *cols]): the listed pairs' share of the energy and of the virial, each pair once:
    sum w K0(r) x_i x_j and sum w K1(r) d_a d_b x_i x_j (the r = 0 constant in U only)"""
    x0 = np.asarray(x)
    xc = dr._columns(x0)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    w = _weights(weights, pairs.shape[0])
    d = images(s, A, pairs)
    k0, k1 = kernels(kind, d, alpha)
    B = 1 if batch is None else int(np.asarray(batch)[-1]) + 1
    which = np.zeros(pairs.shape[0], dtype=np.int64) if batch is None else np.asarray(batch)[pairs[:, 0]]
    U = np.zeros((B, xc.shape[1]), dtype=xc.dtype)
    W = np.zeros((B, 3, 3, xc.shape[1]), dtype=xc.dtype)
    v = xc[pairs[:, 0]] * xc[pairs[:, 1]]  # [m, C]
    np.add.at(U, which, (w * k0)[:, None] * v)
    np.add.at(W, which, (w * k1)[:, None, None, None] * d[:, :, None, None] * d[:, None, :, None] * v[:, None, None, :])
    cols = x0.shape[1:]
    return U.reshape((B,) + cols), W.reshape((B, 3, 3) + cols)


def _minus(whole, listed):
    return whole[0] - listed[0], whole[1] - listed[1]


def coulomb_converged(q, s, A, batch, pairs, weights, alpha=6.0, **kw):
    """(phi, E) of the converged Coulomb sum without the listed pairs"""
    if A is None:
        whole = er.converged(q, s, batch, alpha=alpha, field=True, **kw)
    else:
        whole = eb.converged(q, s, A, batch, alpha=alpha, field=True, **kw)
    return _minus(whole, listed_terms(COULOMB, q, s, A, pairs, weights, alpha))


def coulomb_algorithm(q, s, A, batch, pairs, weights, alpha, r_c, N):
    """(phi, E) of the truncated algorithm in float64 without the listed pairs"""
    if A is None:
        whole = er.exact_algorithm(q, s, batch, alpha, r_c, N, field=True)
    else:
        whole = eb.exact_algorithm(q, s, A, batch, alpha, r_c, N, field=True)
    return _minus(whole, listed_terms(COULOMB, q, s, A, pairs, weights, alpha))


def dispersion_converged(c, s, A, batch, pairs, weights, alpha=3.2, N=30, nimg=2):
    """(psi, G) of the converged dispersion sum (every image within nimg cells, |k| < N / 2) without the listed pairs"""
    return _minus(dr.dispersion(c, s, A, batch, alpha, None, N, nimg=nimg), listed_terms(DISPERSION, c, s, A, pairs, weights, alpha))


def dispersion_algorithm(c, s, A, batch, pairs, weights, alpha, r_c, N):
    """(psi, G) of the truncated algorithm in float64 without the listed pairs"""
    return _minus(dr.dispersion(c, s, A, batch, alpha, r_c, N), listed_terms(DISPERSION, c, s, A, pairs, weights, alpha))


def coulomb_virial_converged(q, s, A, batch, pairs, weights, alpha=6.0, **kw):
    """(U, W) of the converged Coulomb sum without the listed pairs"""
    whole = ev.converged_virial(q, s, dr._box(A), batch, alpha=alpha, **kw)
    return _minus(whole, listed_virial(COULOMB, q, s, A, batch, pairs, weights, alpha))


def coulomb_virial_algorithm(q, s, A, batch, pairs, weights, alpha, r_c, N):
    whole = ev.exact_algorithm_virial(q, s, dr._box(A), batch, alpha, r_c, N)
    return _minus(whole, listed_virial(COULOMB, q, s, A, batch, pairs, weights, alpha))


def dispersion_virial_converged(c, s, A, batch, pairs, weights, alpha=3.2, **kw):
    """(U, W) of the converged dispersion sum without the listed pairs"""
    whole = dv.converged_virial(c, s, dr._box(A), batch, alpha=alpha, **kw)
    return _minus(whole, listed_virial(DISPERSION, c, s, A, batch, pairs, weights, alpha))


def dispersion_virial_algorithm(c, s, A, batch, pairs, weights, alpha, r_c, N):
    whole = dv.exact_algorithm_virial(c, s, dr._box(A), batch, alpha, r_c, N)
    return _minus(whole, listed_virial(DISPERSION, c, s, A, batch, pairs, weights, alpha))


def energy(x, phi, batch=None):
    """U_b = 1/2 sum_{i in set b} x_i phi_i, [B, *cols]"""
    x, phi = np.asarray(x, dtype=np.float64), np.asarray(phi, dtype=np.float64)
    return np.stack([0.5 * (x[sel] * phi[sel]).sum(0) for sel in dr._sets(batch, x.shape[0])])


def csr(pairs, n, weights):
    """(row_start [n + 1], col [2 m], weight [2 m]) of the symmetrised list sorted by (i, j): what ExclusionList must hold"""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    w = _weights(weights, pairs.shape[0])
    rows = np.concatenate([pairs[:, 0], pairs[:, 1]])
    cols = np.concatenate([pairs[:, 1], pairs[:, 0]])
    order = np.lexsort((cols, rows))
    row_start = np.zeros(n + 1, dtype=np.int64)
    np.add.at(row_start, rows + 1, 1)
    return np.cumsum(row_start), cols[order], np.concatenate([w, w])[order]


def bonded_list(s, A, batch, seed=0, hub=20):
    """The list of the GPU tests on the fractional float32 points s [n, 3] (two point sets through batch), MOVING points so that
    every way to go wrong is present once; returns (s, pairs, coulomb_scale, dispersion_scale):

    * chains (i, i + 1) at scale 0 and (i, i + 2) at 0.5 / 0.25 (Coulomb / dispersion) over the first 60 points of each set,
      bonded at 0.02 .. 0.05 box lengths (the first bond of the first set at 0.02 exactly);
    * one hub point with `hub` partners at 0.03 .. 0.05;
    * a pair on opposite sides of a face of the box, on each axis;
    * a coincident listed pair (scale 0);
    * every other point has an empty row."""
    rng = np.random.default_rng(seed)
    s = np.array(s, dtype=np.float64)
    n = s.shape[0]
    batch = np.zeros(n, dtype=np.int64) if batch is None else np.asarray(batch)
    inv = np.linalg.inv(dr._box(A))

    box = dr._box(A)

    def step(length):
        e = rng.standard_normal(3)
        return (length * e / np.linalg.norm(e)) @ inv

    def place(origin, length, others, apart):
        """a point at `length` from s[origin] and at least `apart` from the points `others` (a chain that folds back on itself,
        or two partners of the hub side by side, would put an unlisted pair closer than any bond)"""
        for _ in range(1000):
            y = s[origin] + step(length)
            if all(np.linalg.norm((y - s[o]) @ box) >= apart for o in others):
                return y
        raise AssertionError("no room for the point")

    pairs, sc, sd = [], [], []

    def add(i, j, coulomb, dispersion):
        pairs.append((i, j))
        sc.append(coulomb)
        sd.append(dispersion)

    for b in np.unique(batch):
        first = int(np.flatnonzero(batch == b)[0])
        for k in range(1, 60):
            length = 0.02 if (b == batch[0] and k == 1) else rng.uniform(0.02, 0.05)
            s[first + k] = place(first + k - 1, length, range(first, first + k - 1), 0.03)
        for k in range(59):
            add(first + k, first + k + 1, 0.0, 0.0)
        for k in range(58):
            add(first + k + 2, first + k, 0.5, 0.25)  # (given upper end first)
    base = int(np.flatnonzero(batch == batch[0])[0]) + 70
    for k in range(1, hub + 1):  # the hub and its partners
        s[base + k] = place(base, rng.uniform(0.03, 0.05), range(base + 1, base + k), 0.015)
        add(base, base + k, 0.0, 0.0)
    face = base + hub + 2
    for a in range(3):  # a pair across each face
        y = rng.random(3) - 0.5
        s[face + 2 * a] = y
        s[face + 2 * a + 1] = y + step(0.03)
        s[face + 2 * a, a] = 0.49
        s[face + 2 * a + 1, a] = -0.49
        add(face + 2 * a, face + 2 * a + 1, 1.0 / 1.2, 0.5)
    twin = face + 8
    s[twin + 1] = s[twin]  # a Drude pair
    add(twin, twin + 1, 0.0, 0.0)
    assert twin + 1 < int(np.flatnonzero(batch == batch[0])[-1])
    return s.astype(np.float32), np.array(pairs, dtype=np.int64), np.array(sc), np.array(sd)

