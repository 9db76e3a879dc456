"""Float64 restatement of the Lennard-Jones + Coulomb step with per-type-pair parameters -- TEST
INFRASTRUCTURE ONLY.  ``nfft_ewald_lj_table_step`` is ``lj_step_ref`` / ``lj_excl_ref`` for ``(q, c)`` with no repulsion
coefficient, ``c_i = g[t_i]`` the grid's per-type coefficient, plus the direct sums over the minimum images with
``0 < r < r_c`` of ``C12(t_i, t_j) / r^12`` and ``dC6(t_i, t_j) / r^6``, ``dC6 = C6 - outer(g, g)``.  The listed image of a listed
pair is scaled by ``s^L`` INSIDE those sums, not subtracted afterwards.  A plain module like lj_excl_ref.py; positions are
FRACTIONAL, ``A`` holds the lattice vectors as rows.

A parameter set is ``tab = (C6 [T, T], C12 [T, T], g [T])``.

``mutant`` evaluates a deliberately wrong formula: ``"c6_for_delta"`` takes the pair's whole ``C6`` where ``dC6`` belongs (the
grid's share counted twice), ``"delta_sign"`` adds ``dC6 / r^6`` instead of subtracting it, ``"types_permuted"`` looks the table
up with the types reversed (``T - 1 - t``), ``"delta_unscaled"`` leaves the Lennard-Jones scale of a listed pair off ``dC6``.
"""
import itertools

import numpy as np

import dispersion_ref as dr
import lj_excl_ref as le
import lj_step_ref as lj


def lorentz_berthelot(sigma, eps):
    """(C6, C12, g): sigma_ij = (sigma_i + sigma_j) / 2, eps_ij = sqrt(eps_i eps_j); g = 2 sqrt(eps) sigma^3"""
    sigma, eps = np.asarray(sigma, dtype=np.float64), np.asarray(eps, dtype=np.float64)
    sij = 0.5 * (sigma[:, None] + sigma[None, :])
    e4 = 4.0 * np.sqrt(eps[:, None] * eps[None, :])
    return e4 * sij ** 6, e4 * sij ** 12, 2.0 * np.sqrt(eps) * sigma ** 3


def geometric(sigma, eps):
    """the same for sigma_ij = sqrt(sigma_i sigma_j): C6 = outer(g, g), C12 = outer(a, a) with lj.lj_coefficients' (g, a)"""
    g, a = lj.lj_coefficients(sigma, eps)
    return np.outer(g, g), np.outer(a, a), g


def sigma_of(tab):
    """sigma(t, t') = (C12 / C6)^(1/6) of every type pair"""
    return (tab[1] / tab[0]) ** (1.0 / 6.0)


def _parts(tab, types, mutant):
    C6, C12, g = (np.asarray(v, dtype=np.float64) for v in tab)
    types = np.asarray(types, dtype=np.int64)
    D6 = C6 - np.outer(g, g)
    if mutant == "c6_for_delta":
        D6 = C6
    elif mutant == "delta_sign":
        D6 = -D6
    look = C12.shape[0] - 1 - types if mutant == "types_permuted" else types
    return C12, D6, g[types], look


def pair_terms(tab, types, s, A, batch, r_c, pairs=None, sl=None, nimg=0, mutant=None):
    """(F [n, 3], U_R [B], U_delta [B], W [B, 3, 3]) of the table's pair sums over d = (ds - rint(ds) + n) A with 0 < |d| < r_c:
    U_R = 1/2 sum C12 / r^12, U_delta = 1/2 sum dC6 / r^6 (it enters the energy with a minus sign), F_i = sum_j (12 C12 / r^14 -
    6 dC6 / r^8) d and W the same slope with d d^T, halved.  The listed image (n = 0) of a listed pair is scaled by s^L inside
    the sums.  512 rows at a time."""
    C12, D6, _, look = _parts(tab, types, mutant)
    s = np.asarray(s, dtype=np.float64)
    A = np.asarray(A, dtype=np.float64)
    n = s.shape[0]
    scale = np.ones((n, n))
    if pairs is not None and len(pairs):
        pairs, _, wl = le._lists(pairs, 0.0, sl)
        scale[pairs[:, 0], pairs[:, 1]] = scale[pairs[:, 1], pairs[:, 0]] = 1.0 - wl
    sets = dr._sets(batch, n)
    F, UR, UD, W = np.zeros((n, 3)), np.zeros(len(sets)), np.zeros(len(sets)), np.zeros((len(sets), 3, 3))
    for b, sel in enumerate(sets):
        for r0 in range(0, sel.size, 512):
            rows = sel[r0:r0 + 512]
            ds = s[rows][:, None, :] - s[sel][None, :, :]
            ds = ds - np.rint(ds)
            c12, d6 = C12[np.ix_(look[rows], look[sel])], D6[np.ix_(look[rows], look[sel])]
            for sh in itertools.product(range(-nimg, nimg + 1), repeat=3):
                d = (ds + np.array(sh, dtype=np.float64)) @ A
                rr = (d * d).sum(-1)
                ok = (rr > 0) & (rr < r_c * r_c)
                ir2 = np.where(ok, 1.0 / np.where(ok, rr, 1.0), 0.0)
                listed = scale[np.ix_(rows, sel)] if sh == (0, 0, 0) else 1.0
                w12 = c12 * listed
                w6 = d6 * (1.0 if mutant == "delta_unscaled" else listed)
                UR[b] += 0.5 * (w12 * ir2 ** 6).sum()
                UD[b] += 0.5 * (w6 * ir2 ** 3).sum()
                gd = (12.0 * w12 * ir2 ** 7 - 6.0 * w6 * ir2 ** 4)[:, :, None] * d
                F[rows] += gd.sum(1)
                W[b] += 0.5 * np.einsum("ija,ijb->ab", gd, d)
    return F, UR, UD, W


def exact_lj_table_step(q, tab, types, s, A, batch, alpha_c, alpha_d, r_c, N, pairs=None, sc=None, sl=None, mutant=None):
    """(F [n, 3], U_coulomb [B], U_lj [B], W [B, 3, 3]) of the truncated algorithm in float64; with `pairs` the exclusions"""
    c = _parts(tab, types, None)[2]
    z = np.zeros(c.shape[0])
    if pairs is None:
        F, UC, ULJ, W = lj.exact_lj_step(q, c, z, s, A, batch, alpha_c, alpha_d, r_c, N)
    else:
        F, UC, ULJ, W = le.exact_lj_excl_step(q, c, z, s, A, batch, pairs, sc, sl, alpha_c, alpha_d, r_c, N)
    pF, UR, UD, pW = pair_terms(tab, types, s, A, batch, r_c, pairs, sl, 0, mutant)
    return F + pF, UC, ULJ + UR - UD, W + pW


def converged_lj_table_step(q, tab, types, s, A, r_c, pairs=None, sc=None, sl=None, R=None):
    """the same of one point set from sums carried to convergence -- the converged Coulomb sum, the lattice sum of c_i c_j / r^6
    (brute force over every image within R if given) -- and the table's terms summed directly within r_c over one shell of
    images; and the four energies (U_C, U_D, U_R, U_delta) apart"""
    c = _parts(tab, types, None)[2]
    z = np.zeros(c.shape[0])
    if pairs is None:
        F, UC, ULJ, W, _ = lj.converged_lj_step(q, c, z, s, A, r_c, R=R)
    else:
        F, UC, ULJ, W, _ = le.converged_lj_excl_step(q, c, z, s, A, r_c, pairs, sc, sl)
    pF, UR, UD, pW = pair_terms(tab, types, s, A, None, r_c, pairs, sl, 1)
    return F + pF, UC, ULJ + UR - UD, W + pW, (UC, -ULJ, UR, UD)


def converged_energy(q, tab, types, s, A, r_c):
    """U = U_C - U_D + U_R - U_delta of one point set without exclusions: smooth in s and A except where a pair crosses r_c"""
    c = _parts(tab, types, None)[2]
    _, UR, UD, _ = pair_terms(tab, types, s, A, None, r_c, nimg=1)
    return lj.converged_energy(q, c, np.zeros(c.shape[0]), s, A, r_c) + UR[0] - UD[0]


def near_table_step(q, tab, types, s, A, batch, alpha_c, alpha_d, r_c, pairs=None, sc=None, sl=None):
    """(f [n, 3], eight [B, 8]) of the pair walk by brute force: lj_excl_ref.near_step_scaled on (q, c, 0) plus the table's
    terms, every listed pair scaled inside the sums"""
    c = _parts(tab, types, None)[2]
    none = pairs is None
    f, eight = le.near_step_scaled(q, c, np.zeros(c.shape[0]), s, A, batch, np.zeros((0, 2), np.int64) if none else pairs,
                                   0.0 if none else sc, 0.0 if none else sl, alpha_c, alpha_d, r_c)
    pF, UR, UD, pW = pair_terms(tab, types, s, A, batch, r_c, pairs, sl)
    return f + pF, eight + lj.eight(np.zeros_like(UR), UR - UD, pW)


# ---- points and types --------------------------------------------------------------------------------------------------

def box_stretch(A):
    """the smallest factor by which the box A stretches a fractional length"""
    return float(np.linalg.svd(np.asarray(A, dtype=np.float64), compute_uv=False).min())


def draw_types(rng, n, T, unused=()):
    """n types out of [0, T) without those in `unused`, every other one present"""
    live = np.array([t for t in range(T) if t not in unused])
    types = live[rng.integers(0, live.size, n)]
    types[rng.permutation(n)[:live.size]] = live
    return types.astype(np.int64)


def type_parameters(rng, T, d_min):
    """(sigma [T], eps [T]): sigma between 0.5 and 0.8 d_min -- unlike sizes, or Lorentz-Berthelot and geometric mixing would
    agree -- with the two ends taken when T >= 2; eps in [0.5, 1.5)"""
    sigma = d_min * (0.5 + 0.3 * rng.random(T))
    if T >= 2:
        sigma[0], sigma[T - 1] = 0.8 * d_min, 0.5 * d_min
    return sigma, 0.5 + rng.random(T)


def check_types(tab, types, d_min):
    """asserts sigma(t, t') <= 0.8 d_min for every pair of types present"""
    present = np.unique(types)
    sig = sigma_of(tab)[np.ix_(present, present)]
    assert sig.max() <= 0.8 * d_min * (1 + 1e-12), (sig.max(), d_min)


def typed_lattice(rng, n, T, A, unused=(), rule=lorentz_berthelot):
    """(s [n, 3] float32, types [n], tab, d_min): lj_step_ref.lj_points with types drawn on top.  Asserted in the box's metric:
    no two distinct points closer than d_min (coincident ones are skipped by every sum), sigma(t, t') <= 0.8 d_min."""
    s = lj.lj_points(rng, n)
    d_min = lj.D_MIN_FRACTIONAL * box_stretch(A)
    s64 = s.astype(np.float64)
    for r0 in range(0, n, 512):
        ds = s64[r0:r0 + 512, None, :] - s64[None, :, :]
        d = (ds - np.rint(ds)) @ np.asarray(A, dtype=np.float64)
        r = np.sqrt((d * d).sum(-1))
        assert r[r > 0].min() >= d_min * (1 - 1e-5)
    types = draw_types(rng, n, T, unused)
    tab = rule(*type_parameters(rng, T, d_min))
    check_types(tab, types, d_min)
    return s, types, tab, d_min


def typed_bonded(rng, n, T, A, r_c, G=7, rule=lorentz_berthelot):
    """(s, types, tab, pairs, sc, sl, info): lj_excl_ref.bonded_points (which asserts that every pair that keeps any repulsion
    is at least info["d_min"] apart) with types drawn on top and sigma(t, t') <= 0.8 d_min asserted"""
    s, pairs, sc, sl, info = le.bonded_points(rng, n, A, r_c, G=G)
    types = draw_types(rng, n, T)
    tab = rule(*type_parameters(rng, T, info["d_min"]))
    check_types(tab, types, info["d_min"])
    return s, types, tab, pairs, sc, sl, info
