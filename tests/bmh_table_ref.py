"""Float64 restatement of the Buckingham / Born-Mayer-Huggins + Coulomb step with per-type-pair parameters (DESIGN.md section
7u) -- TEST INFRASTRUCTURE ONLY.  ``nfft_ewald_bmh_table_step`` is ``lj_step_ref`` / ``lj_excl_ref`` for ``(q, c)`` with no
repulsion coefficient, ``c_i = g[t_i]`` the grid's per-type coefficient, plus the direct sums over the minimum images with
``0 < r < r_c`` of ``A e^(-B r)``, ``dC6 / r^6`` and ``C8 / r^8`` of the two types, ``dC6 = C6 - outer(g, g)``.  The listed image of
a listed pair is scaled by ``s^L`` INSIDE those sums, not subtracted afterwards.  A plain module like lj_table_ref.py;
positions are FRACTIONAL, ``A`` (the box) holds the lattice vectors as rows.

A parameter set is ``tab = (PA [T, T], PB [T, T], C6 [T, T], C8 [T, T], g [T])`` for the pair energy
``PA e^(-PB r) - C6 / r^6 - C8 / r^8``.

``mutant`` evaluates a deliberately wrong formula: ``"slope_without_b"`` leaves ``B`` out of the exponential's slope (``A e^(-B r)
/ r`` for ``A B e^(-B r) / r``), ``"c8_sign"`` adds ``C8 / r^8`` and its slope instead of subtracting them, ``"six_for_eight"`` gives
the ``C8`` term the slope factor 6, ``"a_unscaled"`` leaves the scale ``s^L`` of a listed pair off ``A``.
"""
import itertools

import numpy as np

import dispersion_ref as dr
import lj_excl_ref as le
import lj_step_ref as lj
from lj_table_ref import box_stretch, draw_types  # noqa: F401  (the same boxes and type draws as section 7t)


def _parts(tab, types):
    PA, PB, C6, C8, g = (np.asarray(v, dtype=np.float64) for v in tab)
    types = np.asarray(types, dtype=np.int64)
    return PA, PB, C6 - np.outer(g, g), C8, g[types], types


def pair_terms(tab, types, s, A, batch, r_c, pairs=None, sl=None, nimg=0, mutant=None):
    """(F [n, 3], U_A [B], U_delta [B], U_8 [B], W [B, 3, 3], half_ABr [B]) of the table's pair sums over d = (ds - rint(ds) + n) A
    with 0 < |d| < r_c: U_A = 1/2 sum A e^(-B r), U_delta = 1/2 sum dC6 / r^6, U_8 = 1/2 sum C8 / r^8 (the last two enter the energy
    with a minus sign), F_i = sum_j (A B e^(-B r) / r - 6 dC6 / r^8 - 8 C8 / r^10) d, W the same slope with d d^T, halved, and
    1/2 sum A B r e^(-B r) for the trace identity.  The listed image (n = 0) of a listed pair is scaled by s^L inside the sums.
    512 rows at a time."""
    PA, PB, D6, C8, _, look = _parts(tab, types)
    s = np.asarray(s, dtype=np.float64)
    A = np.asarray(A, dtype=np.float64)
    n = s.shape[0]
    scale = np.ones((n, n))
    if pairs is not None and len(pairs):
        pairs, _, wl = le._lists(pairs, 0.0, sl)
        scale[pairs[:, 0], pairs[:, 1]] = scale[pairs[:, 1], pairs[:, 0]] = 1.0 - wl
    sets = dr._sets(batch, n)
    B = len(sets)
    F, UA, UD, U8, W, HB = np.zeros((n, 3)), np.zeros(B), np.zeros(B), np.zeros(B), np.zeros((B, 3, 3)), np.zeros(B)
    sign8 = -1.0 if mutant == "c8_sign" else 1.0
    for b, sel in enumerate(sets):
        for r0 in range(0, sel.size, 512):
            rows = sel[r0:r0 + 512]
            ds = s[rows][:, None, :] - s[sel][None, :, :]
            ds = ds - np.rint(ds)
            ix = np.ix_(look[rows], look[sel])
            pa, pb, d6, c8 = PA[ix], PB[ix], D6[ix], C8[ix]
            for sh in itertools.product(range(-nimg, nimg + 1), repeat=3):
                d = (ds + np.array(sh, dtype=np.float64)) @ A
                rr = (d * d).sum(-1)
                ok = (rr > 0) & (rr < r_c * r_c)
                ir2 = np.where(ok, 1.0 / np.where(ok, rr, 1.0), 0.0)
                r = np.sqrt(np.where(ok, rr, 1.0))
                listed = scale[np.ix_(rows, sel)] if sh == (0, 0, 0) else 1.0
                wa = pa * (1.0 if mutant == "a_unscaled" else listed) * ok
                w6, w8 = d6 * listed, sign8 * c8 * listed
                ex = wa * np.exp(-pb * r)
                UA[b] += 0.5 * ex.sum()
                UD[b] += 0.5 * (w6 * ir2 ** 3).sum()
                U8[b] += 0.5 * (w8 * ir2 ** 4).sum()
                HB[b] += 0.5 * (ex * pb * r).sum()
                slope_a = ex / r if mutant == "slope_without_b" else ex * pb / r
                k8 = 6.0 if mutant == "six_for_eight" else 8.0
                gd = (slope_a - 6.0 * w6 * ir2 ** 4 - k8 * w8 * ir2 ** 5)[:, :, None] * d
                F[rows] += gd.sum(1)
                W[b] += 0.5 * np.einsum("ija,ijb->ab", gd, d)
    return F, UA, UD, U8, W, HB


def half_ABr(tab, types, s, A, batch, r_c, pairs=None, sl=None, nimg=0):
    """1/2 sum A B r e^(-B r) over the pairs of pair_terms: what the exponential adds to tr W beyond a homogeneous term's share"""
    return pair_terms(tab, types, s, A, batch, r_c, pairs, sl, nimg)[5]


def exact_bmh_table_step(q, tab, types, s, A, batch, alpha_c, alpha_d, r_c, N, pairs=None, sc=None, sl=None, mutant=None,
                         shares=True):
    """(F [n, 3], U_coulomb [B], U_sr [B], W [B, 3, 3]) of the truncated algorithm in float64; with `pairs` the exclusions.
    `shares`: assert check_shares on the result (a reference that a relative error is measured against)"""
    c = _parts(tab, types)[4]
    z = np.zeros(c.shape[0])
    if pairs is None:
        F, UC, ULJ, W = lj.exact_lj_step(q, c, z, s, A, batch, alpha_c, alpha_d, r_c, N)
    else:
        F, UC, ULJ, W = le.exact_lj_excl_step(q, c, z, s, A, batch, pairs, sc, sl, alpha_c, alpha_d, r_c, N)
    pF, UA, UD, U8, pW, _ = pair_terms(tab, types, s, A, batch, r_c, pairs, sl, 0, mutant)
    if shares and mutant is None:
        check_shares(UA, UD, U8, ULJ + UA - UD - U8, tab)
    return F + pF, UC, ULJ + UA - UD - U8, W + pW


def converged_bmh_table_step(q, tab, types, s, A, r_c, pairs=None, sc=None, sl=None, R=None):
    """the same of one point set from sums carried to convergence -- the converged Coulomb sum, the lattice sum of c_i c_j / r^6
    (brute force over every image within R if given) -- and the table's terms summed directly within r_c over one shell of
    images; and the energies (U_C, U_D, U_A, U_delta, U_8) and 1/2 sum A B r e^(-B r) apart"""
    c = _parts(tab, types)[4]
    z = np.zeros(c.shape[0])
    if pairs is None:
        F, UC, ULJ, W, _ = lj.converged_lj_step(q, c, z, s, A, r_c, R=R)
    else:
        F, UC, ULJ, W, _ = le.converged_lj_excl_step(q, c, z, s, A, r_c, pairs, sc, sl)
    pF, UA, UD, U8, pW, HB = pair_terms(tab, types, s, A, None, r_c, pairs, sl, 1)
    return F + pF, UC, ULJ + UA - UD - U8, W + pW, (UC, -ULJ, UA, UD, U8, HB)


def converged_energy(q, tab, types, s, A, r_c):
    """U = U_C - U_D + U_A - U_delta - U_8 of one point set without exclusions: smooth in s and A except where a pair crosses r_c"""
    c = _parts(tab, types)[4]
    _, UA, UD, U8, _, _ = pair_terms(tab, types, s, A, None, r_c, nimg=1)
    return lj.converged_energy(q, c, np.zeros(c.shape[0]), s, A, r_c) + UA[0] - UD[0] - U8[0]


def near_bmh_step(q, tab, types, s, A, batch, alpha_c, alpha_d, r_c, pairs=None, sc=None, sl=None, c=None, shares=True):
    """(f [n, 3], eight [B, 8]) of the pair walk by brute force: lj_excl_ref.near_step_scaled on (q, c, 0) plus the table's
    terms, every listed pair scaled inside the sums.  `c` replaces g[types] (zeros: the walk of dispersion=None).  `shares`:
    assert check_shares on the second energy"""
    c = _parts(tab, types)[4] if c is None else np.asarray(c, dtype=np.float64)
    none = pairs is None
    f, eight = le.near_step_scaled(q, c, np.zeros(c.shape[0]), s, A, batch, np.zeros((0, 2), np.int64) if none else pairs,
                                   0.0 if none else sc, 0.0 if none else sl, alpha_c, alpha_d, r_c)
    pF, UA, UD, U8, pW, _ = pair_terms(tab, types, s, A, batch, r_c, pairs, sl)
    eight = eight + lj.eight(np.zeros_like(UA), UA - UD - U8, pW)
    if shares:
        check_shares(UA, UD, U8, eight[:, 1], tab)
    return f + pF, eight


# ---- parameters and points ----------------------------------------------------------------------------------------------

def exp6_parameters(rng, T, d_min):
    """tab of the exp-6 form u = eps / (1 - 6 / a) [(6 / a) e^(a (1 - r / r_m)) - (r_m / r)^6] with a C8 term on top: per type r_m
    between 0.7 and 1.0 d_min -- unlike sizes, with the two ends taken when T >= 2 and the upper one at T = 1 -- eps in [0.5, 1.5) and a between 12 and 14;
    r_m and a mixed arithmetically, eps geometrically; B = a / r_m, A = 6 eps e^a / (a - 6), C6 = eps a r_m^6 / (a - 6),
    C8 = 0.3 C6 r_m^2, g = sqrt(diag(C6)).  The minimum of the pair energy is near r_m <= d_min and its maximum (the turnover)
    near 0.2 r_m."""
    rm = d_min * (0.7 + 0.3 * rng.random(T))
    rm[0] = 1.0 * d_min  # (a single type takes the large end: the exponential keeps a visible share of the energy)
    if T >= 2:
        rm[T - 1] = 0.7 * d_min
    eps, a = 0.5 + rng.random(T), 12.0 + 2.0 * rng.random(T)
    rm = 0.5 * (rm[:, None] + rm[None, :])
    a = 0.5 * (a[:, None] + a[None, :])
    e = np.sqrt(eps[:, None] * eps[None, :])
    C6 = e * a * rm ** 6 / (a - 6.0)
    return 6.0 * e * np.exp(a) / (a - 6.0), a / rm, C6, 0.3 * C6 * rm ** 2, np.sqrt(np.diag(C6))


def to_float32(tab):
    """the table as the device holds it: (A, B, dC6, C8) and the grid coefficient rounded to float32, then float64 again --
    the restatement takes the kernel's parameters, as it takes its float32 positions"""
    PA, PB, C6, C8, g = (np.asarray(v, dtype=np.float64) for v in tab)
    r32 = lambda v: v.astype(np.float32).astype(np.float64)
    g32 = r32(g)
    return r32(PA), r32(PB), r32(C6 - np.outer(g, g)) + np.outer(g32, g32), r32(C8), g32


def check_shares(UA, UD, U8, U_sr, tab=None):
    """asserts, set by set, that each of the three table energies is at least 1e-3 of their sum of magnitudes -- a dropped
    term would show -- and that |U_sr| is at least 0.1 of it: a relative error is not inflated by cancellation.  A term whose
    table is zero up to the rounding of float32 (dC6 of a single type with g = sqrt(C6)) is exempt: there is nothing to drop."""
    for b in range(len(UA)):
        size = abs(UA[b]) + abs(UD[b]) + abs(U8[b])
        if size == 0.0:  # an empty set
            continue
        zero_delta = tab is not None and np.abs(_parts(tab, [0])[2]).max() <= 1e-6 * np.abs(np.asarray(tab[2])).max()
        for name, u in (("U_A", UA[b]), ("U_delta", UD[b]), ("U_8", U8[b])):
            if name == "U_delta" and zero_delta:
                continue
            assert abs(u) >= 1e-3 * size, (name, b, u, size)
        assert U_sr is None or abs(U_sr[b]) >= 0.1 * size, (b, U_sr[b], size)


def check_system(tab, types, s, A, batch, r_c, d_min, pairs=None, sl=None):
    """the builder's assertions in the box's metric: no two points that keep any short-range term closer than d_min (the
    coincident and the fully excluded ones are skipped by every sum) and each table energy's share of check_shares.  The
    share of U_sr itself is asserted where U_sr is formed, by near_bmh_step and exact_bmh_table_step on what they return."""
    none = pairs is None
    sets = dr._sets(batch, np.asarray(s).shape[0])
    for sel in sets:
        if not sel.size:
            continue
        inside = np.full(np.asarray(s).shape[0], -1)
        inside[sel] = np.arange(sel.size)
        if none:
            p, w = np.zeros((0, 2), np.int64), np.zeros(0)
        else:
            keep = np.isin(np.asarray(pairs)[:, 0], sel)
            p, w = inside[np.asarray(pairs)[keep]], np.broadcast_to(np.asarray(sl, dtype=np.float64), (len(pairs),))[keep]
        s64 = np.asarray(s, dtype=np.float64)[sel]
        ds = s64[:, None, :] - s64[None, :, :]
        d = (ds - np.rint(ds)) @ np.asarray(A, dtype=np.float64)
        r = np.sqrt((d * d).sum(-1))
        keeps = r > 0
        off = p[w == 0.0]
        keeps[off[:, 0], off[:, 1]] = keeps[off[:, 1], off[:, 0]] = False
        assert r[keeps].min() >= d_min, (r[keeps].min(), d_min)
    _, UA, UD, U8, _, _ = pair_terms(tab, types, s, A, batch, r_c, pairs, sl)
    check_shares(UA, UD, U8, None, tab)
