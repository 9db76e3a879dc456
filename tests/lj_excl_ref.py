"""Float64 restatement of the Lennard-Jones + Coulomb step with bonded-pair exclusions -- TEST
INFRASTRUCTURE ONLY.  ``nfft_ewald_lj_excl_step`` is ``lj_step_ref`` minus the listed terms, which are written here directly
from their formulas: the ``r = 0`` branch and the repulsion's cut at ``r_c`` included.  A plain module like lj_step_ref.py;
positions are FRACTIONAL, ``A`` holds the lattice vectors as rows.

A list is ``pairs`` [m, 2] (unordered, each once) with two scales per pair, ``sc`` for Coulomb and ``sl`` for both powers of
the Lennard-Jones term; ``w = 1 - s``; ``d_ij = (ds - rint(ds)) A`` is the one image that a listed pair refers to.

``mutant`` evaluates a deliberately wrong formula: ``"repulsion_unscaled"`` leaves the listed pairs' ``r^-12`` terms in,
``"all_images"`` removes every image of a listed pair within one shell instead of the one, ``"constant_sign"`` has the
``alpha_D^6 / 6`` constant of a coincident pair with the wrong sign.
"""
import itertools
import math

import numpy as np
from scipy.special import erf, erfc

import dispersion_ref as dr
import exclusions_ref as xr
import lj_step_ref as lj

SERIES_SWITCH, SERIES_TERMS = 0.125, 8  # of csrc/ewald_lj_excl.hip


def _lists(pairs, sc, sl):
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    m = pairs.shape[0]
    return pairs, 1.0 - np.broadcast_to(np.asarray(sc, dtype=np.float64), (m,)), 1.0 - np.broadcast_to(np.asarray(sl, dtype=np.float64), (m,))


def _set_of(batch, pairs, n):
    B = 1 if batch is None else int(np.asarray(batch)[-1]) + 1
    which = np.zeros(pairs.shape[0], dtype=np.int64) if batch is None else np.asarray(batch)[pairs[:, 0]]
    return B, which


def _scatter(n, B, which, pairs, g, d, uC, uLJ):
    """pair terms to (F [n, 3], U_C [B], U_LJ [B], W [B, 3, 3]): F_i += g d, F_j -= g d, W += g d d^T"""
    F, UC, ULJ, W = np.zeros((n, 3)), np.zeros(B), np.zeros(B), np.zeros((B, 3, 3))
    np.add.at(F, pairs[:, 0], g[:, None] * d)
    np.add.at(F, pairs[:, 1], -g[:, None] * d)
    np.add.at(UC, which, uC)
    np.add.at(ULJ, which, uLJ)
    np.add.at(W, which, g[:, None, None] * d[:, :, None] * d[:, None, :])
    return F, UC, ULJ, W


def listed_terms(q, c, a, s, A, batch, pairs, sc, sl, alpha_c, alpha_d, r_c, mutant=None):
    """(F, U_C, U_LJ, W) that the listed pairs lose -- to SUBTRACT from the step without exclusions"""
    q, c, a = (np.asarray(v, dtype=np.float64) for v in (q, c, a))
    pairs, wc, wl = _lists(pairs, sc, sl)
    n = np.asarray(s).shape[0]
    B, which = _set_of(batch, pairs, n)
    i, j = pairs[:, 0], pairs[:, 1]
    qq, cc, aa = q[i] * q[j], c[i] * c[j], a[i] * a[j]
    d0 = xr.images(s, A, pairs)
    total = None
    shells = itertools.product((-1, 0, 1), repeat=3) if mutant == "all_images" else [(0, 0, 0)]
    for sh in shells:
        d = d0 + np.array(sh, dtype=np.float64) @ dr._box(A)
        r = np.sqrt((d * d).sum(-1))
        ok = r > 0
        rs = np.where(ok, r, 1.0)
        rep = (ok & (r < r_c)).astype(np.float64) * (0.0 if mutant == "repulsion_unscaled" else 1.0)
        zero = -1.0 if mutant == "constant_sign" else 1.0
        uC = wc * qq * np.where(ok, 1.0 / rs, 2.0 * alpha_c / math.sqrt(math.pi))
        uLJ = wl * np.where(ok, aa * rep / rs ** 12 - cc / rs ** 6, -zero * cc * alpha_d ** 6 / 6.0)
        g = np.where(ok, wc * qq / rs ** 3 + wl * (12.0 * aa * rep / rs ** 14 - 6.0 * cc / rs ** 8), 0.0)
        part = _scatter(n, B, which, pairs, g, d, uC, uLJ)
        total = part if total is None else tuple(t + p for t, p in zip(total, part))
    return total


def repulsion_scaled(a, s, A, batch, r_c, pairs, sl, nimg=0):
    """(F_R [n, 3], U_R [B], W_R [B, 3, 3]) of the repulsion with the listed image of a listed pair SCALED by s^L inside the sum,
    as lj.repulsion forms it otherwise: a bonded pair's a_i a_j / r^12 is 5e5 x 4 eps at r = sigma / 3, and taking it out of a
    float64 sum afterwards would leave 1e-10 of it, which is not small against the gates of a float32 kernel"""
    a = np.asarray(a, dtype=np.float64)
    s = np.asarray(s, dtype=np.float64)
    A = np.asarray(A, dtype=np.float64)
    n = s.shape[0]
    pairs, _, wl = _lists(pairs, 0.0, sl)
    scale = np.ones((n, n))
    scale[pairs[:, 0], pairs[:, 1]] = scale[pairs[:, 1], pairs[:, 0]] = 1.0 - wl
    sets = dr._sets(batch, n)
    F, U, W = np.zeros((n, 3)), np.zeros(len(sets)), np.zeros((len(sets), 3, 3))
    for b, sel in enumerate(sets):
        if sel.size == 0:
            continue
        ds = s[sel][:, None, :] - s[sel][None, :, :]
        ds = ds - np.rint(ds)
        aa = np.outer(a[sel], a[sel])
        for sh in itertools.product(range(-nimg, nimg + 1), repeat=3):
            d = (ds + np.array(sh, dtype=np.float64)) @ A
            rr = (d * d).sum(-1)
            ok = (rr > 0) & (rr < r_c * r_c)
            ir2 = np.where(ok, 1.0 / np.where(ok, rr, 1.0), 0.0)
            w = aa * (scale[np.ix_(sel, sel)] if sh == (0, 0, 0) else 1.0)
            U[b] += 0.5 * (w * ir2 ** 6).sum()
            g = 12.0 * w * ir2 ** 7
            F[sel] += np.einsum("ij,ija->ia", g, d)
            W[b] += 0.5 * np.einsum("ij,ija,ijb->ab", g, d, d, optimize=True)
    return F, U, W


def _assemble(whole, q, c, a, s, A, batch, pairs, sc, sl, alpha_c, alpha_d, r_c, mutant, nimg):
    """the step of (q, c) alone minus its listed terms, plus the scaled repulsion"""
    z = np.zeros(np.asarray(s).shape[0])
    F, UC, ULJ, W = whole
    lF, lUC, lULJ, lW = listed_terms(q, c, z, s, A, batch, pairs, sc, sl, alpha_c, alpha_d, r_c, mutant)
    rF, rU, rW = repulsion_scaled(a, s, A, batch, r_c, pairs, 1.0 if mutant == "repulsion_unscaled" else sl, nimg)
    return F - lF + rF, UC - lUC, ULJ - lULJ + rU, W - lW + rW, rU


def exact_lj_excl_step(q, c, a, s, A, batch, pairs, sc, sl, alpha_c, alpha_d, r_c, N, mutant=None):
    """(F [n, 3], U_coulomb [B], U_lj [B], W [B, 3, 3]) of the truncated algorithm in float64 with the exclusions: the Coulomb
    and dispersion sums minus their listed terms (listed_terms: bounded multiples of what stays), the repulsion scaled inside"""
    z = np.zeros(np.asarray(s).shape[0])
    whole = lj.exact_lj_step(q, c, z, s, A, batch, alpha_c, alpha_d, r_c, N)
    return _assemble(whole, q, c, a, s, A, batch, pairs, sc, sl, alpha_c, alpha_d, r_c, mutant, 0)[:4]


def converged_lj_excl_step(q, c, a, s, A, r_c, pairs, sc, sl, alpha_c=6.0, alpha_d=3.2):
    """the same with the two lattice sums carried to convergence (alpha: those of lj.converged_lj_step's sums, which set the
    constants of a coincident pair), and the corrected energies (U_C, U_D, U_R) apart"""
    z = np.zeros(np.asarray(s).shape[0])
    F, UC, ULJ, W, _ = lj.converged_lj_step(q, c, z, s, A, r_c)
    F, UC, ULJ, W, UR = _assemble((F, UC, ULJ, W), q, c, a, s, A, None, pairs, sc, sl, alpha_c, alpha_d, r_c, None, 1)
    return F, UC, ULJ, W, (UC, UR - ULJ, UR)


# ---- the smooth parts that the far field holds ---------------------------------------------------------------------------

def _series(coef, u):
    t = np.full_like(u, coef[-1])
    for k in range(len(coef) - 2, -1, -1):
        t = coef[k] - u * t
    return t


def series_tables(terms):
    """the coefficients of (-u)^k in erf(x) / x and (erf(x) / x - e^-u) / u over 2 / sqrt(pi), and in h(u) and -h'(u), u = x^2"""
    f = math.factorial
    return ([1.0 / (f(k) * (2 * k + 1)) for k in range(terms)], [2.0 * (k + 1) / (2 * k + 3) / f(k + 1) for k in range(terms)],
            [0.5 / (f(k) * (k + 3)) for k in range(terms)], [0.5 / (f(k) * (k + 4)) for k in range(terms)])


def smooth_closed(r, alpha_c, alpha_d):
    """(S_C, T_C, S_D, T_D) from the closed forms in float64, r > 0"""
    r = np.asarray(r, dtype=np.float64)
    slope = 2.0 * alpha_c / math.sqrt(math.pi)
    SC = erf(alpha_c * r) / r
    TC = (SC - slope * np.exp(-(alpha_c * r) ** 2)) / (r * r)
    u = (alpha_d * r) ** 2
    e = np.exp(-u)
    h = (1.0 - e * (1.0 + u + 0.5 * u * u)) / u ** 3
    return SC, TC, alpha_d ** 6 * h, alpha_d ** 8 * (6.0 * h - e) / u


def smooth_series(r, alpha_c, alpha_d, terms):
    """the same from `terms` terms of the series at r = 0"""
    r = np.asarray(r, dtype=np.float64)
    c0, c1, h0, h1 = series_tables(terms)
    slope = 2.0 * alpha_c / math.sqrt(math.pi)
    uc, ud = (alpha_c * r) ** 2, (alpha_d * r) ** 2
    return slope * _series(c0, uc), slope * alpha_c ** 2 * _series(c1, uc), alpha_d ** 6 * _series(h0, ud), 2.0 * alpha_d ** 8 * _series(h1, ud)


def smooth_parts(r, alpha_c, alpha_d, switch=0.5, terms=30):
    """(S_C, T_C, S_D, T_D) [m] in float64 for r >= 0: S_C = erf(alpha_C r) / r, T_C = -S_C' / r, S_D = 1 / r^6 - w_D(r),
    T_D = -S_D' / r.  Thirty terms of the series below u = alpha^2 r^2 = 1/2 (exact to float64 there), the closed forms above:
    neither the kernel's switch point nor its number of terms"""
    r = np.asarray(r, dtype=np.float64)
    rs = np.where(r > 0, r, 1.0)
    cl, se = smooth_closed(rs, alpha_c, alpha_d), smooth_series(r, alpha_c, alpha_d, terms)
    low = [(alpha_c * r) ** 2 < switch] * 2 + [(alpha_d * r) ** 2 < switch] * 2
    return tuple(np.where(lo, s_, c_) for lo, s_, c_ in zip(low, se, cl))


def list_step(q, c, s, A, batch, pairs, sc, sl, alpha_c, alpha_d, r_c):
    """(f [n, 3], eight [B, 8]) of the list kernel, to ADD to the pair walk's: minus the smooth share of the listed pairs
    with r < r_c (r = 0 included), minus their whole Coulomb and dispersion terms beyond"""
    q, c = (np.asarray(v, dtype=np.float64) for v in (q, c))
    pairs, wc, wl = _lists(pairs, sc, sl)
    n = np.asarray(s).shape[0]
    B, which = _set_of(batch, pairs, n)
    d = xr.images(s, A, pairs)
    r = np.sqrt((d * d).sum(-1))
    SC, TC, SD, TD = smooth_parts(r, alpha_c, alpha_d)
    far = r >= r_c
    rs = np.where(far, r, 1.0)
    SC, TC = np.where(far, 1.0 / rs, SC), np.where(far, 1.0 / rs ** 3, TC)
    SD, TD = np.where(far, 1.0 / rs ** 6, SD), np.where(far, 6.0 / rs ** 8, TD)
    wqq, wcc = wc * q[pairs[:, 0]] * q[pairs[:, 1]], wl * c[pairs[:, 0]] * c[pairs[:, 1]]
    g = wcc * TD - wqq * TC
    F, UC, ULJ, W = _scatter(n, B, which, pairs, g, d, -wqq * SC, wcc * SD)
    return F, lj.eight(UC, ULJ, W)


def near_step_scaled(q, c, a, s, A, batch, pairs, sc, sl, alpha_c, alpha_d, r_c):
    """(f [n, 3], eight [B, 8]) of the masked pair walk by brute force: every pair 0 < r < r_c with its terms SCALED -- q_i q_j
    by s^C, c_i c_j and a_i a_j by s^L, one for an unlisted pair -- and nothing subtracted (512 rows at a time)"""
    q, c, a = (np.asarray(v, dtype=np.float64) for v in (q, c, a))
    s = np.asarray(s, dtype=np.float64)
    n = s.shape[0]
    pairs, wc, wl = _lists(pairs, sc, sl)
    SCm, SLm = np.ones((n, n)), np.ones((n, n))
    for m_, w in ((SCm, wc), (SLm, wl)):
        m_[pairs[:, 0], pairs[:, 1]] = 1.0 - w
        m_[pairs[:, 1], pairs[:, 0]] = 1.0 - w
    sets = dr._sets(batch, n)
    f, out = np.zeros((n, 3)), np.zeros((len(sets), 8))
    slope = 2.0 * alpha_c / math.sqrt(math.pi)
    for b, sel in enumerate(sets):
        for r0 in range(0, sel.size, 512):
            rows = sel[r0:r0 + 512]
            ds = s[rows][:, None, :] - s[sel][None, :, :]
            d = (ds - np.rint(ds)) @ dr._box(A)
            rr = (d * d).sum(-1)
            ok = (rr > 0) & (rr < r_c * r_c)
            r2 = np.where(ok, rr, 1.0)
            r = np.sqrt(r2)
            qq = SCm[np.ix_(rows, sel)] * np.outer(q[rows], q[sel]) * ok
            cc = SLm[np.ix_(rows, sel)] * np.outer(c[rows], c[sel]) * ok
            p = SLm[np.ix_(rows, sel)] * np.outer(a[rows], a[sel]) * ok / r2 ** 6
            wC = erfc(alpha_c * r) / r
            mgC = (wC + slope * np.exp(-alpha_c ** 2 * r2)) / r2
            a2 = alpha_d ** 2 * r2
            e = np.exp(-a2)
            w6 = e * (1.0 + a2 + 0.5 * a2 * a2) / r2 ** 3
            mg6 = e * (6.0 + 6.0 * a2 + 3.0 * a2 ** 2 + a2 ** 3) / r2 ** 4
            g = qq * mgC - cc * mg6 + 12.0 * p / r2
            gd = g[:, :, None] * d
            f[rows] = gd.sum(1)
            W = 0.5 * np.einsum("ija,ijb->ab", gd, d)
            out[b] += [0.5 * (qq * wC).sum(), 0.5 * (p - cc * w6).sum(), W[0, 0], W[1, 1], W[2, 2], W[1, 2], W[0, 2], W[0, 1]]
    return f, out


# ---- points --------------------------------------------------------------------------------------------------------------

AMBER_14 = (1.0 / 1.2, 0.5)  # the scales of a 1-4 pair: Coulomb, Lennard-Jones
SPECIAL_POINTS = 32          # hub 21, faces 6, coincident 2, beyond the cut 2, the far index 1


def _rotation(rng):
    qm, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return qm


def bonded_points(rng, n, A, r_c, G=7):
    """n float32 FRACTIONAL points with a bonded topology for r^-12, on a jittered lattice of G^3 sites (spacing h = 1 / G, jitter
    0.014 h) in the box A; every length below is in units of h times the box's smallest stretch.  Returns
    (s [n, 3], pairs [m, 2], sc [m], sl [m], info) with info = {"sigma": the largest sigma of a point (0.35), "d_min": 0.4375,
    "tight": the indices [k, 2] of the tightest fully excluded bonds, "hub", "coincident", "beyond", "far_index"}.

    * water-like molecules of 3 atoms, bonds sigma / 3 at 104 degrees, every pair listed at scale 0 -- the tightest bonds;
    * chains of 4 atoms, all intramolecular pairs listed: 1-2 and 1-3 at scale 0, 1-4 at (1 / 1.2, 1 / 2).  A 1-4 pair keeps half
      its repulsion and must therefore be d_min = 1.25 sigma apart, which three bonds of sigma / 3 cannot span: the chains'
      bonds are 0.45 sigma (a carbon chain's: 1.53 A against sigma = 3.4 A), nearly straight, 1-4 at 1.33 sigma;
    * a hub with 20 partners within 0.25 and no two closer than 0.09, every pair among the 21 listed at scale 0 (rows of 20
      entries);
    * a listed pair through each face: axis 0 a bond of sigma / 3 at scale 0, axes 1 and 2 at 1.3 sigma with the 1-4 scales;
    * a coincident listed pair at scale 0; a listed pair farther apart than r_c, at (0.5, 0.25);
    * point 0 (an atom of the first molecule) listed with point n - 1, a single atom on the neighbouring site, at (0.5, 0.5):
      the row of point 0 spans nearly all indices, and the search must miss for every unlisted neighbour;
    * sixteen atoms of molecules given one box to the right or two boxes to the left of where they act;
    * single atoms on further sites make up n.

    Asserted here, in the box's metric: every pair that keeps any repulsion (unlisted, or s^L > 0) is at least d_min apart
    (sigma <= 0.8 d_min); the far pair is beyond r_c and the others within; no listed pair is within 1e-4 r_c of r_c."""
    A = np.asarray(A, dtype=np.float64)
    inv = np.linalg.inv(A)
    h = 1.0 / G
    unit = h * np.linalg.svd(A, compute_uv=False).min()  # Cartesian length of one unit
    sigma, d_min = 0.35 * unit, 0.4375 * unit
    centre = lambda k: (np.asarray(k, dtype=np.float64) + 0.5) / G - 0.5
    jitter = lambda: (rng.random(3) * 2.0 - 1.0) * 0.014 * h
    mid = G // 2
    reserved = {}
    for ax in range(3):  # the two sites on either side of the face, on a line of their own
        k = [1 + ax, 2 + ax, 3 + ax]
        for end in (0, G - 1):
            k[ax] = end
            reserved[tuple(k)] = "face"
    far = int(round(0.43 * G))
    named = {"first": (mid, mid, mid), "last": (mid + 1, mid, mid), "hub": (mid, mid + 2, mid), "coincident": (mid, mid, mid + 2),
             "beyond0": (0, 0, 1), "beyond1": (far, far, 1 + far)}
    for name, k in named.items():
        assert k not in reserved
        reserved[k] = name
    free = [k for k in itertools.product(range(G), repeat=3) if k not in reserved]
    free = [free[t] for t in rng.permutation(len(free))]
    avail = n - SPECIAL_POINTS
    chains, waters = avail // 9, avail // 6
    singles = avail - 4 * chains - 3 * waters
    assert singles >= 0 and chains + waters + singles <= len(free) + 1
    pts, pairs, sc, sl, tight = [], [], [], [], []

    def add_pair(i, j, scales):
        pairs.append((i, j))
        sc.append(scales[0])
        sl.append(scales[1])

    def molecule(site, shape, scales_of):
        """atoms at site + shape (Cartesian, centred), all pairs listed with scales_of(topological distance)"""
        first = len(pts)
        shape = (shape - shape.mean(0)) @ _rotation(rng).T
        for p in shape:
            pts.append(site + p @ inv)
        for u in range(len(shape)):
            for v in range(u + 1, len(shape)):
                add_pair(first + (v if (u + v) % 2 else u), first + (u if (u + v) % 2 else v), scales_of(u, v))  # (either order)
        return first

    b3, b4 = sigma / 3.0, 0.45 * sigma
    t = math.radians(104.0)
    water = np.array([[0.0, 0.0, 0.0], [b3, 0.0, 0.0], [b3 * math.cos(t), b3 * math.sin(t), 0.0]])
    z = math.radians(20.0)
    chain = np.cumsum(np.array([[0.0, 0.0, 0.0], [b4, 0.0, 0.0], [b4 * math.cos(z), b4 * math.sin(z), 0.0], [b4, 0.0, 0.0]]), 0)
    sites = iter(free)
    # point 0: an atom of the first molecule, on its named site
    kinds = ["chain"] * chains + ["water"] * waters
    kinds = [kinds[t_] for t_ in rng.permutation(len(kinds))]
    moved = []
    for m_, kind in enumerate(kinds):
        site = centre(named["first"] if m_ == 0 else next(sites)) + jitter()
        if kind == "water":
            first = molecule(site, water, lambda u, v: (0.0, 0.0))
            tight += [(first, first + 1), (first, first + 2)]
        else:
            first = molecule(site, chain, lambda u, v: AMBER_14 if v - u == 3 else (0.0, 0.0))
        if 2 <= m_ < 10:
            moved.append((first + 1, 1.0))
        elif 10 <= m_ < 18:
            moved.append((first, -2.0))
    info = {"sigma": sigma, "d_min": d_min}
    # the hub and its 20 partners
    site = centre(named["hub"]) + jitter()
    hub = len(pts)
    cluster = []
    while len(cluster) < 21:  # (no two closer than 0.09: the float64 restatement subtracts their r^-12 terms)
        e = rng.standard_normal(3)
        p = 0.25 * unit * rng.random() ** (1.0 / 3.0) * e / np.linalg.norm(e)
        if all(np.linalg.norm(p - o) >= 0.09 * unit for o in cluster):
            cluster.append(p)
    pts += [site + p @ inv for p in cluster]
    for u in range(21):
        for v in range(u + 1, 21):
            add_pair(hub + u, hub + v, (0.0, 0.0))
    info["hub"] = hub
    # a pair through each face, along the fractional axis
    for ax in range(3):
        k = np.array([1.0 + ax, 2.0 + ax, 3.0 + ax])
        mid_face = centre(k)
        length = b3 if ax == 0 else 1.3 * sigma
        half = 0.5 * length / np.linalg.norm(A[ax])
        lo_, hi_ = mid_face.copy(), mid_face.copy()
        lo_[ax], hi_[ax] = 0.5 - half, -0.5 + half
        add_pair(len(pts), len(pts) + 1, (0.0, 0.0) if ax == 0 else AMBER_14)
        if ax == 0:
            tight.append((len(pts), len(pts) + 1))
        pts += [lo_, hi_]
    # a coincident pair
    site = centre(named["coincident"]) + jitter()
    add_pair(len(pts) + 1, len(pts), (0.0, 0.0))
    info["coincident"] = (len(pts), len(pts) + 1)
    pts += [site, site.copy()]
    # a listed pair beyond the cut
    add_pair(len(pts), len(pts) + 1, (0.5, 0.25))
    info["beyond"] = (len(pts), len(pts) + 1)
    pts += [centre(named["beyond0"]) + jitter(), centre(named["beyond1"]) + jitter()]
    for _ in range(singles):
        pts.append(centre(next(sites)) + jitter())
    pts.append(centre(named["last"]) + jitter())
    assert len(pts) == n
    add_pair(n - 1, 0, (0.5, 0.5))
    info["far_index"] = (0, n - 1)
    s = np.array(pts)
    s -= np.rint(s)
    for i, shift in moved:
        s[i] += shift
    s = s.astype(np.float32)
    pairs, sc, sl = np.array(pairs, dtype=np.int64), np.array(sc), np.array(sl)
    info["tight"] = np.array(tight, dtype=np.int64)
    # the assertions, on the float32 positions
    r = check_separation(s, A, pairs, sl, d_min * (1 - 1e-5))
    rl = r[pairs[:, 0], pairs[:, 1]]
    assert np.abs(rl - r_c).min() > 1e-4 * r_c
    beyond = rl >= r_c
    assert beyond.sum() == 1 and tuple(pairs[beyond][0]) == info["beyond"]
    assert (rl == 0).sum() == 1 and rl[(pairs[:, 0] == n - 1)][0] < r_c
    rt = r[info["tight"][:, 0], info["tight"][:, 1]]
    assert np.abs(rt / b3 - 1).max() < 1e-3
    return s, pairs, sc, sl, info


def check_separation(s, A, pairs, sl, least):
    """asserts that every pair that keeps any repulsion (unlisted, or s^L > 0) is at least `least` apart in the box A; returns
    the distances [n, n] of the minimum images"""
    s64 = np.asarray(s, dtype=np.float64)
    n = s64.shape[0]
    r = np.empty((n, n))
    for r0 in range(0, n, 512):
        ds = s64[r0:r0 + 512, None, :] - s64[None, :, :]
        d = (ds - np.rint(ds)) @ np.asarray(A, dtype=np.float64)
        r[r0:r0 + 512] = np.sqrt((d * d).sum(-1))
    keeps = np.ones((n, n), dtype=bool)
    off = pairs[np.asarray(sl) == 0.0]
    keeps[off[:, 0], off[:, 1]] = keeps[off[:, 1], off[:, 0]] = False
    keeps[np.arange(n), np.arange(n)] = False
    assert r[keeps].min() >= least, (r[keeps].min(), least)
    return r


def coefficients(rng, n, info):
    """(q, c, a) float32: standard normal charges, sigma in [0.95, 1] x info["sigma"] (<= 0.8 d_min), epsilon in [0.5, 1.5)"""
    sigma, eps = info["sigma"] * (0.95 + 0.05 * rng.random(n)), 0.5 + rng.random(n)
    c, a = lj.lj_coefficients(sigma, eps)
    return rng.standard_normal(n).astype(np.float32), c.astype(np.float32), a.astype(np.float32)
