"""Float64 restatement of the Lennard-Jones + Coulomb step -- TEST INFRASTRUCTURE ONLY.

``nfft_ewald_lj_step`` returns ``(F, U_coulomb, U_lj, W)`` of ``U = U_C + U_LJ`` with ``U_LJ = U_R - U_D``: the Coulomb Ewald
sum of the charges ``q``, the dispersion Ewald sum of the coefficients ``c`` (``C6_ij = c_i c_j``) and the repulsion
``U_R = 1/2 sum_ij a_i a_j / r_ij^12`` over the minimum images with ``0 < r_ij < r_c`` (``C12_ij = a_i a_j``), plainly
truncated.  The Coulomb and dispersion parts are compositions of the committed restatements (``ewald_box_ref``,
``ewald_virial_ref``, ``dispersion_ref``, ``dispersion_virial_ref``); new here are only the ``r^-12`` pair terms.  A plain module
like ewald_step_ref.py; positions are FRACTIONAL, ``A`` holds the lattice vectors as rows, one column.

``mutant`` evaluates a deliberately wrong formula: ``"dispersion_sign"`` adds the dispersion part instead of subtracting it,
``"six"`` has the factor 6 in place of 12 in the repulsion's slope, ``"no_self"`` leaves the dispersion sum's self term out of
``U_lj``.
"""
import itertools

import numpy as np

import dispersion_ref as dr
import dispersion_virial_ref as dv
import ewald_box_ref as eb
import ewald_virial_ref as ev


def lj_coefficients(sigma, epsilon):
    """(c, a) = (2 sqrt(eps) sigma^3, 2 sqrt(eps) sigma^6)"""
    sigma, epsilon = np.asarray(sigma, dtype=np.float64), np.asarray(epsilon, dtype=np.float64)
    return 2.0 * np.sqrt(epsilon) * sigma ** 3, 2.0 * np.sqrt(epsilon) * sigma ** 6


def repulsion(a, s, A, batch, r_c, nimg=0, slope=12.0):
    """(rho [n], H [n, 3], U_R [B], W_R [B, 3, 3]): rho_i = sum_j a_j / r^12, H_i = sum_j slope a_j d / r^14,
    U_R = 1/2 sum_i a_i rho_i, W_R = 1/2 sum_ij a_i a_j slope d_a d_b / r^14 over d = (ds - rint(ds) + n) A with
    0 < |d| < r_c (`nimg` shells of images n: within r_c <= w / 3 only n = 0 contributes)"""
    a = np.asarray(a, dtype=np.float64)
    s = np.asarray(s, dtype=np.float64)
    A = np.asarray(A, dtype=np.float64)
    sets = dr._sets(batch, s.shape[0])
    rho, H = np.zeros(s.shape[0]), np.zeros((s.shape[0], 3))
    U, W = np.zeros(len(sets)), np.zeros((len(sets), 3, 3))
    for b, sel in enumerate(sets):
        if sel.size == 0:
            continue
        ds = s[sel][:, None, :] - s[sel][None, :, :]
        ds = ds - np.rint(ds)
        for sh in itertools.product(range(-nimg, nimg + 1), repeat=3):
            d = (ds + np.array(sh, dtype=np.float64)) @ A
            rr = (d * d).sum(-1)
            ok = (rr > 0) & (rr < r_c * r_c)
            ir2 = np.where(ok, 1.0 / np.where(ok, rr, 1.0), 0.0)
            rho[sel] += (ir2 ** 6) @ a[sel]
            g = slope * ir2 ** 7  # [n, n]
            H[sel] += np.einsum("ij,ija,j->ia", g, d, a[sel])
            W[b] += 0.5 * np.einsum("i,ij,ija,ijb,j->ab", a[sel], g, d, d, a[sel], optimize=True)
        U[b] = 0.5 * (a[sel] * rho[sel]).sum()
    return rho, H, U, W


def exact_lj_step(q, c, a, s, A, batch, alpha_c, alpha_d, r_c, N, mutant=None):
    """(F [n, 3], U_coulomb [B], U_lj [B], W [B, 3, 3]) of the truncated algorithm in float64"""
    q, c, a = (np.asarray(v, dtype=np.float64) for v in (q, c, a))
    _, E = eb.exact_algorithm(q, s, A, batch, alpha_c, r_c, N, field=True)
    U_C, W_C = ev.exact_algorithm_virial(q, s, A, batch, alpha_c, r_c, N)
    _, G = dr.dispersion(c, s, A, batch, alpha_d, r_c, N)
    U_D, W_D = dv.exact_algorithm_virial(c, s, A, batch, alpha_d, r_c, N)
    _, H, U_R, W_R = repulsion(a, s, A, batch, r_c, slope=6.0 if mutant == "six" else 12.0)
    if mutant == "no_self":
        U_D = U_D - dv._self_energy(c, batch, alpha_d)[:, 0]
    sign = 1.0 if mutant == "dispersion_sign" else -1.0
    F = q[:, None] * E + sign * c[:, None] * G + a[:, None] * H
    return F, U_C, U_R + sign * U_D, W_C + sign * W_D + W_R


def converged_lj_step(q, c, a, s, A, r_c, batch=None, R=None):
    """the same four with the two lattice sums carried to convergence (the repulsion stays cut at r_c: that is its
    definition), and the three energies (U_C, U_D, U_R) apart.  With `R` the dispersion potential, field and energy are
    those of the brute-force sum over every image within R (dr.lattice_sum); otherwise the converged split's."""
    q, c, a = (np.asarray(v, dtype=np.float64) for v in (q, c, a))
    _, E = eb.converged(q, s, A, batch, field=True)
    U_C, W_C = ev.converged_virial(q, s, A, batch)
    if R is None:
        _, G = dr.dispersion(c, s, A, batch, 3.2, None, 30, nimg=2)
    else:
        _, G = dr.lattice_sum(c, s, A, R, batch)
    U_D, W_D = dv.converged_virial(c, s, A, batch, R=R)
    _, H, U_R, W_R = repulsion(a, s, A, batch, r_c, nimg=1)
    F = q[:, None] * E - c[:, None] * G + a[:, None] * H
    return F, U_C, U_R - U_D, W_C - W_D + W_R, (U_C, U_D, U_R)


def converged_energy(q, c, a, s, A, r_c):
    """U = U_C - U_D + U_R of one point set from the converged sums: a smooth function of s and A except where a pair
    crosses r_c"""
    q, c, a = (np.asarray(v, dtype=np.float64) for v in (q, c, a))
    phi = eb.converged(q, s, A)
    psi = dr.dispersion(c, s, A, None, 3.2, None, 30, nimg=2)[0]
    rho = repulsion(a, s, A, None, r_c, nimg=1)[0]
    return 0.5 * ((q * phi).sum() - (c * psi).sum() + (a * rho).sum())


def eight(U_C, U_LJ, W):
    """in the layout of the native reductions: [B, 8], U_C, U_LJ, xx, yy, zz, yz, xz, xy"""
    return np.stack([U_C, U_LJ, W[:, 0, 0], W[:, 1, 1], W[:, 2, 2], W[:, 1, 2], W[:, 0, 2], W[:, 0, 1]], 1)


# ---- pair sums alone, as the native pair walk forms them (tests/test_gpu_lj_step.py) ------------------------------------

def near_step(q, c, a, s, A, batch, alpha_c, alpha_d, r_c):
    """(f [n, 3], eight [B, 8]) of the pair walk: f_i = sum_j (q_i q_j mg_C - c_i c_j mg_D + 12 a_i a_j / r^14) d_ij and the
    halved pair sums of q_i q_j w_C, a_i a_j / r^12 - c_i c_j w_D and s_ij d_a d_b"""
    q, c, a = (np.asarray(v, dtype=np.float64) for v in (q, c, a))
    fC = eb.near_field(q, s, A, batch, alpha_c, r_c)
    fD = dr.near_field(c, s, A, batch, alpha_d, r_c)
    UC, WC = ev.near_virial(q, s, A, batch, alpha_c, r_c)
    UD, WD = dv.near_virial(c, s, A, batch, alpha_d, r_c)
    _, H, UR, WR = repulsion(a, s, A, batch, r_c)
    f = q[:, None] * fC - c[:, None] * fD + a[:, None] * H
    return f, eight(UC, UR - UD, WC - WD + WR)


# ---- points --------------------------------------------------------------------------------------------------------

D_MIN_FRACTIONAL = 0.064  # no two distinct points of lj_points are closer than this in fractional terms (wrapped)
LJ_SPACING = 0.1          # its lattice spacing


def _wrapped_distance(x, y):
    d = np.asarray(x, dtype=np.float64) - np.asarray(y, dtype=np.float64)
    return np.sqrt(((d - np.rint(d)) ** 2).sum(-1))


def lj_points(rng, n=700):
    """n float32 FRACTIONAL points for r^-12: a 10^3 jittered lattice (spacing 0.1, jitter 0.018: no two closer than 0.064)
    thinned to n, with the edge cases of the wrap placed first and every lattice point closer than 0.064 to one of them
    left out.  Uniform random points would not do: one near-coincident pair's r^-12 would be the whole norm.  The layout:
    0 .. 19 lattice points, 20 .. 39 their exact duplicates (r = 0, skipped), 40 .. 75 the edge cases, then lattice points.
    The edge cases sit at distinct nodes of a coarse grid (-0.3, -0.1, 0.1, 0.3)^3 and are: a point on each lower face
    (-1/2), one at the largest float32 below 1/2 on each axis and one in that corner, each of the seven with a neighbour
    0.078 away; a pair 0.0714 apart through each face; eight points given one box to the right and eight two boxes to the
    left of where they act."""
    lattice = rng.permutation(dr.jittered_lattice(rng, 10, LJ_SPACING, 0.018).reshape(-1, 3))
    g = np.array([-0.3, -0.1, 0.1, 0.3], dtype=np.float32)
    anchors = iter(rng.permutation(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)))
    below = np.nextafter(np.float32(0.5), np.float32(0))  # the largest float32 below 1/2
    special = []
    step = np.float32(0.045)

    def place(make):
        """the points that `make` builds on the next coarse node at which they stay 0.15 clear of those placed before"""
        while True:
            pts = make(next(anchors).copy())
            if all(_wrapped_distance(np.array(special), p).min() >= 0.15 for p in pts if special):
                special.extend(pts)
                return

    def on_face(a, value, sign):
        def make(p):
            p[a] = value
            return [p, p + sign * step]
        return make

    def through_face(a):
        def make(y):
            z = y + np.float32(0.01)
            y[a], z[a] = -0.465, 0.465
            return [y, z]
        return make

    corner = np.full(3, below, dtype=np.float32)
    special += [corner, corner - step]
    for a in range(3):
        place(on_face(a, np.float32(-0.5), 1))
        place(on_face(a, below, -1))
        place(through_face(a))
    for shift in (1.0, -2.0):
        for _ in range(8):
            place(lambda p: [p + np.float32(shift)])
    special = np.array(special, dtype=np.float32)
    assert special.shape == (36, 3)
    keep = [p for p in lattice if _wrapped_distance(special, p).min() >= D_MIN_FRACTIONAL]
    assert len(keep) >= n - 56
    keep = np.array(keep[:n - 56], dtype=np.float32)
    return np.concatenate([keep[:20], keep[:20], special, keep[20:]]).astype(np.float32)


def separated_points(rng, n, A, d_min):
    """n float64 fractional points in [-1/2, 1/2)^3, no two closer than d_min in the box A (rejection sampling)"""
    A = np.asarray(A, dtype=np.float64)
    pts = []
    while len(pts) < n:
        x = rng.random(3) - 0.5
        if pts:
            ds = np.array(pts) - x
            d = (ds - np.rint(ds)) @ A
            if (d * d).sum(-1).min() < d_min * d_min:
                continue
        pts.append(x)
    return np.array(pts)
