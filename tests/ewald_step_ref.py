"""Float64 restatement of the fused Ewald step -- TEST INFRASTRUCTURE ONLY.

``nfft_ewald_step`` returns ``(phi, E, U, W)``; nothing about them is new, so the restatement is a composition of the
committed ones and adds no formula of its own: ``(phi, E)`` is ``ewald_box_ref.exact_algorithm(..., field=True)``, ``(U, W)``
is ``ewald_virial_ref.exact_algorithm_virial``, and a list of excluded pairs takes ``exclusions_ref.listed_terms`` and
``listed_virial`` out of them.  tests/test_ewald_step_ref.py checks the composition against the converged sums and against
itself (``U = 1/2 sum q phi``).  A plain module like ewald_ref.py; positions are FRACTIONAL, ``A`` holds the lattice vectors
as rows."""
import numpy as np

import ewald_box_ref as eb
import ewald_virial_ref as ev
import exclusions_ref as xr


def exact_step(q, s, A, batch, alpha, r_c, N, pairs=None, weights=None, mutant=None):
    """(phi [n, *cols], E [n, 3, *cols], U [B, *cols], W [B, 3, 3, *cols]) of the truncated algorithm in float64; `pairs`
    [m, 2] with `weights` 1 - scale: without those pairs; `mutant`: as ewald_virial_ref takes it (U and W only)"""
    phi, E = eb.exact_algorithm(q, s, A, batch, alpha, r_c, N, field=True)
    U, W = ev.exact_algorithm_virial(q, s, A, batch, alpha, r_c, N, mutant=mutant)
    if pairs is not None:
        zx, fx = xr.listed_terms(xr.COULOMB, q, s, A, pairs, weights, alpha)
        Ux, Wx = xr.listed_virial(xr.COULOMB, q, s, A, batch, pairs, weights, alpha)
        phi, E, U, W = phi - zx, E - fx, U - Ux, W - Wx
    return phi, E, U, W


def converged_step(q, s, A, batch=None, **kw):
    """the same four from the sums carried to convergence"""
    phi, E = eb.converged(q, s, A, batch, field=True, **kw)
    U, W = ev.converged_virial(q, s, A, batch, **kw)
    return phi, E, U, W


def energy_of(q, phi, batch=None):
    """U_b = 1/2 sum_{i in set b} q_i phi_i [B, *cols]"""
    return xr.energy(q, phi, batch)


def seven(U, W):
    """(U, W) in the layout of the native reductions: [B, 7, *cols], energy, xx, yy, zz, yz, xz, xy"""
    return np.stack([U, W[:, 0, 0], W[:, 1, 1], W[:, 2, 2], W[:, 1, 2], W[:, 0, 2], W[:, 0, 1]], 1)
