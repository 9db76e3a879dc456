"""Periodic Stokeslet sum (Hasimoto's Ewald sum): the velocity of a periodic array of point forces in Stokes flow and its
gradient, NFFT far field + wrapped pair sum (no reference counterpart; Hasimoto, J. Fluid Mech. 5,
317 (1959); Lindbo and Tornberg, J. Comput. Phys. 229, 8994 (2010)).

Notation as in ``ewald.py`` and ``dipole.py``: integer frequency ``k``, ``kappa = A^-1 k``, ``V = det A``, ``x = s A`` with
fractional ``s`` in ``[-1/2, 1/2)^3``; the unit cube is ``A = I``.  Source ``j`` carries a Cartesian force ``f_j``.  The sum is
``u_i = sum'_{j, p} S(x_i - x_j + p) f_j`` with the Stokeslet ``S(r) = I / r + r r^T / r^3`` over the sources of i's point set
and all lattice vectors ``p``, the self pair left out; the physical velocity is ``u / (8 pi eta)``.  The ``k = 0`` mode is
dropped: zero mean flow, the net force balanced by a pressure gradient (Hasimoto's convention).  With ``d = d_ij`` the
minimum image of ``x_i - x_j``, ``r = |d|``, ``m = d . f_j``, ``B_0 = erfc(alpha r) / r``, ``g = (2 alpha / sqrt(pi)) e^(-alpha^2 r^2)``,
``B_1 = (B_0 + g) / r^2`` and ``B_2 = (3 B_1 + 2 alpha^2 g) / r^2``::

    u_i,a  =   sum_{j: 0 < r < r_c} (B_0 - g) f_j,a + B_1 m d_a                                                     near
             + sum_{k != 0} c_k ((I - kappa kappa^T / |kappa|^2) rho_k)_a e^{2 pi i k.s_i},   rho_k = sum_j f_j e^{-2 pi i k.s_j}   far
             - (4 alpha / sqrt(pi)) f_i,a                                                                           self
    G_i,ab =   sum_j (2 alpha^2 g - B_1) f_j,a d_b + B_1 (d_a f_j,b + m delta_ab) - B_2 m d_a d_b
             + far with the further factor 2 pi i kappa_b

``c_k = 2 b_k (1 + pi^2 |kappa|^2 / alpha^2)`` with the ``b_k`` of ``EwaldSplitting`` (``EwaldSplitting.stokeslet_coeffs``),
``G_ab = d u_a / d x_b`` is not symmetric and ``tr G = 0`` (incompressibility); the operator ``f -> u`` is real symmetric.  The
formulas are written with ``e^{-2 pi i k.s_j}`` in ``rho``; the transforms sum ``e^{+2 pi i k.s}`` in the adjoint and the signs
in the code follow them, as in ``EwaldSplitting.field_coeffs``.  The far part is one adjoint transform of the forces, one
native spectral pass (``ops.nfft_ewald_stokeslet_spectral``) and one forward transform that carries the 3 or 12 spectra as
further columns; the near part is one native pair sweep (``ops.nfft_ewald_stokeslet_near``).
"""
import math

import torch
from torch.autograd.function import once_differentiable

from . import ops
from .ewald import EwaldSplitting, _fractional, _set_sums
from .nfft import nfft_adjoint, nfft_forward


def _stokeslet(f, pos, batch, splitting, cutoff, order):
    """``[n, 3 or 12, *cols]``: u and at ``order = 2`` the nine entries of G, row-major, of the forces ``f`` ``[n, 3, *cols]``,
    without autograd: far field, pair sweep, self term (with a box: ``pos`` fractional; ``f``, ``u`` and ``G`` Cartesian)"""
    N, alpha = splitting.bandwidth, splitting.alpha
    box = () if splitting.box is None else splitting.box6
    band = nfft_adjoint(f, pos, batch, bandwidth=N, cutoff=cutoff)  # [B, N, N, N, 3, *cols]
    spectra = ops.nfft_ewald_stokeslet_spectral(band, splitting.stokeslet_coeffs, box, order)  # [B, N, N, N, 3 or 12, *cols]
    out = nfft_forward(spectra, pos, batch, cutoff=cutoff, real_output=True)
    out = out + ops.nfft_ewald_stokeslet_near(pos, f, batch, box, alpha, splitting.r_cut, order)
    out[:, :3] -= (4.0 * alpha / math.sqrt(math.pi)) * f
    return out


def _matrix(nine):
    """``[n, 9, *cols]`` row-major as ``[n, 3, 3, *cols]``"""
    return nine.reshape((nine.size(0), 3, 3) + tuple(nine.shape[2:]))


def _symmetric_backward(evaluate, f, g, splitting, need_f, need_pos):
    """``(df, dpos)`` of ``sum g . u[f]`` for a real symmetric operator ``evaluate(forces, order) -> [n, 3 or 12, *cols]``: see
    ``NfftEwaldStokesletFunction``"""
    g = g.contiguous()
    df = dpos = None
    if need_pos:
        out = evaluate(torch.stack([f, g], 2), 2)  # [n, 12, 2, *cols]
        df = out[:, :3, 1]
        Gf, Gg = _matrix(out[:, 3:, 0]), _matrix(out[:, 3:, 1])  # [n, 3 (a), 3 (b), *cols]
        w = (g.unsqueeze(2) * Gf + f.unsqueeze(2) * Gg).sum(1)  # [n, 3 (b), *cols]
        dpos = w.reshape(w.size(0), 3, math.prod(w.shape[2:])).sum(2)
        if splitting.box is not None:
            dpos = dpos @ splitting._matrices(dpos.device)[0].t()
    elif need_f:
        df = evaluate(g, 1)
    return df if need_f else None, dpos


class NfftEwaldStokesletFunction(torch.autograd.Function):
    """``(u, G)`` of ``nfft_ewald_stokeslet`` (``G`` empty without ``gradient``).  The operator ``f -> u`` is real symmetric, so
    for ``g = dL/du`` the gradient in the forces is that operator applied to ``g``, ``df = u[g]``, and the gradient in the
    positions is ``dL/dpos_i,b = sum_c sum_a (g_i,a G[f]_i,ab + f_i,a G[g]_i,ab)``: one evaluation of order 2 with ``f`` and
    ``g`` side by side as columns (order 1 of ``g`` alone when ``pos`` needs no gradient).  First order only
    (``once_differentiable``); ``G`` is not differentiable.  With a box ``pos`` holds the fractional coordinates, the formula
    gives ``dL/dx`` and the backward returns ``dL/ds = (dL/dx) A^T``."""

    @staticmethod
    def forward(ctx, f, pos, batch, splitting, cutoff, gradient):
        if batch is not None and batch.requires_grad:
            raise AssertionError("nfft_ewald_stokeslet is differentiable w.r.t. f and pos only, but batch requires grad")
        ctx.splitting, ctx.cutoff = splitting, cutoff
        ctx.save_for_backward(f, pos, batch)
        out = _stokeslet(f, pos, batch, splitting, cutoff, 2 if gradient else 1)
        G = _matrix(out[:, 3:]).clone() if gradient else f.new_empty(0)
        ctx.mark_non_differentiable(G)
        return out[:, :3].clone(), G

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _):
        f, pos, batch = ctx.saved_tensors
        df, dpos = _symmetric_backward(lambda x, order: _stokeslet(x, pos, batch, ctx.splitting, ctx.cutoff, order), f, g,
                                       ctx.splitting, *ctx.needs_input_grad[:2])
        return df, dpos, None, None, None, None


def _check(what, f, pos, batch, splitting, name="Stokeslet"):
    if not isinstance(splitting, EwaldSplitting):
        raise TypeError("%s: splitting must be an EwaldSplitting" % what)
    if pos.dim() != 2 or pos.size(1) != 3:
        raise ValueError("%s: the periodic %s sum is three-dimensional, pos must be [n, 3]" % (what, name))
    if f.is_complex():
        raise ValueError("%s: f must be real (float32), not complex" % what)
    if f.dtype != torch.float32:
        raise ValueError("%s: f must be float32" % what)
    if f.dim() < 2 or f.size(0) != pos.size(0) or f.size(1) != 3:
        raise ValueError("%s: f must be [n, 3, *cols]" % what)
    if batch is not None and batch.requires_grad:
        raise AssertionError("%s is differentiable w.r.t. f and pos only, but batch requires grad" % what)


def nfft_ewald_stokeslet(f, pos, batch=None, /, splitting=None, cutoff=4, gradient=False, fractional=False):
    """The periodic Stokeslet sum ``u_i = sum'_{j, p} S(x_i - x_j + p) f_j``, ``S(r) = I / r + r r^T / r^3``, of the point forces
    ``f`` ``[n, 3, *cols]`` (float32, Cartesian) at ``pos`` ``[n, 3]``, over the sources of i's point set (``batch``: sorted
    point-set indices) and all their periodic images: the self pair is left out and the mean flow is zero (the ``k = 0`` mode is
    dropped; a net force is balanced by a pressure gradient).  The velocity of Stokes flow is ``u / (8 pi eta)``.  Coincident
    sources do not see each other in the pair sum.

    Returns ``u`` ``[n, 3, *cols]``; with ``gradient=True`` ``(u, G)``, ``G_ab = d u_a / d x_b`` ``[n, 3, 3, *cols]``, not symmetric,
    ``tr G_i = 0``.  ``splitting`` is an ``EwaldSplitting`` (TypeError otherwise; ``stokeslet_splitting`` chooses one for a
    tolerance); complex input is refused (ValueError).  Positions, boxes, ``fractional`` and ``cutoff`` are those of
    ``nfft_ewald``: Cartesian positions are taken modulo the lattice, with ``fractional=True`` (which needs a box: ValueError)
    they are the fractional coordinates; ``f``, ``u`` and ``G`` are always Cartesian.

    Differentiable once in ``f`` and ``pos`` through ``u``; ``G`` is not differentiable, a second derivative raises a
    RuntimeError, and ``batch`` must not require grad (AssertionError).  The gradient comes back in the coordinates that were
    passed."""
    _check("nfft_ewald_stokeslet", f, pos, batch, splitting)
    pos = _fractional("nfft_ewald_stokeslet", pos, splitting, fractional)
    u, G = NfftEwaldStokesletFunction.apply(f, pos, batch, splitting, int(cutoff), bool(gradient))
    return (u, G) if gradient else u


def nfft_ewald_stokeslet_power(f, pos, batch=None, /, splitting=None, cutoff=4, fractional=False):
    """``P_b = 1/2 sum_{i in point set b} f_i . u_i`` with ``u = nfft_ewald_stokeslet(f, pos, batch, ...)``: ``[B, *cols]``, one
    value per point set and column (``P / (4 pi eta)`` is the rate at which the forces work on the fluid).  Its gradient in ``pos``
    is ``dP/dpos_i,b = sum_a f_i,a G_i,ab`` summed over the columns (Cartesian ``pos`` in a box; ``fractional`` as for
    ``nfft_ewald_stokeslet``)."""
    _check("nfft_ewald_stokeslet_power", f, pos, batch, splitting)
    u = nfft_ewald_stokeslet(f, pos, batch, splitting=splitting, cutoff=cutoff, fractional=fractional)
    return 0.5 * _set_sums((f * u).sum(1), batch)[0]


# ---- a splitting for a tolerance ---------------------------------------------------------------------------------------
SAFETY = 10.0  # see stokeslet_splitting


def near_tail(a):
    """An upper bound of what one pair at the distance ``r >= r_c`` still contributes to u and to G, relative to the
    unscreened Stokeslet and its gradient at that distance, ``a = alpha r_c``.  The screened tensor ``(B_0 - g) I + B_1 d d^T``
    has the eigenvalues ``B_0 - g`` (twice) and ``2 B_0``, the Stokeslet ``1 / r`` (twice) and ``2 / r``: the largest ratio is
    ``max(erfc a, |erfc a - (2 a / sqrt(pi)) e^(-a^2)|)``.  For G the four terms are bounded one by one, ``r^3 |2 alpha^2 g - B_1|
    + (1 + sqrt 3) r^3 B_1 + r^5 B_2``, against the same expression at ``alpha = 0``, ``5 + sqrt 3``.  Both fall monotonically for
    ``a >= 1.5``."""
    e = 2.0 * a / math.sqrt(math.pi) * math.exp(-a * a)  # r g
    b0 = math.erfc(a)  # r B_0
    b1 = b0 + e  # r^3 B_1
    g2 = 2.0 * a * a * e  # r^3 2 alpha^2 g
    b2 = 3.0 * b1 + g2  # r^5 B_2
    u = max(b0, abs(b0 - e))
    G = (abs(g2 - b1) + (1.0 + math.sqrt(3.0)) * b1 + b2) / (5.0 + math.sqrt(3.0))
    return max(u, G)


def far_tail(y):
    """An upper bound of the far sum beyond the sphere ``|kappa| >= kappa_c``, ``y = pi kappa_c / alpha``, with every phase taken
    as 1 and the projector as the identity, the lattice sum as its integral: ``int 4 pi kappa^2 V c_k d kappa = (8 alpha / pi)
    int_y^inf (1 + t^2) e^(-t^2) dt``, relative to the self term ``4 alpha / sqrt(pi)`` (the size of the far part at a source):
    ``(3/2) erfc y + (y / sqrt(pi)) e^(-y^2)``.  For G the integrand carries ``2 pi kappa = 2 alpha t``, relative to
    ``alpha`` times the self term: ``(2 / sqrt(pi)) (2 + y^2) e^(-y^2)``."""
    e = math.exp(-y * y)
    return max(1.5 * math.erfc(y) + y / math.sqrt(math.pi) * e, 2.0 / math.sqrt(math.pi) * (2.0 + y * y) * e)


def _smallest(tail, tol):
    """the smallest argument >= 1.5 (to 1e-6) at which the falling ``tail`` is <= tol"""
    lo, hi = 1.5, 1.5
    while tail(hi) > tol:
        lo, hi = hi, hi + 0.5
    if hi == lo:
        return hi
    while hi - lo > 1e-6:
        mid = 0.5 * (lo + hi)
        lo, hi = (lo, mid) if tail(mid) <= tol else (mid, hi)
    return hi


def stokeslet_splitting(tol, r_cut, box=None, device="cuda"):
    """An ``EwaldSplitting`` for ``nfft_ewald_stokeslet`` whose two truncation tails, of u and of G, are at most ``tol``:
    ``alpha = a / r_cut`` with the smallest ``a`` such that ``SAFETY near_tail(a) <= tol``, and ``bandwidth`` the next even integer
    ``>= 2 alpha y max_a |a_a| / pi`` with the smallest ``y`` such that ``SAFETY far_tail(y) <= tol`` (the first plane that the grid
    leaves out, ``k_a = N/2``, lies at ``kappa >= (N/2) / |a_a|``; the longest lattice vector sets ``N`` for all three axes).

    ``near_tail`` and ``far_tail`` are upper bounds, not rms estimates, of this sum's own kernels -- the far one carries the
    factor ``1 + pi^2 kappa^2 / alpha^2`` that the Coulomb sum's does not -- for one pair at the cut and for the continuous
    spectrum of one source.  ``SAFETY = 10`` stands for what they leave out: the number of pairs in the shell just beyond the
    cut against the neighbours inside it, and the lattice sum against its integral.  Both tails fall like ``e^(-a^2)``, so
    the factor moves ``a`` and ``y`` by ``ln 10 / (2 a)``, about 8 % at ``tol = 1e-5``.  ValueError as for
    ``EwaldSplitting.from_tolerance``."""
    tol, r_cut, A, longest = EwaldSplitting._tolerance_box(tol, r_cut, box)
    alpha = _smallest(near_tail, tol / SAFETY) / r_cut
    y = _smallest(far_tail, tol / SAFETY)
    N = max(2, 2 * math.ceil(alpha * y * longest / math.pi))
    return EwaldSplitting(alpha, r_cut, N, box=A, device=device)
