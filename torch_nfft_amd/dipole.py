"""Ewald summation for point charges and point dipoles: potential, field and field gradient of a periodic box, NFFT far
field + wrapped pair sum (no reference counterpart; Smith, CCP5 Newsletter 46, 18 (1998); Aguado and
Madden, J. Chem. Phys. 119, 7471 (2003)).

Notation as in ``ewald.py``: integer frequency ``k``, ``kappa = A^-1 k``, ``V = det A``, ``x = s A`` with fractional ``s`` in
``[-1/2, 1/2)^3``; the unit cube is ``A = I``.  Source ``j`` carries a charge ``q_j`` and a Cartesian dipole ``mu_j``.  With
``d = d_ij`` the minimum image of ``x_i - x_j``, ``r = |d|``, ``m = mu_j . d`` and the Smith functions ``B_0 = erfc(alpha r) / r``,
``B_l = ((2l - 1) B_(l-1) + (2 alpha^2)^l / (alpha sqrt(pi)) e^(-alpha^2 r^2)) / r^2``::

    phi_i  =   sum_{j: 0 < r < r_c} q_j B_0 + m B_1                                                       near
             + sum_{k != 0} b_k rho_k e^{2 pi i k.s_i},   rho_k = sum_j (q_j - 2 pi i kappa . mu_j) e^{-2 pi i k.s_j}   far
             - (2 alpha / sqrt(pi)) q_i - pi Q / (alpha^2 V)                                              self and background
    E_i,a  =   sum_j (q_j B_1 + m B_2) d_a - mu_j,a B_1   + far with the factor (-2 pi i kappa_a)   + (4 alpha^3 / (3 sqrt(pi))) mu_i,a
    T_i,ab =   sum_j q_j (delta_ab B_1 - d_a d_b B_2) + (mu_j,a d_b + mu_j,b d_a + m delta_ab) B_2 - m d_a d_b B_3
             + far with the factor 4 pi^2 kappa_a kappa_b   - (4 alpha^3 / (3 sqrt(pi))) q_i delta_ab

``E = -grad_x phi``, ``T_ab = d E_a / d x_b``, ``b_k`` are the coefficients of ``EwaldSplitting`` (written with the sign
convention of the formulas above; the transforms sum ``e^{+2 pi i k.s}`` in the adjoint and the signs in the code follow
them, as in ``EwaldSplitting.field_coeffs``).  The energy is ``U = 1/2 sum_i (q_i phi_i - mu_i . E_i)`` and the force on
source ``i`` is ``q_i E_i + T_i mu_i``.  The far part is one adjoint transform of the packed sources ``(q, mu)``, one native
spectral pass (``ops.nfft_ewald_dipole_spectral``) and one forward transform that carries the 4 or 10 spectra as further
columns; the near part is one native pair sweep (``ops.nfft_ewald_dipole_near``).
"""
import math

import torch
from torch.autograd.function import once_differentiable

from . import ops
from .ewald import EwaldSplitting, _fractional, _set_sums, _voigt_to_matrix
from .nfft import nfft_adjoint, nfft_forward


def _dipole(xs, pos, batch, splitting, cutoff, order):
    """``[n, 4 or 10, *cols]``: (phi, E) and at ``order = 2`` the six entries of T in the order of ``ewald._VOIGT``, of the
    packed sources ``xs`` ``[n, 4, *cols]``, without autograd: far field, pair sweep, self and background terms (with a box:
    ``pos`` fractional; ``mu``, ``E`` and ``T`` Cartesian)"""
    N, alpha = splitting.bandwidth, splitting.alpha
    box = () if splitting.box is None else splitting.box6
    band = nfft_adjoint(xs, pos, batch, bandwidth=N, cutoff=cutoff)  # [B, N, N, N, 4, *cols]
    spectra = ops.nfft_ewald_dipole_spectral(band, splitting.coeffs, box, order)  # [B, N, N, N, 4 or 10, *cols]
    out = nfft_forward(spectra, pos, batch, cutoff=cutoff, real_output=True)
    out = out + ops.nfft_ewald_dipole_near(pos, xs, batch, box, alpha, splitting.r_cut, order)
    q, mu = xs[:, 0], xs[:, 1:]
    self3 = 4.0 * alpha ** 3 / (3.0 * math.sqrt(math.pi))
    out[:, 0] -= (2.0 * alpha / math.sqrt(math.pi)) * q + (math.pi / (alpha * alpha * splitting.volume)) * _set_sums(q, batch)[1]
    out[:, 1:4] += self3 * mu
    if order == 2:
        out[:, 4:7] -= self3 * q.unsqueeze(1)
    return out


class NfftEwaldDipoleFunction(torch.autograd.Function):
    """``(phi, E, T)`` of ``nfft_ewald_dipole`` (``T`` empty without ``gradient``).  The operator ``(q, mu) -> (phi, -E)`` is
    real symmetric, so for ``g_phi = dL/dphi`` and ``g_E = dL/dE`` the gradients in the sources are that operator applied to
    the weights ``(q~, mu~) = (g_phi, -g_E)``: ``dq = phi[q~, mu~]``, ``dmu = -E[q~, mu~]``, and the gradient in the positions is
    ``dL/dpos_i = -sum_c (q~_i E[s]_i + T[s]_i mu~_i + q_i E[s~]_i + T[s~]_i mu_i)``: one evaluation of order 2 with the sources
    ``s`` and the weights ``s~`` side by side as columns.  First order only (``once_differentiable``); ``T`` is not
    differentiable.  With a box ``pos`` holds the fractional coordinates, the formula gives ``dL/dx`` and the backward
    returns ``dL/ds = (dL/dx) A^T``."""

    @staticmethod
    def forward(ctx, q, mu, pos, batch, splitting, cutoff, gradient):
        if batch is not None and batch.requires_grad:
            raise AssertionError("nfft_ewald_dipole is differentiable w.r.t. q, mu and pos only, but batch requires grad")
        ctx.splitting, ctx.cutoff = splitting, cutoff
        ctx.save_for_backward(q, mu, pos, batch)
        out = _dipole(torch.cat([q.unsqueeze(1), mu], 1), pos, batch, splitting, cutoff, 2 if gradient else 1)
        T = _voigt_to_matrix(out[:, 4:]) if gradient else q.new_empty(0)
        ctx.mark_non_differentiable(T)
        return out[:, 0].clone(), out[:, 1:4].clone(), T

    @staticmethod
    @once_differentiable
    def backward(ctx, g_phi, g_E, _):
        q, mu, pos, batch = ctx.saved_tensors
        need_q, need_mu, need_pos = ctx.needs_input_grad[:3]
        xt = torch.cat([g_phi.unsqueeze(1), -g_E], 1)  # the weights (q~, mu~)
        dq = dmu = dpos = None
        if need_pos:
            xs = torch.cat([q.unsqueeze(1), mu], 1)
            out = _dipole(torch.stack([xs, xt], 2), pos, batch, ctx.splitting, ctx.cutoff, 2)  # [n, 10, 2, *cols]
            own, adj = out[:, :, 0], out[:, :, 1]
            dq, dmu = adj[:, 0], -adj[:, 1:4]
            w = xt[:, :1] * own[:, 1:4] + (_voigt_to_matrix(own[:, 4:]) * xt[:, 1:].unsqueeze(1)).sum(2)
            w = w + xs[:, :1] * adj[:, 1:4] + (_voigt_to_matrix(adj[:, 4:]) * xs[:, 1:].unsqueeze(1)).sum(2)
            dpos = -w.reshape(w.size(0), 3, math.prod(w.shape[2:])).sum(2)
            if ctx.splitting.box is not None:
                dpos = dpos @ ctx.splitting._matrices(dpos.device)[0].t()
        elif need_q or need_mu:
            adj = _dipole(xt, pos, batch, ctx.splitting, ctx.cutoff, 1)
            dq, dmu = adj[:, 0], -adj[:, 1:4]
        return dq if need_q else None, dmu if need_mu else None, dpos, None, None, None, None


def _sources(what, q, mu, pos, batch, splitting):
    """the checks; ``(q, mu)`` with a missing one as zeros"""
    if not isinstance(splitting, EwaldSplitting):
        raise TypeError("%s: splitting must be an EwaldSplitting" % what)
    if pos.dim() != 2 or pos.size(1) != 3:
        raise ValueError("%s: the periodic dipole sum is three-dimensional, pos must be [n, 3]" % what)
    if q is None and mu is None:
        raise ValueError("%s: q and mu must not both be None" % what)
    for name, v in (("q", q), ("mu", mu)):
        if v is None:
            continue
        if v.is_complex():
            raise ValueError("%s: %s must be real (float32), not complex" % (what, name))
        if v.dtype != torch.float32:
            raise ValueError("%s: %s must be float32" % (what, name))
    n = pos.size(0)
    if mu is not None and (mu.dim() < 2 or mu.size(0) != n or mu.size(1) != 3):
        raise ValueError("%s: mu must be [n, 3, *cols]" % what)
    if q is not None and (q.dim() < 1 or q.size(0) != n):
        raise ValueError("%s: q must be [n, *cols]" % what)
    if q is not None and mu is not None and tuple(q.shape[1:]) != tuple(mu.shape[2:]):
        raise ValueError("%s: q [n, *cols] and mu [n, 3, *cols] must have the same columns" % what)
    if batch is not None and batch.requires_grad:
        raise AssertionError("%s is differentiable w.r.t. q, mu and pos only, but batch requires grad" % what)
    if q is None:
        q = mu.new_zeros((n,) + tuple(mu.shape[2:]))
    if mu is None:
        mu = q.new_zeros((n, 3) + tuple(q.shape[1:]))
    return q, mu


def nfft_ewald_dipole(q, mu, pos, batch=None, /, splitting=None, cutoff=4, gradient=False, fractional=False):
    """Potential, field and field gradient of periodic point charges ``q`` ``[n, *cols]`` and point dipoles ``mu``
    ``[n, 3, *cols]`` (float32, Cartesian) at ``pos`` ``[n, 3]``, over the sources of i's point set (``batch``: sorted point-set
    indices) and all their periodic images, in the Ewald sense: the self pair is left out, and a point set that is not
    neutral gets a uniform neutralising background.  ``q=None`` is a set of pure dipoles, ``mu=None`` one of pure charges
    (``phi`` and ``E`` are then those of ``nfft_ewald``).  Coincident sources do not see each other in the pair sum.

    Returns ``(phi, E)``, ``phi`` ``[n, *cols]`` and ``E = -grad_x phi`` ``[n, 3, *cols]``; with ``gradient=True``
    ``(phi, E, T)``, ``T_ab = d E_a / d x_b`` ``[n, 3, 3, *cols]``, symmetric, ``tr T_i = -4 pi Q / V`` (the background).
    ``splitting`` is an ``EwaldSplitting`` (TypeError otherwise); complex input is refused (ValueError).  Positions, boxes,
    ``fractional`` and ``cutoff`` are those of ``nfft_ewald``: Cartesian positions are taken modulo the lattice, with
    ``fractional=True`` (which needs a box: ValueError) they are the fractional coordinates; ``mu``, ``E`` and ``T`` are
    always Cartesian.

    Differentiable once in ``q``, ``mu`` and ``pos`` through ``phi`` and ``E``; ``T`` is not differentiable, a second
    derivative raises a RuntimeError, and ``batch`` must not require grad (AssertionError).  The gradient comes back in the
    coordinates that were passed."""
    q, mu = _sources("nfft_ewald_dipole", q, mu, pos, batch, splitting)
    pos = _fractional("nfft_ewald_dipole", pos, splitting, fractional)
    phi, E, T = NfftEwaldDipoleFunction.apply(q, mu, pos, batch, splitting, int(cutoff), bool(gradient))
    return (phi, E, T) if gradient else (phi, E)


def nfft_ewald_dipole_energy(q, mu, pos, batch=None, /, splitting=None, cutoff=4, fractional=False):
    """``U_b = 1/2 sum_{i in point set b} (q_i phi_i - mu_i . E_i)`` with ``(phi, E) = nfft_ewald_dipole(q, mu, pos, batch,
    ...)``: ``[B, *cols]``, one energy per point set and column.  Its gradient in ``pos`` is minus the force,
    ``dU/dpos_i = -(q_i E_i + T_i mu_i)`` summed over the columns (Cartesian ``pos`` in a box; ``fractional`` as for
    ``nfft_ewald_dipole``)."""
    q, mu = _sources("nfft_ewald_dipole_energy", q, mu, pos, batch, splitting)
    phi, E = nfft_ewald_dipole(q, mu, pos, batch, splitting=splitting, cutoff=cutoff, fractional=fractional)
    return 0.5 * _set_sums(q * phi - (mu * E).sum(1), batch)[0]
