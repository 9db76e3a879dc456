"""Ewald summation for the periodic 1/r: the Coulomb sum of charges in a periodic unit box, NFFT far field + wrapped pair
sum (no reference counterpart; P2NFFT in the NFFT3 family).

For charges ``q_j`` at ``x_j`` on the torus ``[-1/2, 1/2)^3`` (Gaussian units, box length 1), ``Q = sum_j q_j``::

    phi_i = sum'_{j, n} q_j / |x_i - x_j + n|      (Ewald / tin-foil sense; a uniform neutralising background if Q != 0)
          =   sum_{j != i, 0 < r_ij < r_c} q_j erfc(alpha r_ij) / r_ij          near: r_ij = |minimum image of x_i - x_j|
            + sum_{k != 0} b_k e^{2 pi i k.x_i} sum_j q_j e^{-2 pi i k.x_j}      far:  b_k = exp(-pi^2 |k|^2 / alpha^2) / (pi |k|^2)
            - (2 alpha / sqrt(pi)) q_i - pi Q / alpha^2                         self and background
    E_i   = -grad phi_i

The far part is ``nfft_fastsum`` on the whole torus with the coefficients ``b`` (cut to ``k in [-N/2, N/2)^3``, the
unpaired planes ``k_a = -N/2`` zeroed so that a real ``q`` gives a real ``phi`` and the operator stays symmetric); the near
part is one native pair sweep that wraps around the box (``ops.nfft_ewald_near``).  A box of length ``L`` is a rescaling
that the caller does: ``phi_L(x) = phi_1(x / L) / L`` and ``E_L(x) = E_1(x / L) / L^2``.
"""
import math

import torch
from torch.autograd.function import once_differentiable

from . import ops
from .nfft import nfft_adjoint, nfft_forward, nfft_fastsum

MAX_R_CUT = 1.0 / 3.0  # the pair sweep needs 3 cells of edge >= r_cut per axis


class EwaldSplitting:
    """The three parameters of the split and the far field's coefficients.

    ``alpha > 0`` is the splitting parameter, ``r_cut`` in ``(0, 1/3]`` the radius of the pair sum, ``bandwidth`` (even)
    the number ``N`` of frequencies per axis.  ``coeffs`` is ``[N, N, N]`` float32 on ``device``: ``b_k`` at index
    ``k + N/2``, evaluated in float64 on the host, ``b_0 = 0`` and the unpaired planes ``k_a = -N/2`` zeroed.
    ValueError for an odd or too small ``bandwidth``, ``alpha <= 0`` or ``r_cut`` outside ``(0, 1/3]``."""

    def __init__(self, alpha, r_cut, bandwidth, device="cuda"):
        alpha, r_cut, N = float(alpha), float(r_cut), int(bandwidth)
        if N != bandwidth or N < 2 or N % 2:
            raise ValueError("EwaldSplitting: bandwidth must be even and >= 2")
        if not (alpha > 0.0 and math.isfinite(alpha)):
            raise ValueError("EwaldSplitting: alpha must be positive")
        if not 0.0 < r_cut <= MAX_R_CUT:
            raise ValueError("EwaldSplitting: r_cut must lie in (0, 1/3]")
        self.alpha, self.r_cut, self.bandwidth = alpha, r_cut, N
        k = torch.arange(-(N // 2), N // 2, dtype=torch.float64)
        k2 = (k * k).reshape(N, 1, 1) + (k * k).reshape(1, N, 1) + (k * k).reshape(1, 1, N)
        b = torch.exp(-(math.pi / alpha) ** 2 * k2) / (math.pi * k2.clamp(min=1.0))
        b[N // 2, N // 2, N // 2] = 0.0
        b[0, :, :] = 0.0
        b[:, 0, :] = 0.0
        b[:, :, 0] = 0.0
        self.coeffs = b.to(torch.float32).to(torch.device(device)).contiguous()
        self._field_coeffs = None

    @classmethod
    def from_tolerance(cls, tol, r_cut, device="cuda"):
        """``alpha = sqrt(-ln tol) / r_cut`` and ``bandwidth`` the next even integer ``>= 2 alpha sqrt(-ln tol) / pi``:
        the two truncation factors -- ``erfc(alpha r_c) ~ e^(-alpha^2 r_c^2)`` of the pair sum at ``r_cut`` and
        ``e^(-pi^2 k^2 / alpha^2)`` of the far sum at ``k = N/2`` -- both set to ``tol``.  A rule of thumb, not a bound:
        the errors of the two sums also carry the number of charges and the prefactors ``1/r`` and ``1/(pi k^2)``."""
        tol = float(tol)
        if not 0.0 < tol < 1.0:
            raise ValueError("EwaldSplitting.from_tolerance: tol must lie in (0, 1)")
        if not 0.0 < float(r_cut) <= MAX_R_CUT:
            raise ValueError("EwaldSplitting: r_cut must lie in (0, 1/3]")
        s = math.sqrt(-math.log(tol))
        alpha = s / float(r_cut)
        N = max(2, 2 * math.ceil(alpha * s / math.pi))
        return cls(alpha, r_cut, N, device=device)

    def field_coeffs(self):
        """``[N, N, N, 4]`` complex64: ``b_k`` and, for the three axes, ``(+2 pi i k_a) b_k`` -- the coefficients of
        ``phi`` and of ``E = -grad phi`` as four columns of one forward transform (built on first use)."""
        if self._field_coeffs is None:
            N, b = self.bandwidth, self.coeffs
            freq = 2.0 * math.pi * torch.arange(-(N // 2), N // 2, dtype=torch.float32, device=b.device)
            cols = [torch.complex(b, torch.zeros_like(b))]
            for a in range(3):
                shape = [1, 1, 1]
                shape[a] = N
                cols.append(torch.complex(torch.zeros_like(b), b * freq.reshape(shape)))
            self._field_coeffs = torch.stack(cols, 3).contiguous()
        return self._field_coeffs


def _set_sums(q, batch):
    """(``[B, *cols]`` sums of ``q`` over every point set, the same gathered back to ``[n, *cols]``)"""
    if batch is None:
        total = q.sum(0, keepdim=True)
        return total, total.expand_as(q)
    B = int(batch[-1]) + 1 if batch.numel() else 0
    total = torch.zeros((B,) + tuple(q.shape[1:]), dtype=q.dtype, device=q.device).index_add_(0, batch, q)
    return total, total.index_select(0, batch)


def _ewald(q, pos, batch, splitting, cutoff, field):
    """(phi, E or None) without autograd: far field, pair sweep, self and background terms"""
    N = splitting.bandwidth
    if field:
        cols = [1] * (q.dim() - 1)
        band = nfft_adjoint(q, pos, batch, bandwidth=N, cutoff=cutoff)  # [B, N, N, N, *cols]
        band = band.unsqueeze(4) * splitting.field_coeffs().reshape([1, N, N, N, 4] + cols)
        far = nfft_forward(band, pos, batch, cutoff=cutoff, real_output=not q.is_complex())  # [n, 4, *cols]
        phi, E = far[:, 0], far[:, 1:]
    else:
        phi, E = nfft_fastsum(q, splitting.coeffs, pos, None, batch, None, cutoff=cutoff), None
    z, f = ops.nfft_ewald_near(pos, q, batch, splitting.alpha, splitting.r_cut, field)
    alpha = splitting.alpha
    phi = phi + z - (2.0 * alpha / math.sqrt(math.pi)) * q - (math.pi / (alpha * alpha)) * _set_sums(q, batch)[1]
    return phi, (E + f if field else None)


class NfftEwaldFunction(torch.autograd.Function):
    """``(phi, E)`` of ``nfft_ewald`` (``E`` empty without ``field``).  The operator ``q -> phi`` is real symmetric, so for
    ``g = dL/dphi`` the gradient in ``q`` is the operator applied to ``g``, and the gradient in the positions is
    ``dL/dpos_i = -sum_c (g_ic E[q_c]_i + q_ic E[g_c]_i)``: one field evaluation with ``q`` and ``g`` side by side as
    columns.  First order only (``once_differentiable``); ``E`` is not differentiable."""

    @staticmethod
    def forward(ctx, q, pos, batch, splitting, cutoff, field):
        if batch is not None and batch.requires_grad:
            raise AssertionError("nfft_ewald is differentiable w.r.t. q and pos only, but batch requires grad")
        ctx.splitting, ctx.cutoff = splitting, cutoff
        ctx.save_for_backward(q, pos, batch)
        phi, E = _ewald(q, pos, batch, splitting, cutoff, field)
        if E is None:
            E = q.new_empty(0)
        ctx.mark_non_differentiable(E)
        return phi, E

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _):
        q, pos, batch = ctx.saved_tensors
        need_q, need_pos = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        g = g.contiguous()
        dq = dpos = None
        if need_pos:
            phi, E = _ewald(torch.stack([q, g], 1), pos, batch, ctx.splitting, ctx.cutoff, True)  # [n, (3,) 2, *cols]
            dq = phi[:, 1]
            w = g.unsqueeze(1).conj() * E[:, :, 0] + q.unsqueeze(1).conj() * E[:, :, 1]
            w = w.real if w.is_complex() else w
            dpos = -w.reshape(w.size(0), 3, math.prod(w.shape[2:])).sum(2)
        elif need_q:
            dq = _ewald(g, pos, batch, ctx.splitting, ctx.cutoff, False)[0]
        return dq if need_q else None, dpos, None, None, None, None


def _check(what, q, pos, batch, splitting):
    if not isinstance(splitting, EwaldSplitting):
        raise TypeError("%s: splitting must be an EwaldSplitting" % what)
    if pos.dim() != 2 or pos.size(1) != 3:
        raise ValueError("%s: the periodic 1/r sum is three-dimensional, pos must be [n, 3]" % what)
    if batch is not None and batch.requires_grad:
        raise AssertionError("%s is differentiable w.r.t. q and pos only, but batch requires grad" % what)


def nfft_ewald(q, pos, batch=None, /, splitting=None, cutoff=4, field=False):
    """The periodic Coulomb potential ``phi_i = sum'_{j, n} q_j / |x_i - x_j + n|`` of the charges ``q`` ``[n, *cols]``
    (float32 or complex64) at ``pos`` ``[n, 3]`` in the unit box, over the charges of i's point set (``batch``: sorted
    point-set indices, as everywhere) and all their periodic images, in the Ewald sense: the self pair is left out, and
    a point set that is not neutral gets a uniform neutralising background.  Any real positions are accepted; they are
    taken modulo 1.  Coincident charges do not see each other in the pair sum.

    Returns ``phi`` with the shape and dtype of ``q``; with ``field=True`` ``(phi, E)``, ``E = -grad phi`` ``[n, 3, *cols]``.
    ``splitting`` is an ``EwaldSplitting``; the far part is ``nfft_fastsum`` with ``splitting.coeffs`` (with ``field``: one
    adjoint and one forward transform that carries the 1 + 3 coefficient arrays as further columns), the near part one
    native pair sweep, then the self and background terms.

    Differentiable once in ``q`` and ``pos`` (for ``U = nfft_ewald_energy``, ``-dU/dpos_i = q_i E_i``); ``E`` itself is not
    differentiable, a second derivative raises a RuntimeError, and ``batch`` must not require grad (AssertionError)."""
    _check("nfft_ewald", q, pos, batch, splitting)
    phi, E = NfftEwaldFunction.apply(q, pos, batch, splitting, int(cutoff), bool(field))
    return (phi, E) if field else phi


def nfft_ewald_energy(q, pos, batch=None, /, splitting=None, cutoff=4):
    """``U_b = 1/2 sum_{i in point set b} q_i phi_i`` with ``phi = nfft_ewald(q, pos, batch, ...)``: ``[B, *cols]``, one
    energy per point set and column (bilinear in ``q``: no conjugate for complex charges).  Its gradient in ``pos`` is
    minus the force, ``dU/dpos_i = -q_i E_i`` summed over the columns."""
    _check("nfft_ewald_energy", q, pos, batch, splitting)
    phi = nfft_ewald(q, pos, batch, splitting=splitting, cutoff=cutoff)
    return 0.5 * _set_sums(q * phi, batch)[0]
