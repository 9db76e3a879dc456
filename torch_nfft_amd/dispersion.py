"""Ewald summation for the periodic 1/r^6: the dispersion sum of a periodic box (LJ-PME with geometric mixing), NFFT far
field + wrapped pair sum (no reference counterpart; Essmann et al., J. Chem. Phys. 103, 8577 (1995);
in 't Veld, Ismail, Grest, J. Chem. Phys. 127, 144711 (2007)).

Notation as in ``ewald.py``: integer frequency ``k``, ``kappa = A^-1 k``, ``V = det A``, ``x = s A`` with fractional ``s`` in
``[-1/2, 1/2)^3``; the unit cube is ``A = I``.  For coefficients ``c_j`` at ``x_j``::

    psi_i = sum'_{j, n} c_j / |x_i - x_j + n|^6        (absolutely convergent; only the pair j = i, n = 0 is left out)
          =   sum_{j: 0 < r_ij < r_c} w(r_ij) c_j                              near: w(r) = e^(-a^2) (1 + a^2 + a^4 / 2) / r^6, a = alpha r
            + sum_k b_k e^{2 pi i k.s_i} sum_j c_j e^{-2 pi i k.s_j}           far:  b_k = pi^(3/2) alpha^3 f(b) / (3 V), b = pi |kappa| / alpha,
                                                                                     f(b) = (1 - 2 b^2) e^(-b^2) + 2 sqrt(pi) b^3 erfc(b)
            - (alpha^6 / 6) c_i                                                self: the smooth far kernel at r = 0
    G_i   = -grad_x psi_i

Against the Coulomb sum: ``b_0 = pi^(3/2) alpha^3 / (3 V)`` is kept (``f(0) = 1``: the sum converges absolutely, its
``k = 0`` term is finite), so there is no background term and no neutrality to ask for.  The far part is ``nfft_fastsum`` on
the whole torus with ``b`` (cut to ``k in [-N/2, N/2)^3``, the unpaired planes ``k_a = -N/2`` zeroed), the near part one
native pair sweep (``ops.nfft_ewald_dispersion_near`` / ``_near_box``).
"""
import math

import torch
from torch.autograd.function import once_differentiable

from . import ops
from . import exclusions as _exclusions
from .ewald import _IDENTITY6, _TorusSplitting, _fractional, _set_sums, _symmetric_backward, _voigt_to_matrix
from .nfft import nfft_adjoint, nfft_forward, nfft_fastsum


def _pair_factor(a):
    """``e^(-a^2) (1 + a^2 + a^4 / 2)``: what is left of ``1 / r^6`` in the pair sum at ``a = alpha r``"""
    a2 = a * a
    return math.exp(-a2) * (1.0 + a2 + 0.5 * a2 * a2)


def _far_factor(b):
    """``f(b) = (1 - 2 b^2) e^(-b^2) + 2 sqrt(pi) b^3 erfc(b)`` of a float64 tensor, clamped at 0: ``f(0) = 1``, decreasing,
    ``f ~ 3 e^(-b^2) / (2 b^2)`` for large ``b``, where the two terms cancel (to nothing that float32 could hold)"""
    b2 = b * b
    f = (1.0 - 2.0 * b2) * torch.exp(-b2) + 2.0 * math.sqrt(math.pi) * b2 * b * torch.special.erfc(b)
    return f.clamp(min=0.0)


def _strain_factor(b):
    """``f'(b) / (6 b) = sqrt(pi) b erfc(b) - e^(-b^2)`` of a float64 tensor, clamped at 0 from above: ``-1`` at ``b = 0``,
    increasing, ``~ -e^(-b^2) / (2 b^2)`` for large ``b``"""
    return (math.sqrt(math.pi) * b * torch.special.erfc(b) - torch.exp(-b * b)).clamp(max=0.0)


class DispersionSplitting(_TorusSplitting):
    """The three parameters of the dispersion split, the box and the far field's coefficients: the counterpart of
    ``EwaldSplitting`` for ``1 / r^6``, with the same arguments, checks, box conventions and attributes (``alpha``,
    ``r_cut``, ``bandwidth``, ``box``, ``volume``, ``widths``, ``cells``, ``box6``).

    ``coeffs`` is ``[N, N, N]`` float32 on ``device``: ``b_k = pi^(3/2) alpha^3 f(pi |kappa| / alpha) / (3 V)`` at index
    ``k + N/2``, evaluated in float64 on the host, ``b_0`` kept and the unpaired planes ``k_a = -N/2`` zeroed."""
    _A_NAME = "a DispersionSplitting"

    def __init__(self, alpha, r_cut, bandwidth, box=None, device="cuda"):
        k2 = self._setup(alpha, r_cut, bandwidth, box)
        b = (math.pi ** 1.5 * self.alpha ** 3 / (3.0 * self.volume)) * _far_factor((math.pi / self.alpha) * torch.sqrt(k2))
        self._b64 = self._zero_unpaired(b)
        self.coeffs = b.to(torch.float32).to(torch.device(device)).contiguous()
        self._strain_coeffs = None

    @classmethod
    def from_tolerance(cls, tol, r_cut, box=None, device="cuda"):
        """``alpha`` solves ``e^(-a^2) (1 + a^2 + a^4 / 2) = tol`` at ``a = alpha r_cut`` (by bisection), and ``bandwidth`` is
        the first even integer ``N`` with ``f(b) <= tol`` at ``b = pi (N/2) / (alpha max_a |a_a|)``, the plane ``k_a = N/2``
        of the longest lattice vector (the grid is cubic in ``N``, as for ``EwaldSplitting``).  These are the factors by
        which the two sums are cut relative to ``1 / r^6`` at ``r_cut`` and to ``b_0``.  A rule of thumb, not a bound: the
        errors also carry the number of points and the density of pairs and of frequencies at the two cuts."""
        tol, r_cut, A, longest = cls._tolerance_box(tol, r_cut, box)
        lo, hi = 0.0, 1.0
        while _pair_factor(hi) > tol:
            hi *= 2.0
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            if _pair_factor(mid) > tol:
                lo = mid
            else:
                hi = mid
        alpha = hi / r_cut  # (the side on which the factor is <= tol)
        N = 2
        while float(_far_factor(torch.tensor(math.pi * (N // 2) / (alpha * longest), dtype=torch.float64))) > tol:
            N += 2
        return cls(alpha, r_cut, N, box=A, device=device)

    def field_coeffs(self):
        """``[N, N, N, 4]`` complex64: ``b_k`` and the three Cartesian components ``(+2 pi i kappa_b) b_k`` -- the
        coefficients of ``psi`` and of ``G = -grad_x psi`` as four columns of one forward transform, in the convention of
        ``EwaldSplitting.field_coeffs`` (from the float64 values on the host; built on first use)."""
        if self._field_coeffs is None:
            b = self._b64
            cols = [torch.complex(b, torch.zeros_like(b))]
            kappa = self._kappa()
            for a in range(3):
                cols.append(torch.complex(torch.zeros_like(b), 2.0 * math.pi * kappa[..., a] * b))
            self._field_coeffs = torch.stack(cols, 3).to(torch.complex64).to(self.coeffs.device).contiguous()
        return self._field_coeffs

    def strain_coeffs(self):
        """``[N, N, N]`` float32 on the device of ``coeffs``: ``t_k = (d b_k / d |kappa|) / |kappa| = (2 pi^(7/2) alpha / V)
        (sqrt(pi) b erfc(b) - e^(-b^2))``, ``b = pi |kappa| / alpha`` -- what the strain ``A -> A (1 + eps)`` does to ``b_k``,
        ``d b_k / d eps_ab = -t_k kappa_a kappa_b`` beside the volume's ``-b_k delta_ab`` (``nfft_ewald_dispersion_virial``).
        Evaluated in float64 on the host (the two terms cancel to ``-e^(-b^2) / (2 b^2)`` at large ``b``), clamped at ``<= 0``,
        finite at ``k = 0`` and zero wherever ``coeffs`` is zero (the unpaired planes ``k_a = -N/2``, and cells whose ``b_k`` is
        below float32: the native reduction skips them); built on first use."""
        if self._strain_coeffs is None:
            b = (math.pi / self.alpha) * torch.sqrt((self._kappa() ** 2).sum(3))
            t = (2.0 * math.pi ** 3.5 * self.alpha / self.volume) * _strain_factor(b)
            t[self.coeffs.cpu() == 0] = 0.0
            self._strain_coeffs = t.to(torch.float32).to(self.coeffs.device).contiguous()
        return self._strain_coeffs


def _dispersion(c, pos, batch, splitting, cutoff, field, exclusions=None):
    """(psi, G or None) without autograd: far field, pair sweep, self term (with a box: ``pos`` fractional, ``G``
    Cartesian).  The listed pairs of ``exclusions`` are taken out of the pair sweep's sums before anything else is added to
    them, as in ``ewald._ewald``."""
    N = splitting.bandwidth
    if field:
        cols = [1] * (c.dim() - 1)
        band = nfft_adjoint(c, pos, batch, bandwidth=N, cutoff=cutoff)  # [B, N, N, N, *cols]
        band = band.unsqueeze(4) * splitting.field_coeffs().reshape([1, N, N, N, 4] + cols)
        far = nfft_forward(band, pos, batch, cutoff=cutoff, real_output=not c.is_complex())  # [n, 4, *cols]
        psi, G = far[:, 0], far[:, 1:]
    else:
        psi, G = nfft_fastsum(c, splitting.coeffs, pos, None, batch, None, cutoff=cutoff), None
    alpha = splitting.alpha
    if splitting.box is not None:
        z, f = ops.nfft_ewald_dispersion_near_box(pos, c, batch, splitting.box6, alpha, splitting.r_cut, field)
    else:
        z, f = ops.nfft_ewald_dispersion_near(pos, c, batch, alpha, splitting.r_cut, field)
    if exclusions is not None:
        zx, fx = _exclusions.correction(_exclusions.DISPERSION, c, pos, batch, splitting, exclusions, field)
        z, f = z - zx, (f - fx if field else f)
    psi = psi + z - (alpha ** 6 / 6.0) * c
    return psi, (G + f if field else None)


class NfftEwaldDispersionFunction(torch.autograd.Function):
    """``(psi, G)`` of ``nfft_ewald_dispersion`` (``G`` empty without ``field``), on the pattern of ``NfftEwaldFunction``:
    the operator ``c -> psi`` is real symmetric, so ``dL/dc`` is the operator applied to ``g = dL/dpsi`` and
    ``dL/dpos_i = -sum_c (g_ic G[c]_i + c_ic G[g]_i)`` (times ``A^T`` for the fractional positions of a box).  First
    order only (``once_differentiable``); ``G`` is not differentiable."""

    @staticmethod
    def forward(ctx, c, pos, batch, splitting, cutoff, field, exclusions=None):
        if batch is not None and batch.requires_grad:
            raise AssertionError("nfft_ewald_dispersion is differentiable w.r.t. c and pos only, but batch requires grad")
        ctx.splitting, ctx.cutoff, ctx.exclusions = splitting, cutoff, exclusions
        ctx.save_for_backward(c, pos, batch)
        psi, G = _dispersion(c, pos, batch, splitting, cutoff, field, exclusions)
        if G is None:
            G = c.new_empty(0)
        ctx.mark_non_differentiable(G)
        return psi, G

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _):
        return _symmetric_backward(_dispersion, ctx, g) + (None,)


def _check(what, c, pos, batch, splitting, differentiable=True):
    if not isinstance(splitting, DispersionSplitting):
        raise TypeError("%s: splitting must be a DispersionSplitting" % what)
    if pos.dim() != 2 or pos.size(1) != 3:
        raise ValueError("%s: the periodic 1/r^6 sum is three-dimensional, pos must be [n, 3]" % what)
    if batch is not None and batch.requires_grad:
        if differentiable:
            raise AssertionError("%s is differentiable w.r.t. c and pos only, but batch requires grad" % what)
        raise AssertionError("%s: batch holds point-set indices and must not require grad" % what)


def nfft_ewald_dispersion(c, pos, batch=None, /, splitting=None, cutoff=4, field=False, fractional=False, exclusions=None):
    """The periodic dispersion sum ``psi_i = sum'_{j, n} c_j / |x_i - x_j + n|^6`` of the coefficients ``c`` ``[n, *cols]``
    (float32 or complex64) at ``pos`` ``[n, 3]``, over the points of i's point set (``batch``: sorted point-set indices) and
    all their periodic images; only the self pair is left out.  The sum converges absolutely: no background, no
    neutrality.  Coincident points do not see each other in the pair sum, and pairs closer than ``1.6e-5`` overflow
    float32 in the field (``1 / r^8``).

    Returns ``psi`` with the shape and dtype of ``c``; with ``field=True`` ``(psi, G)``, ``G = -grad_x psi``
    ``[n, 3, *cols]``.  ``splitting`` is a ``DispersionSplitting`` (TypeError otherwise); positions, boxes, ``fractional`` and
    ``cutoff`` are those of ``nfft_ewald``: the far part is ``nfft_fastsum`` with ``splitting.coeffs`` (with ``field``: one
    adjoint and one forward transform with 1 + 3 coefficient arrays), the near part one native pair sweep, then
    ``-(alpha^6 / 6) c``.  That self term cancels against the far sum: a sparse point set (few neighbours within
    ``r_cut``) loses the digits of that cancellation.

    Differentiable once in ``c`` and ``pos``; ``G`` itself is not differentiable, a second derivative raises a
    RuntimeError, and ``batch`` must not require grad (AssertionError).  The gradient comes back in the coordinates that
    were passed.

    ``exclusions`` is ``None`` or an ``ExclusionList`` over the ``n`` points (TypeError, ValueError as for ``nfft_ewald``):
    every listed pair ``{i, j}`` loses ``(1 - s^D_ij) c_j / r^6`` in ``psi_i`` and ``6 (1 - s^D_ij) c_j d_ij / r^8`` in ``G_i``
    for the one image that the sweep sees (a pair at ``r = 0``: ``(1 - s^D_ij) c_j alpha^6 / 6`` and no field), by one more
    native call; the gradients are those of the corrected sum.  The sweep has added the pair before the correction
    removes it: an excluded pair leaves a rounding of about ``2^-24 |c_j| / r^6`` in ``psi_i`` (``exclusions.py``)."""
    _check("nfft_ewald_dispersion", c, pos, batch, splitting)
    exclusions = _exclusions.check_exclusions("nfft_ewald_dispersion", exclusions, pos)
    pos = _fractional("nfft_ewald_dispersion", pos, splitting, fractional)
    if exclusions is None:
        psi, G = NfftEwaldDispersionFunction.apply(c, pos, batch, splitting, int(cutoff), bool(field))
    else:
        psi, G = NfftEwaldDispersionFunction.apply(c, pos, batch, splitting, int(cutoff), bool(field), exclusions)
    return (psi, G) if field else psi


def nfft_ewald_dispersion_energy(c, pos, batch=None, /, splitting=None, cutoff=4, fractional=False, exclusions=None):
    """``U_b = 1/2 sum_{i in point set b} c_i psi_i`` with ``psi = nfft_ewald_dispersion(c, pos, batch, ...)``:
    ``[B, *cols]``, one value per point set and column (bilinear in ``c``).  The physical dispersion energy of the pair
    coefficients ``C6_ij = c_i c_j`` (geometric mixing) is its NEGATIVE, ``-U``: the attraction is ``-C6 / r^6``.
    ``dU/dpos_i = -c_i G_i`` summed over the columns.  ``exclusions`` as for ``nfft_ewald_dispersion``: every listed pair loses
    ``(1 - s^D_ij) c_i c_j / r^6``."""
    _check("nfft_ewald_dispersion_energy", c, pos, batch, splitting)
    if splitting.box is None and fractional:
        raise ValueError("nfft_ewald_dispersion_energy: fractional=True needs a DispersionSplitting with a box")
    psi = nfft_ewald_dispersion(c, pos, batch, splitting=splitting, cutoff=cutoff, fractional=fractional, exclusions=exclusions)
    return 0.5 * _set_sums(c * psi, batch)[0]


def nfft_ewald_dispersion_virial(c, pos, batch=None, /, splitting=None, cutoff=4, fractional=False, exclusions=None):
    """``(U, W)``: ``U_b = 1/2 sum_{i in point set b} c_i psi_i`` ``[B, *cols]`` of ``nfft_ewald_dispersion_energy`` and the
    virial tensor ``W_ab = -dU / d eps_ab`` ``[B, 3, 3, *cols]`` for the homogeneous strain ``A -> A (1 + eps)`` of the box at
    fixed fractional coordinates, per point set and column, both with the dtype of ``c``: the counterpart of
    ``nfft_ewald_virial`` for ``1 / r^6``.  ``W`` is symmetric and in the box's units (energy);
    ``psi`` is homogeneous of degree -6 in the box, so ``tr W = 6 U`` up to the truncation of the sum (``tr W = U`` for
    ``1/r``).  The signs are those of ``nfft_ewald_dispersion_energy``: the physical dispersion energy and virial of the pair
    coefficients ``C6_ij = c_i c_j`` are the NEGATIVES ``-U`` and ``-W``, ``-W / splitting.volume`` is the dispersion part of
    the pressure tensor, and ``virial_to_box_gradient(W, splitting.box)`` is the gradient of ``U`` in the box's entries.

    ``c`` ``[n, *cols]`` must be real (float32): the energy is bilinear and for complex coefficients the far part is not
    ``|S_k|^2`` (ValueError).  ``pos``, ``batch``, ``cutoff`` and ``fractional`` are those of ``nfft_ewald_dispersion``,
    ``splitting`` a ``DispersionSplitting`` (TypeError otherwise); without a box the cell is the unit cube.

    One adjoint transform, then two native reductions in float64 and without atomics -- over the frequencies of its output,
    ``1/2 sum_k |S_k|^2 (b_k, b_k delta_ab + t_k kappa_a kappa_b)`` with ``t = splitting.strain_coeffs()``, and over the pairs
    within ``r_cut``, ``1/2 sum_ij c_i c_j (w, mg d_a d_b)`` -- and the self term ``-(alpha^6 / 12) sum c_i^2`` (in ``U`` only: it
    has no strain in it) added in float64 before the cast.  The ``k = 0`` term is part of both sums: no background.  With
    ``exclusions`` (as for ``nfft_ewald_dispersion``) a third native reduction takes ``(1 - s^D_ij) c_i c_j / r^6`` out of ``U`` and
    ``6 (1 - s^D_ij) c_i c_j d_a d_b / r^8`` out of ``W`` for every listed pair (``tr W = 6 U`` stays; a pair at ``r = 0``:
    ``(1 - s^D_ij) c_i c_j alpha^6 / 6`` in ``U`` only).

    Runs under ``torch.no_grad()``: ``U`` and ``W`` are constants to autograd.  Inputs that require grad are accepted and
    get no gradient from here (use ``nfft_ewald_dispersion_energy`` for forces); ``batch`` must not require grad
    (AssertionError)."""
    _check("nfft_ewald_dispersion_virial", c, pos, batch, splitting, differentiable=False)
    if c.is_complex():
        raise ValueError("nfft_ewald_dispersion_virial: the coefficients must be real (the energy is bilinear in c)")
    exclusions = _exclusions.check_exclusions("nfft_ewald_dispersion_virial", exclusions, pos)
    with torch.no_grad():
        c, pos = c.detach(), pos.detach()
        pos = _fractional("nfft_ewald_dispersion_virial", pos, splitting, fractional)
        alpha, N = splitting.alpha, splitting.bandwidth
        box6 = _IDENTITY6 if splitting.box is None else splitting.box6
        band = nfft_adjoint(c, pos, batch, bandwidth=N, cutoff=int(cutoff))  # [B, N, N, N, *cols]
        seven = ops.nfft_ewald_dispersion_virial_far(band, splitting.coeffs, splitting.strain_coeffs(), box6)
        seven = seven + ops.nfft_ewald_dispersion_virial_near(pos, c, batch, box6, alpha, splitting.r_cut)  # [B, 7, *cols] float64
        if exclusions is not None:
            seven = seven - _exclusions.virial_correction(_exclusions.DISPERSION, c, pos, batch, splitting, exclusions)
        c64 = c.double()
        U = seven[:, 0] - (alpha ** 6 / 12.0) * _set_sums(c64 * c64, batch)[0]
        return U.to(c.dtype), _voigt_to_matrix(seven[:, 1:]).to(c.dtype)
