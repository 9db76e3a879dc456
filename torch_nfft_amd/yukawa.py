"""Ewald summation for the periodic screened Coulomb (Yukawa) potential e^(-lambda r) / r: the pair potential of dusty and
strongly coupled plasmas, of charged colloids (DLVO) and of Debye-Hueckel electrolytes, NFFT far field + wrapped pair sum (no
reference counterpart; Salin and Caillol, J. Chem. Phys. 113, 10459 (2000)).

Notation as in ``ewald.py``: integer frequency ``k``, ``kappa = A^-1 k``, ``V = det A``, ``x = s A`` with fractional ``s`` in
``[-1/2, 1/2)^3``; the unit cube is ``A = I``.  The screening parameter is ``lambda`` (the keyword ``screening``),
``beta = lambda / (2 alpha)`` and ``K_k = 4 pi^2 |kappa|^2 + lambda^2``.  For charges ``q_j`` at ``x_j``::

    phi_i = sum'_{j, n} q_j e^(-lambda |x_ij + n|) / |x_ij + n|        (absolutely convergent for lambda > 0; only j = i, n = 0 left out)
          =   sum_{j: 0 < r_ij < r_c} w(r_ij) q_j                       near
            + sum_k b_k e^{2 pi i k.s_i} sum_j q_j e^{-2 pi i k.s_j}    far:  b_k = 4 pi e^(-K_k / (4 alpha^2)) / (V K_k), k = 0 INCLUDED
            - q_i ((2 alpha / sqrt(pi)) e^(-beta^2) - lambda erfc(beta))  self
    E_i   = -grad_x phi_i

    w(r)  = (e^(lambda r) erfc(alpha r + beta) + e^(-lambda r) erfc(alpha r - beta)) / (2 r)
    D(r)  = (e^(lambda r) erfc(alpha r + beta) - e^(-lambda r) erfc(alpha r - beta)) / 2          (<= 0)
    g(r)  = (2 alpha / sqrt(pi)) e^(-alpha^2 r^2 - beta^2)
    mg(r) = -w'(r) / r = (w - lambda D + g) / r^2

At ``lambda = 0`` these are the Coulomb weights of ``ewald.py``, and ``w <= erfc(alpha r) / r`` everywhere.  The sum converges
without a background; ``background=True`` on the splitting gives the convention of the one-component plasma, in which the
charges move in a uniform neutralising background that is screened too: ``b_0 = 0`` and ``phi_i += Q (4 pi / (V lambda^2))
expm1(-beta^2)`` with ``Q`` the total charge of the point set.  Then ``phi - lambda q`` tends to the ``phi`` of ``nfft_ewald`` as
``lambda -> 0``, with a remainder of the order ``lambda^2`` (the ``lambda q_i`` is the ``-lambda`` of ``e^(-lambda r) / r = 1/r -
lambda + ...`` in the self pair that is left out).

The virial (``nfft_ewald_yukawa_virial``) is taken for the strain ``A -> A (1 + eps)`` at fixed fractional coordinates and FIXED
``lambda``: ``lambda`` carries a length, so ``tr W != U``.  With ``W_ab = -dU / d eps_ab`` and ``U = 1/2 sum q_i phi_i``::

    near:  1/2 sum_i q_i sum_j (w, mg d_a d_b) q_j
    far:   1/2 sum_k |S_k|^2 (b_k, b_k delta_ab + t_k kappa_a kappa_b),   t_k = -8 pi^2 b_k (1 / (4 alpha^2) + 1 / K_k)
    self:  -1/2 ((2 alpha / sqrt(pi)) e^(-beta^2) - lambda erfc(beta)) sum q_i^2          in U only
    background=True:  U_bg = 1/2 Q^2 (4 pi / (V lambda^2)) expm1(-beta^2)             added to U and to W_aa (U_bg ~ 1 / V)

The far line is the reduction of the dispersion sum's virial (``ops.nfft_ewald_dispersion_virial_far``) with this sum's grids.
Out of scope: ``exclusions=`` for this sum, second derivatives, gradients in ``lambda`` or the box (the virial covers the box),
one ``lambda`` per species.
"""
import math

import torch
from torch.autograd.function import once_differentiable

from . import ops
from .ewald import _IDENTITY6, _TorusSplitting, _fractional, _set_sums, _symmetric_backward, _voigt_to_matrix
from .nfft import nfft_adjoint, nfft_forward, nfft_fastsum

MAX_SCREENING_R_CUT = 50.0  # the native sweep's bound on lambda r_cut (float32 exponentials; e^-50 / r_cut is nothing to sum)


class YukawaSplitting(_TorusSplitting):
    """The parameters of the screened Coulomb split, the box and the far field's coefficients: the counterpart of
    ``EwaldSplitting`` for ``e^(-lambda r) / r``, with the same ``alpha``, ``r_cut``, ``bandwidth`` and ``box``, their checks, box
    conventions and attributes (``alpha``, ``r_cut``, ``bandwidth``, ``box``, ``volume``, ``widths``, ``cells``, ``box6``), and

    ``screening``: ``lambda``, finite and ``> 0`` in the box's inverse length (ValueError; for ``lambda = 0`` use
    ``EwaldSplitting``, whose ``k = 0`` term needs the background that this sum can do without) with
    ``screening * r_cut <= 50`` (ValueError: the pair sweep's bound; past it the weight at the cut is below ``e^-50 / r_cut``).
    ``background``: False keeps ``b_0 = 4 pi e^(-beta^2) / (V lambda^2)`` -- the plain lattice sum; True zeroes it and adds the
    screened uniform background of the one-component plasma (the module docstring).

    ``coeffs`` is ``[N, N, N]`` float32 on ``device``: ``b_k = 4 pi e^(-K_k / (4 alpha^2)) / (V K_k)`` at index ``k + N/2``,
    evaluated in float64 on the host, the unpaired planes ``k_a = -N/2`` zeroed.  ``self_term`` is the float64 constant
    ``(2 alpha / sqrt(pi)) e^(-beta^2) - lambda erfc(beta)`` and ``background_term`` the float64 constant
    ``(4 pi / (V lambda^2)) expm1(-beta^2)`` (0.0 without ``background``)."""
    _A_NAME = "a YukawaSplitting"

    def __init__(self, alpha, r_cut, bandwidth, screening, box=None, background=False, device="cuda"):
        lam = float(screening)
        if lam == 0.0:
            raise ValueError("YukawaSplitting: screening must be positive; screening = 0 is the Coulomb sum: use EwaldSplitting")
        if not (lam > 0.0 and math.isfinite(lam)):
            raise ValueError("YukawaSplitting: screening must be positive and finite")
        k2 = self._setup(alpha, r_cut, bandwidth, box)
        if not lam * self.r_cut <= MAX_SCREENING_R_CUT:
            raise ValueError("YukawaSplitting: screening * r_cut <= 50 is required (at 50 the pair weight at r_cut is below "
                             "e^-50 / r_cut: no Ewald split is needed there)")
        self.screening, self.background = lam, bool(background)
        N, beta = self.bandwidth, lam / (2.0 * self.alpha)
        K = 4.0 * math.pi ** 2 * k2 + lam * lam
        b = 4.0 * math.pi * torch.exp(-K / (4.0 * self.alpha ** 2)) / (self.volume * K)
        if self.background:
            b[N // 2, N // 2, N // 2] = 0.0
        self._b64 = self._zero_unpaired(b)
        self._K = K
        self.coeffs = b.to(torch.float32).to(torch.device(device)).contiguous()
        self._strain_coeffs = None
        self.self_term = 2.0 * self.alpha / math.sqrt(math.pi) * math.exp(-beta * beta) - lam * math.erfc(beta)
        self.background_term = 4.0 * math.pi / (self.volume * lam * lam) * math.expm1(-beta * beta) if self.background else 0.0

    @classmethod
    def from_tolerance(cls, tol, r_cut, screening, box=None, background=False, device="cuda"):
        """``alpha`` and ``bandwidth`` of ``EwaldSplitting.from_tolerance(tol, r_cut, box)``: ``alpha = sqrt(-ln tol) / r_cut`` and
        ``N`` the next even integer ``>= 2 alpha sqrt(-ln tol) max_a |a_a| / pi``.  For this sum they are upper bounds: the pair
        weight is below the Coulomb one, ``w <= erfc(alpha r) / r``, and so are the coefficients, ``b_k <= e^(-pi^2 |kappa|^2 /
        alpha^2) / (pi V |kappa|^2)``, so both truncations are at most what they are for ``1/r`` -- by the factor ``e^(-lambda
        r_cut)`` or so in the pair sum, which a large ``lambda`` would let one spend on a smaller ``alpha``.  A rule of thumb
        all the same, as there."""
        tol, r_cut, A, longest = cls._tolerance_box(tol, r_cut, box)
        s = math.sqrt(-math.log(tol))
        alpha = s / r_cut
        N = max(2, 2 * math.ceil(alpha * s * longest / math.pi))
        return cls(alpha, r_cut, N, screening, box=A, background=background, device=device)

    def field_coeffs(self):
        """``[N, N, N, 4]`` complex64: ``b_k`` and the three Cartesian components ``(+2 pi i kappa_b) b_k`` -- the
        coefficients of ``phi`` and of ``E = -grad_x phi`` as four columns of one forward transform, in the convention of
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
        """``[N, N, N]`` float32 on the device of ``coeffs``: ``t_k = (d b_k / d |kappa|) / |kappa| = -8 pi^2 b_k (1 / (4 alpha^2)
        + 1 / K_k)`` at fixed ``lambda`` -- what the strain ``A -> A (1 + eps)`` does to ``b_k``, ``d b_k / d eps_ab = -t_k kappa_a
        kappa_b`` beside the volume's ``-b_k delta_ab`` (``nfft_ewald_yukawa_virial``).  From the float64 values on the host,
        zero wherever ``coeffs`` is zero (the unpaired planes, ``k = 0`` with ``background``, and cells whose ``b_k`` is below
        float32: the native reduction skips them); built on first use."""
        if self._strain_coeffs is None:
            t = -8.0 * math.pi ** 2 * self._b64 * (1.0 / (4.0 * self.alpha ** 2) + 1.0 / self._K)
            t[self.coeffs.cpu() == 0] = 0.0
            self._strain_coeffs = t.to(torch.float32).to(self.coeffs.device).contiguous()
        return self._strain_coeffs


def _yukawa(q, pos, batch, splitting, cutoff, field):
    """(phi, E or None) without autograd: far field, pair sweep, self and background terms (with a box: ``pos`` fractional,
    ``E`` Cartesian)"""
    N = splitting.bandwidth
    if field:
        cols = [1] * (q.dim() - 1)
        band = nfft_adjoint(q, pos, batch, bandwidth=N, cutoff=cutoff)  # [B, N, N, N, *cols]
        band = band.unsqueeze(4) * splitting.field_coeffs().reshape([1, N, N, N, 4] + cols)
        far = nfft_forward(band, pos, batch, cutoff=cutoff, real_output=not q.is_complex())  # [n, 4, *cols]
        phi, E = far[:, 0], far[:, 1:]
    else:
        phi, E = nfft_fastsum(q, splitting.coeffs, pos, None, batch, None, cutoff=cutoff), None
    box6 = () if splitting.box is None else splitting.box6
    z, f = ops.nfft_ewald_yukawa_near(pos, q, batch, box6, splitting.alpha, splitting.r_cut, splitting.screening, field)
    phi = phi + z - splitting.self_term * q
    if splitting.background:
        phi = phi + splitting.background_term * _set_sums(q, batch)[1]
    return phi, (E + f if field else None)


class NfftEwaldYukawaFunction(torch.autograd.Function):
    """``(phi, E)`` of ``nfft_ewald_yukawa`` (``E`` empty without ``field``), on the pattern of ``NfftEwaldFunction``: the
    operator ``q -> phi`` is real symmetric, so ``dL/dq`` is the operator applied to ``g = dL/dphi`` and
    ``dL/dpos_i = -sum_c (g_ic E[q]_i + q_ic E[g]_i)`` (times ``A^T`` for the fractional positions of a box).  First order
    only (``once_differentiable``); ``E`` is not differentiable."""

    @staticmethod
    def forward(ctx, q, pos, batch, splitting, cutoff, field):
        if batch is not None and batch.requires_grad:
            raise AssertionError("nfft_ewald_yukawa is differentiable w.r.t. q and pos only, but batch requires grad")
        ctx.splitting, ctx.cutoff = splitting, cutoff
        ctx.save_for_backward(q, pos, batch)
        phi, E = _yukawa(q, pos, batch, splitting, cutoff, field)
        if E is None:
            E = q.new_empty(0)
        ctx.mark_non_differentiable(E)
        return phi, E

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _):
        return _symmetric_backward(_yukawa, ctx, g)


def _check(what, q, pos, batch, splitting, differentiable=True):
    if not isinstance(splitting, YukawaSplitting):
        raise TypeError("%s: splitting must be a YukawaSplitting" % what)
    if pos.dim() != 2 or pos.size(1) != 3:
        raise ValueError("%s: the periodic screened Coulomb sum is three-dimensional, pos must be [n, 3]" % what)
    if batch is not None and batch.requires_grad:
        if differentiable:
            raise AssertionError("%s is differentiable w.r.t. q and pos only, but batch requires grad" % what)
        raise AssertionError("%s: batch holds point-set indices and must not require grad" % what)


def nfft_ewald_yukawa(q, pos, batch=None, /, splitting=None, cutoff=4, field=False, fractional=False):
    """The periodic screened Coulomb potential ``phi_i = sum'_{j, n} q_j e^(-lambda |x_i - x_j + n|) / |x_i - x_j + n|`` of the
    charges ``q`` ``[n, *cols]`` (float32 or complex64) at ``pos`` ``[n, 3]``, over the points of i's point set (``batch``: sorted
    point-set indices) and all their periodic images; only the self pair is left out.  The sum converges absolutely: no
    neutrality is asked for, and the background is a choice of the splitting (``YukawaSplitting(..., background=True)``).
    Coincident points do not see each other in the pair sum.

    Returns ``phi`` with the shape and dtype of ``q``; with ``field=True`` ``(phi, E)``, ``E = -grad_x phi`` ``[n, 3, *cols]``.
    ``splitting`` is a ``YukawaSplitting`` (TypeError otherwise); positions, boxes, ``fractional`` and ``cutoff`` are those of
    ``nfft_ewald``: the far part is ``nfft_fastsum`` with ``splitting.coeffs`` (with ``field``: one adjoint and one forward
    transform with 1 + 3 coefficient arrays), the near part one native pair sweep, then the self and background terms.

    Differentiable once in ``q`` and ``pos``; ``E`` itself is not differentiable, a second derivative raises a RuntimeError,
    and ``batch`` must not require grad (AssertionError).  The gradient comes back in the coordinates that were passed.
    There is no gradient in ``screening`` or the box, and no ``exclusions=`` for this sum."""
    _check("nfft_ewald_yukawa", q, pos, batch, splitting)
    pos = _fractional("nfft_ewald_yukawa", pos, splitting, fractional)
    phi, E = NfftEwaldYukawaFunction.apply(q, pos, batch, splitting, int(cutoff), bool(field))
    return (phi, E) if field else phi


def nfft_ewald_yukawa_energy(q, pos, batch=None, /, splitting=None, cutoff=4, fractional=False):
    """``U_b = 1/2 sum_{i in point set b} q_i phi_i`` with ``phi = nfft_ewald_yukawa(q, pos, batch, ...)``: ``[B, *cols]``, one
    energy per point set and column (bilinear in ``q``: no conjugate for complex charges).  ``dU/dpos_i = -q_i E_i`` summed
    over the columns."""
    _check("nfft_ewald_yukawa_energy", q, pos, batch, splitting)
    if splitting.box is None and fractional:
        raise ValueError("nfft_ewald_yukawa_energy: fractional=True needs a YukawaSplitting with a box")
    phi = nfft_ewald_yukawa(q, pos, batch, splitting=splitting, cutoff=cutoff, fractional=fractional)
    return 0.5 * _set_sums(q * phi, batch)[0]


def nfft_ewald_yukawa_virial(q, pos, batch=None, /, splitting=None, cutoff=4, fractional=False):
    """``(U, W)``: ``U_b = 1/2 sum_{i in point set b} q_i phi_i`` ``[B, *cols]`` of ``nfft_ewald_yukawa_energy`` and the virial
    tensor ``W_ab = -dU / d eps_ab`` ``[B, 3, 3, *cols]`` for the homogeneous strain ``A -> A (1 + eps)`` of the box at fixed
    fractional coordinates and fixed ``lambda``, per point set and column, both with the dtype of ``q``: the counterpart of
    ``nfft_ewald_virial`` for ``e^(-lambda r) / r``.  ``W`` is symmetric and in the box's units (energy); ``lambda`` carries a
    length, so ``tr W`` is not ``U``.  ``W / splitting.volume`` is this interaction's part of the pressure tensor, and
    ``virial_to_box_gradient(W, splitting.box)`` the gradient of ``U`` in the box's entries.

    ``q`` ``[n, *cols]`` must be real (float32): the energy is bilinear and for complex charges the far part is not
    ``|S_k|^2`` (ValueError).  ``pos``, ``batch``, ``cutoff`` and ``fractional`` are those of ``nfft_ewald_yukawa``, ``splitting`` a
    ``YukawaSplitting`` (TypeError otherwise); without a box the cell is the unit cube.

    One adjoint transform, then two native reductions in float64 and without atomics -- over the frequencies of its output,
    ``1/2 sum_k |S_k|^2 (b_k, b_k delta_ab + t_k kappa_a kappa_b)`` with ``t = splitting.strain_coeffs()`` (the dispersion sum's
    reduction with this sum's grids), and over the pairs within ``r_cut``, ``1/2 sum_ij q_i q_j (w, mg d_a d_b)`` -- and the self
    term ``-1/2 self_term sum q_i^2`` (in ``U`` only: it has no strain in it) and, with ``background``, ``1/2 background_term
    Q^2`` (in ``U`` and on the diagonal of ``W``: it goes like ``1 / V``) added in float64 before the cast.

    Runs under ``torch.no_grad()``: ``U`` and ``W`` are constants to autograd.  Inputs that require grad are accepted and
    get no gradient from here (use ``nfft_ewald_yukawa_energy`` for forces); ``batch`` must not require grad
    (AssertionError)."""
    _check("nfft_ewald_yukawa_virial", q, pos, batch, splitting, differentiable=False)
    if q.is_complex():
        raise ValueError("nfft_ewald_yukawa_virial: the charges must be real (the energy is bilinear in q)")
    with torch.no_grad():
        q, pos = q.detach(), pos.detach()
        pos = _fractional("nfft_ewald_yukawa_virial", pos, splitting, fractional)
        N = splitting.bandwidth
        box6 = _IDENTITY6 if splitting.box is None else splitting.box6
        band = nfft_adjoint(q, pos, batch, bandwidth=N, cutoff=int(cutoff))  # [B, N, N, N, *cols]
        seven = ops.nfft_ewald_dispersion_virial_far(band, splitting.coeffs, splitting.strain_coeffs(), box6)
        seven = seven + ops.nfft_ewald_yukawa_virial_near(pos, q, batch, box6, splitting.alpha, splitting.r_cut,
                                                          splitting.screening)  # [B, 7, *cols] float64
        q64 = q.double()
        U = seven[:, 0] - 0.5 * splitting.self_term * _set_sums(q64 * q64, batch)[0]
        W = _voigt_to_matrix(seven[:, 1:])
        if splitting.background:
            total = _set_sums(q64, batch)[0]
            background = 0.5 * splitting.background_term * total * total
            U = U + background
            for a in range(3):
                W[:, a, a] += background
        return U.to(q.dtype), W.to(q.dtype)
