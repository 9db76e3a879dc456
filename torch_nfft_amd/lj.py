"""Nonbonded step of a Lennard-Jones + Coulomb model in a periodic box: forces, energies and the virial tensor from one pass
(no reference counterpart).

Every point carries a charge ``q_i``, a dispersion coefficient ``c_i`` and a repulsion coefficient ``a_i``, with geometric
mixing for both powers, ``C6_ij = c_i c_j`` and ``C12_ij = a_i a_j``.  With ``lj_coefficients(sigma, epsilon)`` these are
``4 eps_ij sigma_ij^6`` and ``4 eps_ij sigma_ij^12`` for ``eps_ij = sqrt(eps_i eps_j)``, ``sigma_ij = sqrt(sigma_i sigma_j)`` (the
OPLS rule).  The energy of a point set is ``U = U_coulomb + U_lj``::

    U_coulomb = 1/2 sum_i q_i phi_i                               phi: the Ewald sum of ewald.py (tin-foil, self and background terms)
    U_lj      = 1/2 sum_i a_i rho_i - 1/2 sum_i c_i psi_i         psi: the dispersion Ewald sum of dispersion.py (LJ-PME, all images)
    rho_i     = sum_{j: 0 < r_ij < r_cut} a_j / r_ij^12           minimum images, plainly truncated: no shift, no tail correction

The attraction is summed over the whole lattice, the repulsion over the pairs within ``r_cut`` only: what the truncation
leaves out of a pair just beyond the cut is ``a_i a_j / r_cut^12``.

Force fields outside geometric mixing (Lorentz-Berthelot, NBFIX) give their parameters per pair of TYPES in an ``LJPairTable``
and call ``nfft_ewald_lj_table_step``: the grid keeps a per-type geometric ``c_i``, and the pair walk
applies the exact ``C12`` and the difference ``C6 - c_i c_j`` within ``r_cut``.
"""
import math

import torch

from . import ops
from .dispersion import DispersionSplitting
from .exclusions import check_exclusions
from .ewald import EwaldSplitting, _IDENTITY6, _fractional, _set_sums, _voigt_to_matrix
from .nfft import nfft_adjoint, nfft_forward


def lj_coefficients(sigma, epsilon):
    """``(c, a)`` with ``c = 2 sqrt(epsilon) sigma^3`` and ``a = 2 sqrt(epsilon) sigma^6``, elementwise: the per-point
    coefficients whose products are the Lennard-Jones pair coefficients under geometric mixing, ``c_i c_j = 4 eps_ij
    sigma_ij^6`` and ``a_i a_j = 4 eps_ij sigma_ij^12`` with ``eps_ij = sqrt(eps_i eps_j)`` and ``sigma_ij = sqrt(sigma_i
    sigma_j)``.  Pure torch, differentiable, any dtype and device."""
    sigma, epsilon = torch.as_tensor(sigma), torch.as_tensor(epsilon)
    root = 2.0 * torch.sqrt(epsilon)
    s3 = sigma * sigma * sigma
    return root * s3, root * s3 * s3


def _check_splittings(what, coulomb, dispersion):
    if not isinstance(coulomb, EwaldSplitting):
        raise TypeError("%s: coulomb must be an EwaldSplitting" % what)
    if not isinstance(dispersion, DispersionSplitting):
        raise TypeError("%s: dispersion must be a DispersionSplitting" % what)
    if coulomb.r_cut != dispersion.r_cut:
        raise ValueError("%s: the two splittings must have the same r_cut (%r and %r): one walk serves both sums"
                         % (what, coulomb.r_cut, dispersion.r_cut))
    if coulomb.bandwidth != dispersion.bandwidth:
        raise ValueError("%s: the two splittings must have the same bandwidth (%d and %d): one transform serves both sums"
                         % (what, coulomb.bandwidth, dispersion.bandwidth))
    if (coulomb.box is None) != (dispersion.box is None) or (coulomb.box is not None and not torch.equal(coulomb.box, dispersion.box)):
        raise ValueError("%s: the two splittings must have the same box" % what)


def _check_values(what, values, pos):
    """``(q, c, a)`` as three float32 ``[n]`` tensors, ``None`` as zeros"""
    n, out = pos.size(0), []
    for name, v in zip("qca", values):
        if v is None:
            out.append(torch.zeros(n, dtype=torch.float32, device=pos.device))
            continue
        if v.is_complex():
            raise ValueError("%s: %s must be real (the energy is bilinear in it)" % (what, name))
        if v.dim() != 1:
            raise ValueError("%s: %s must be [n]: columns are not supported" % (what, name))
        if v.size(0) != n:
            raise ValueError("%s: %s must hold one value per point" % (what, name))
        if v.dtype != torch.float32:
            raise ValueError("%s: %s must be float32" % (what, name))
        out.append(v.detach())
    return out


def _step_tail(far_force, far8, f, near8, listed, q, c, alpha_c, alpha_d, coulomb, batch):
    """``(F, U_coulomb, U_sr, W)`` of a step from its parts: the far field's force and eight sums, the pair walk's ``(f, near8)``,
    the list step's ``(lf, list8)`` (``None`` without exclusions), then the self and background terms in float64"""
    if listed is None:
        F = f + far_force
    else:
        F = (f.double() + listed[0].double() + far_force.double()).float()
        near8 = near8 + listed[1]
    eight = far8 + near8  # [B, 8] float64
    q64, c64 = q.double(), c.double()
    total = _set_sums(q64, batch)[0]
    background = (math.pi / (2.0 * alpha_c * alpha_c * coulomb.volume)) * total * total
    U_coulomb = eight[:, 0] - (alpha_c / math.sqrt(math.pi)) * _set_sums(q64 * q64, batch)[0] - background
    U_sr = eight[:, 1] + (alpha_d ** 6 / 12.0) * _set_sums(c64 * c64, batch)[0]
    W = _voigt_to_matrix(eight[:, 2:])
    for e in range(3):
        W[:, e, e] -= background
    return F, U_coulomb.float(), U_sr.float(), W.float()


def nfft_ewald_lj_step(q, c, a, pos, batch=None, /, coulomb=None, dispersion=None, cutoff=4, fractional=False):
    """``(F, U_coulomb, U_lj, W)``: what one molecular-dynamics step needs from the nonbonded part of a Lennard-Jones +
    Coulomb model, in one pass.

    ``q``, ``c``, ``a`` are real float32 ``[n]`` -- charges, dispersion and repulsion coefficients with ``C6_ij = c_i c_j`` and
    ``C12_ij = a_i a_j`` (``lj_coefficients``) -- and any of them may be ``None``, meaning zeros.  A trailing dimension
    (columns) or complex values raise ValueError.  ``pos`` ``[n, 3]``, ``batch``, ``cutoff`` and ``fractional`` are those of
    ``nfft_ewald_step``.  ``coulomb`` is an ``EwaldSplitting`` and ``dispersion`` a ``DispersionSplitting`` (TypeError otherwise)
    with the same ``r_cut``, ``bandwidth`` and ``box`` (ValueError naming the field otherwise); their ``alpha`` may differ.

    The energy of a point set is ``U = U_coulomb + U_lj``.  ``U_coulomb`` is the ``U`` of ``nfft_ewald_virial`` (tin-foil, self
    and background terms).  ``U_lj = 1/2 sum_i a_i rho_i - 1/2 sum_i c_i psi_i`` with ``psi`` the full lattice sum of
    ``nfft_ewald_dispersion`` (self term included) and ``rho_i = sum_{j: 0 < r_ij < r_cut} a_j / r_ij^12`` over minimum images,
    plainly truncated at ``r_cut`` with no shift and no tail correction: the pair term that the truncation drops just beyond
    the cut is ``a_i a_j / r_cut^12``.

    Returns

    * ``F`` ``[n, 3]`` float32, the physical force ``-dU/dx_i = q_i E_i - c_i G_i + a_i H_i``, Cartesian and in the box's units:
      ``E`` and ``G`` are the fields of ``nfft_ewald`` and ``nfft_ewald_dispersion`` and ``H_i = sum_j 12 a_j d_ij / r_ij^14``;
    * ``U_coulomb``, ``U_lj`` ``[B]`` float32;
    * ``W`` ``[B, 3, 3]`` float32, ``W_ab = -dU / d eps_ab`` of the total for the strain ``A -> A (1 + eps)`` at fixed fractional
      coordinates: ``W = W_C - W_D + W_R`` with ``W_C`` of ``nfft_ewald_virial``, ``W_D`` of ``nfft_ewald_dispersion_virial`` and
      ``W_R = 1/2 sum_ij a_i a_j 12 d_a d_b / r^14``, hence ``tr W = U_C - 6 U_D + 12 U_R`` for the converged sums.
      ``virial_to_box_gradient`` applies unchanged.

    One adjoint transform of the two columns ``(q, c)``, one native spectral pass (the six spectra of ``(E, G)`` and the
    frequencies' share of the energies and of ``W`` from one read), one forward transform of the six spectra, one native walk
    over the pairs within ``r_cut`` (eleven sums per point, eight of them reduced in float64), then the self and background
    terms in float64 before the cast -- where ``nfft_ewald_step``, ``nfft_ewald_dispersion(field=True)`` and
    ``nfft_ewald_dispersion_virial`` together do three adjoint transforms and three walks.  The two native steps use no atomics
    and give the same bits on every call; the transforms around them spread with float atomics, so the whole does not.

    Coincident points do not see each other.  The pair walk works in float32: separations below ``1.6e-5``, or so small that
    ``12 a_i a_j / r^14`` exceeds ``3.4e38``, give values that are not numbers.

    Exclusions are not handled here and there is no ``exclusions=`` keyword: ``nfft_ewald_lj_excl_step`` is this call with an
    ``ExclusionList``.  It scales the terms of bonded pairs inside the pair loop, since the subtract-afterwards correction
    that serves ``1/r`` would leave a rounding of ``2^-24 a_i a_j / r^12`` per bonded pair, which at bonded distances is not small.

    Runs under ``torch.no_grad()``: all four outputs are constants to autograd.  Inputs that require grad are accepted and get
    no gradient from here; ``batch`` must not require grad (AssertionError)."""
    return _lj_step("nfft_ewald_lj_step", q, c, a, pos, batch, coulomb, dispersion, None, cutoff, fractional)


def nfft_ewald_lj_excl_step(q, c, a, pos, batch=None, /, coulomb=None, dispersion=None, exclusions=None, cutoff=4, fractional=False):
    """``(F, U_coulomb, U_lj, W)`` of ``nfft_ewald_lj_step`` with bonded-pair exclusions: the same
    inputs, outputs, checks and ``no_grad`` behaviour, and ``exclusions``, an ``ExclusionList`` over the points of ``pos`` or
    ``None`` (TypeError, ValueError as for ``nfft_ewald(exclusions=)``).  With ``None`` it returns exactly what
    ``nfft_ewald_lj_step`` returns, by that code path.

    The Coulomb scale ``s^C`` of a listed pair is the list's ``coulomb_scale``; the Lennard-Jones scale ``s^L`` is its
    ``dispersion_scale`` and applies to BOTH powers, ``r^-6`` and ``r^-12`` (AMBER and OPLS scale the whole 1-4 Lennard-Jones
    term; a force field with separate 1-4 parameters is not covered).  With ``w = 1 - s``, ``d`` the minimum image of
    ``x_i - x_j`` as the pair sweeps form it and ``r = |d|``, each listed pair once, the ONE image that the bond refers to loses::

        U_C  -= w^C q_i q_j / r                F_i -= w^C q_i q_j d / r^3               W -= w^C q_i q_j d d^T / r^3
        U_LJ -= w^L (a_i a_j / r^12 [r < r_cut] - c_i c_j / r^6)
        F_i  -= w^L (12 a_i a_j / r^14 [r < r_cut] - 6 c_i c_j / r^8) d                  (F_j the opposite; W likewise with d d^T)

    and ``tr W = U_C - 6 U_D + 12 U_R`` holds for the corrected converged sums.  A listed pair at ``r = 0`` (a virtual site on
    its atom) takes ``U_C -= w^C q_i q_j 2 alpha_C / sqrt(pi)`` and ``U_LJ += w^L c_i c_j alpha_D^6 / 6``, no force, no virial
    term and no repulsion, which makes the sums continuous in ``r -> 0`` for a fully excluded pair; with ``s > 0`` a coincident
    pair is the caller's error.

    Nothing is subtracted afterwards from a large number: the pair walk looks every passing pair up in the list (a binary
    search of the lane's row, for the pairs whose index falls between the row's ends only) and scales its terms by ``s`` before
    they reach an accumulator -- a fully excluded pair adds nothing at all -- and a second native step over the list removes
    the smooth share of the listed pairs that the far field holds, ``erf(alpha_C r) / r`` and ``1 / r^6`` minus the dispersion
    pair weight, which are bounded by their values at ``r = 0``.  Both steps use no atomics and give the same bits on every
    call; the transforms and the spectral step are those of ``nfft_ewald_lj_step``."""
    return _lj_step("nfft_ewald_lj_excl_step", q, c, a, pos, batch, coulomb, dispersion, exclusions, cutoff, fractional)


MAX_TYPES = 32  # the pair kernel keeps the table in LDS


class LJPairTable:
    """Lennard-Jones parameters per PAIR OF TYPES, for force fields whose ``C6_ij`` and ``C12_ij`` are not products of
    per-point numbers.  Built once per topology, like ``ExclusionList``.

    ``c6`` and ``c12`` are real, symmetric ``[T, T]`` with ``1 <= T <= 32``: the pair energy of types ``t, t'`` is
    ``c12[t, t'] / r^12 - c6[t, t'] / r^6``.  ``types`` is integer ``[n]`` with values in ``[0, T)``, one per point; it is
    checked here, once, which costs a host synchronisation.  ``grid_c`` ``[T]`` is the per-type coefficient that the far field
    carries -- the grid can only hold a rank-one ``c_i c_j`` -- and defaults to ``sqrt(diag(c6))``, which is exact for pairs of
    one type.  ValueError for a table that is not square, not symmetric or not finite, ``T`` outside ``[1, 32]`` (the limit is
    named), a type out of range (the first offender is named), a negative diagonal of ``c6`` without ``grid_c``, or a
    ``grid_c`` that is not ``[T]``.

    NBFIX, or any fitted cross term, is the caller editing single entries of ``c6`` and ``c12`` (both ``[t, t']`` and
    ``[t', t]``) before construction; nothing else is needed.

    Attributes, on the device of ``types`` and derived in float64 before the cast: ``types`` int32 ``[n]``, ``c =
    grid_c[types]`` float32 ``[n]``, ``table`` float32 ``[T, T, 2] = (c12, c6 - outer(grid_c, grid_c))``; ``num_types``,
    ``num_points`` and ``grid_c`` (float64 ``[T]``)."""

    def __init__(self, c6, c12, types, grid_c=None):
        types = torch.as_tensor(types)
        device = types.device
        if types.dim() != 1 or types.dtype.is_floating_point or types.dtype.is_complex or types.dtype == torch.bool:
            raise ValueError("LJPairTable: types must be an integer [n] tensor")
        c6, c12 = torch.as_tensor(c6).detach(), torch.as_tensor(c12).detach()
        if c6.is_complex() or c12.is_complex():
            raise ValueError("LJPairTable: c6 and c12 must be real")
        if c6.dim() != 2 or c6.size(0) != c6.size(1) or c12.shape != c6.shape:
            raise ValueError("LJPairTable: c6 and c12 must be [T, T], both")
        T = c6.size(0)
        if T < 1 or T > MAX_TYPES:
            raise ValueError("LJPairTable: %d types, the limit is %d (the pair kernel keeps the table in LDS)" % (T, MAX_TYPES))
        c6, c12 = c6.to(device=device, dtype=torch.float64), c12.to(device=device, dtype=torch.float64)
        if not bool(torch.isfinite(c6).all()) or not bool(torch.isfinite(c12).all()):
            raise ValueError("LJPairTable: c6 and c12 must be finite")
        if not torch.equal(c6, c6.t()) or not torch.equal(c12, c12.t()):
            raise ValueError("LJPairTable: c6 and c12 must be symmetric")
        bad = ((types < 0) | (types >= T)).nonzero()
        if bad.numel():
            i = int(bad[0, 0])
            raise ValueError("LJPairTable: types[%d] = %d lies outside [0, %d)" % (i, int(types[i]), T))
        if grid_c is None:
            diag = torch.diagonal(c6)
            if bool((diag < 0).any()):
                raise ValueError("LJPairTable: c6 has a negative diagonal entry, grid_c = sqrt(diag(c6)) does not exist")
            grid_c = torch.sqrt(diag)
        else:
            grid_c = torch.as_tensor(grid_c).detach()
            if grid_c.is_complex() or grid_c.shape != (T,):
                raise ValueError("LJPairTable: grid_c must be real [T]")
            grid_c = grid_c.to(device=device, dtype=torch.float64)
            if not bool(torch.isfinite(grid_c).all()):
                raise ValueError("LJPairTable: grid_c must be finite")
        self.num_types, self.num_points = T, types.size(0)
        self.grid_c = grid_c
        self.types = types.detach().to(torch.int32).contiguous()
        self.c = grid_c[types.long()].float().contiguous()
        self.table = torch.stack([c12, c6 - torch.outer(grid_c, grid_c)], 2).float().contiguous()

    @classmethod
    def lorentz_berthelot(cls, sigma, epsilon, types):
        """``sigma``, ``epsilon`` ``[T]`` per type: ``sigma_ij = (sigma_i + sigma_j) / 2``, ``eps_ij = sqrt(eps_i eps_j)``,
        ``c6 = 4 eps_ij sigma_ij^6``, ``c12 = 4 eps_ij sigma_ij^12`` and, on the grid, the geometric approximation ``grid_c =
        2 sqrt(eps) sigma^3`` (what GROMACS's ``ljpme-comb-rule = LB`` puts there): beyond ``r_cut`` unlike pairs attract with
        ``4 eps_ij (sigma_i sigma_j)^3`` in place of ``4 eps_ij sigma_ij^6``."""
        sigma, epsilon = _per_type(sigma, epsilon)
        s = 0.5 * (sigma.unsqueeze(0) + sigma.unsqueeze(1))
        return cls._mixed(s, sigma, epsilon, types)

    @classmethod
    def geometric(cls, sigma, epsilon, types):
        """The OPLS rule, ``sigma_ij = sqrt(sigma_i sigma_j)`` and ``eps_ij = sqrt(eps_i eps_j)``, for which the grid's product
        is the pair's ``c6`` (``table[..., 1]`` is zero up to rounding): the model of ``nfft_ewald_lj_step`` with
        ``lj_coefficients``."""
        sigma, epsilon = _per_type(sigma, epsilon)
        s = torch.sqrt(sigma.unsqueeze(0) * sigma.unsqueeze(1))
        return cls._mixed(s, sigma, epsilon, types)

    @classmethod
    def _mixed(cls, s, sigma, epsilon, types):
        e4 = 4.0 * torch.sqrt(epsilon.unsqueeze(0) * epsilon.unsqueeze(1))
        s6 = s ** 6
        c6, c12 = e4 * s6, e4 * s6 * s6
        c6, c12 = 0.5 * (c6 + c6.t()), 0.5 * (c12 + c12.t())  # (symmetric to the last bit)
        return cls(c6, c12, types, grid_c=2.0 * torch.sqrt(epsilon) * sigma ** 3)

    def __repr__(self):
        return "LJPairTable(%d types over %d points, device=%s)" % (self.num_types, self.num_points, self.types.device)


def _per_type(sigma, epsilon):
    sigma = torch.as_tensor(sigma).detach().to(torch.float64)
    epsilon = torch.as_tensor(epsilon).detach().to(torch.float64)
    if sigma.dim() != 1 or epsilon.shape != sigma.shape:
        raise ValueError("LJPairTable: sigma and epsilon must be [T], both")
    if bool((epsilon < 0).any()):
        raise ValueError("LJPairTable: epsilon must not be negative")
    return sigma.cpu(), epsilon.cpu()


def nfft_ewald_lj_table_step(q, table, pos, batch=None, /, coulomb=None, dispersion=None, exclusions=None, cutoff=4,
                             fractional=False):
    """``(F, U_coulomb, U_lj, W)`` of ``nfft_ewald_lj_excl_step`` for a force field with per-type-pair parameters -- Lorentz-
    Berthelot mixing, NBFIX -- given as an ``LJPairTable``.  ``q``, ``pos``, ``batch``, the two
    splittings, ``exclusions`` (an ``ExclusionList`` or ``None``), ``cutoff``, ``fractional``, the shapes and dtypes of the
    outputs, the checks and the ``no_grad`` behaviour are those of ``nfft_ewald_lj_excl_step``; ``table`` must be an
    ``LJPairTable`` (TypeError) over ``pos.size(0)`` points on the device of ``pos`` (ValueError).

    With ``t_i`` the type of point ``i``, ``c_i = grid_c[t_i]``, ``dC6 = C6 - c_i c_j`` from the table, ``d`` the minimum image
    of ``x_i - x_j`` and ``r = |d|``::

        U_lj = 1/2 sum_{i != j, 0 < r < r_cut} [C12(t_i, t_j) / r^12 - dC6(t_i, t_j) / r^6]  -  1/2 sum_i c_i psi_i
        F_i  = q_i E_i - c_i G_i + sum_j [12 C12 / r^14 - 6 dC6 / r^8] d
        W    = W_C - W_D(c) + 1/2 sum_ij [12 C12 / r^14 - 6 dC6 / r^8] d d^T

    with ``psi``, ``G`` and ``W_D`` the full lattice sums of ``nfft_ewald_dispersion`` on ``c``.  Inside ``r_cut`` a pair
    interacts with its exact ``C6_ij``; beyond it, with ``c_i c_j``: the grid keeps a rank-one coefficient, as LJ-PME with
    Lorentz-Berthelot mixing does in GROMACS and LAMMPS.  Both truncations are plain, no shift and no tail correction: the
    pair energy jumps by ``dC6_ij / r_cut^6 - C12_ij / r_cut^12`` at the cut.  ``tr W = U_C - 6 U_D + 12 U_R - 6 U_delta`` with
    ``U_delta = 1/2 sum dC6 / r^6`` over the same pairs, which enters ``U_lj`` with a minus sign as ``U_D`` does.

    With ``exclusions`` the Lennard-Jones scale ``s^L`` of a listed pair multiplies ``C12``, ``dC6`` and ``c_i c_j`` alike and
    ``s^C`` its ``q_i q_j``, inside the pair loop; the conventions at ``r = 0`` and ``r >= r_cut`` are those of
    ``nfft_ewald_lj_excl_step`` (beyond the cut only ``c_i c_j / r^6`` exists to remove).  A force field with separate 1-4
    parameters is not covered.

    The transforms, the spectral step, the list step and the self and background terms are those of
    ``nfft_ewald_lj_excl_step`` on ``(q, c, 0)``; the pair walk is one native step of its own that looks ``(C12, dC6)`` up in a
    copy of the table in LDS (no atomics: the same bits on every call).  It works in float32: separations below ``1.6e-5``, or
    so small that ``12 C12 / r^14`` or ``6 dC6 / r^8`` exceeds ``3.4e38``, give values that are not numbers.  A value of
    ``table.types`` changed on the device after construction to one outside ``[0, T)`` is clamped, never followed."""
    what = "nfft_ewald_lj_table_step"
    _check_splittings(what, coulomb, dispersion)
    if not isinstance(table, LJPairTable):
        raise TypeError("%s: table must be an LJPairTable" % what)
    if pos.dim() != 2 or pos.size(1) != 3:
        raise ValueError("%s: the periodic sums are three-dimensional, pos must be [n, 3]" % what)
    if table.num_points != pos.size(0):
        raise ValueError("%s: table holds the types of %d points, pos has %d" % (what, table.num_points, pos.size(0)))
    if table.types.device != pos.device:
        raise ValueError("%s: table lives on %s, pos on %s" % (what, table.types.device, pos.device))
    if batch is not None and batch.requires_grad:
        raise AssertionError("%s: batch holds point-set indices and must not require grad" % what)
    q, = _check_values(what, (q,), pos)
    ex = check_exclusions(what, exclusions, pos)
    with torch.no_grad():
        pos = _fractional(what, pos.detach(), coulomb, fractional)
        c = table.c
        alpha_c, alpha_d, N = coulomb.alpha, dispersion.alpha, coulomb.bandwidth
        box6 = _IDENTITY6 if coulomb.box is None else coulomb.box6
        band = nfft_adjoint(torch.stack([q, c], 1), pos, batch, bandwidth=N, cutoff=int(cutoff))  # [B, N, N, N, 2]
        spectra, far8 = ops.nfft_ewald_lj_step_spectral(band, coulomb.coeffs, dispersion.coeffs, dispersion.strain_coeffs(), box6,
                                                        alpha_c)
        far = nfft_forward(spectra, pos, batch, cutoff=int(cutoff), real_output=True)  # [n, 6]: E, then G
        far_force = q.unsqueeze(1) * far[:, :3] - c.unsqueeze(1) * far[:, 3:]
        xs = torch.stack([q, c], 1)
        walk = (box6, alpha_c, alpha_d, coulomb.r_cut)
        lists, listed = (None, None, None, None), None
        if ex is not None:
            # the listed pairs come scaled out of the walk; the list step of 7s takes the smooth share of q_i q_j and c_i c_j
            # back out of the far field, which holds nothing of C12 and dC6
            lists = (ex.row_start, ex.col, ex.coulomb_weight, ex.dispersion_weight)
            listed = ops.nfft_ewald_lj_excl_list(pos, torch.stack([q, c, torch.zeros_like(q)], 1), batch, *lists, *walk)
        f, near8 = ops.nfft_ewald_lj_table_near(pos, xs, table.types, table.table, batch, *lists, *walk)
        return _step_tail(far_force, far8, f, near8, listed, q, c, alpha_c, alpha_d, coulomb, batch)


def _lj_step(what, q, c, a, pos, batch, coulomb, dispersion, exclusions, cutoff, fractional):
    """the body of both calls; exclusions=None is nfft_ewald_lj_step"""
    _check_splittings(what, coulomb, dispersion)
    if pos.dim() != 2 or pos.size(1) != 3:
        raise ValueError("%s: the periodic sums are three-dimensional, pos must be [n, 3]" % what)
    if batch is not None and batch.requires_grad:
        raise AssertionError("%s: batch holds point-set indices and must not require grad" % what)
    q, c, a = _check_values(what, (q, c, a), pos)
    ex = check_exclusions(what, exclusions, pos)
    with torch.no_grad():
        pos = _fractional(what, pos.detach(), coulomb, fractional)
        alpha_c, alpha_d, N = coulomb.alpha, dispersion.alpha, coulomb.bandwidth
        box6 = _IDENTITY6 if coulomb.box is None else coulomb.box6
        band = nfft_adjoint(torch.stack([q, c], 1), pos, batch, bandwidth=N, cutoff=int(cutoff))  # [B, N, N, N, 2]
        spectra, far8 = ops.nfft_ewald_lj_step_spectral(band, coulomb.coeffs, dispersion.coeffs, dispersion.strain_coeffs(), box6,
                                                        alpha_c)
        far = nfft_forward(spectra, pos, batch, cutoff=int(cutoff), real_output=True)  # [n, 6]: E, then G
        far_force = q.unsqueeze(1) * far[:, :3] - c.unsqueeze(1) * far[:, 3:]
        xs = torch.stack([q, c, a], 1)
        walk = (box6, alpha_c, alpha_d, coulomb.r_cut)
        if ex is None:
            f, near8 = ops.nfft_ewald_lj_step_near(pos, xs, batch, *walk)
            listed = None
        else:
            # the listed pairs come scaled out of the walk; the list step takes their smooth share back out of the far field
            lists = (ex.row_start, ex.col, ex.coulomb_weight, ex.dispersion_weight)
            f, near8 = ops.nfft_ewald_lj_excl_near(pos, xs, batch, *lists, *walk)
            listed = ops.nfft_ewald_lj_excl_list(pos, xs, batch, *lists, *walk)
        return _step_tail(far_force, far8, f, near8, listed, q, c, alpha_c, alpha_d, coulomb, batch)
