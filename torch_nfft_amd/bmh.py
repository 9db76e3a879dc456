"""Nonbonded step of a Buckingham or Born-Mayer-Huggins + Coulomb model in a periodic box: forces, energies and the virial
tensor from one pass (no reference counterpart).

The ionic force fields -- Tosi-Fumi for the alkali halides and their melts, BKS for silica, the Buckingham tables of MgO, UO2
and most ceramics -- repel with an exponential where Lennard-Jones has ``C12 / r^12``.  The pair energy of types ``t, t'`` is::

    u(r) = A e^(-B r) - C6 / r^6 - C8 / r^8          A >= 0, B = 1 / rho >= 0; attractions enter with POSITIVE C6 and C8

given per pair of types in a ``BMHPairTable``.  ``nfft_ewald_bmh_table_step`` is ``nfft_ewald_lj_table_step`` (section 7t) with
this pair energy inside ``r_cut``: the Coulomb Ewald sum, optionally LJ-PME for ``r^-6`` with a per-type grid coefficient,
exclusion lists, and one native pair walk.  With ``dispersion=None`` nothing of ``r^-6`` goes on the grid -- what BKS, Tosi-Fumi
as published and LAMMPS' ``buck/coul/long`` and ``born/coul/long`` do.

The exponential is finite at ``r = 0`` and the attractions are not: below the maximum of ``u`` (the Buckingham turnover, well
inside the first neighbour shell for published tables) the model attracts without bound.  Nothing here guards that inner
wall; a configuration that crosses it is the caller's to prevent.
"""
import torch

from . import ops
from .dispersion import DispersionSplitting
from .exclusions import check_exclusions
from .ewald import EwaldSplitting, _IDENTITY6, _fractional
from .lj import MAX_TYPES, _check_splittings, _check_values, _step_tail
from .nfft import nfft_adjoint, nfft_forward

_FLOAT32_MAX = 3.4028234663852886e38


class BMHPairTable:
    """Buckingham / Born-Mayer-Huggins parameters per PAIR OF TYPES.  Built once per topology, like
    ``LJPairTable`` and ``ExclusionList``.

    ``A``, ``B``, ``c6`` and ``c8`` are real, symmetric ``[T, T]`` with ``1 <= T <= 32``: the pair energy of types ``t, t'`` is
    ``A e^(-B r) - c6 / r^6 - c8 / r^8`` with ``B = 1 / rho``; an attraction has a positive ``c6`` or ``c8``.  ``types`` is integer
    ``[n]`` with values in ``[0, T)``, one per point; it is checked here, once, which costs a host synchronisation.  ``grid_c``
    ``[T]`` is the per-type coefficient that the far field carries for ``r^-6`` and defaults to ``sqrt(diag(c6))``; force fields
    that truncate the dispersion pass ``grid_c = zeros(T)`` and call the step with ``dispersion=None``.  ValueError for a table
    that is not square, not symmetric or not finite, ``T`` outside ``[1, 32]`` (the limit is named), a negative entry of ``A`` or
    ``B`` (the entry is named), a type out of range (the first offender is named), a negative diagonal of ``c6`` without
    ``grid_c``, or a ``grid_c`` that is not ``[T]``.

    Attributes, on the device of ``types`` and derived in float64 before the cast: ``types`` int32 ``[n]``, ``c =
    grid_c[types]`` float32 ``[n]``, ``table`` float32 ``[T, T, 4] = (A, B, c6 - outer(grid_c, grid_c), c8)``; ``num_types``,
    ``num_points``, ``grid_c`` (float64 ``[T]``) and ``has_grid``, a Python bool decided here: whether any ``grid_c`` is
    non-zero."""

    def __init__(self, A, B, c6, c8, types, grid_c=None):
        types = torch.as_tensor(types)
        device = types.device
        if types.dim() != 1 or types.dtype.is_floating_point or types.dtype.is_complex or types.dtype == torch.bool:
            raise ValueError("BMHPairTable: types must be an integer [n] tensor")
        tabs = [torch.as_tensor(v).detach() for v in (A, B, c6, c8)]
        if any(v.is_complex() for v in tabs):
            raise ValueError("BMHPairTable: A, B, c6 and c8 must be real")
        if tabs[0].dim() != 2 or tabs[0].size(0) != tabs[0].size(1) or any(v.shape != tabs[0].shape for v in tabs):
            raise ValueError("BMHPairTable: A, B, c6 and c8 must be [T, T], all four")
        T = tabs[0].size(0)
        if T < 1 or T > MAX_TYPES:
            raise ValueError("BMHPairTable: %d types, the limit is %d (the pair kernel keeps the table in LDS)" % (T, MAX_TYPES))
        tabs = [v.to(device=device, dtype=torch.float64) for v in tabs]
        if not all(bool(torch.isfinite(v).all()) for v in tabs):
            raise ValueError("BMHPairTable: A, B, c6 and c8 must be finite")
        if not all(torch.equal(v, v.t()) for v in tabs):
            raise ValueError("BMHPairTable: A, B, c6 and c8 must be symmetric")
        for name, v in zip("AB", tabs):
            neg = (v < 0).nonzero()
            if neg.numel():
                i, j = int(neg[0, 0]), int(neg[0, 1])
                raise ValueError("BMHPairTable: %s[%d, %d] = %g is negative" % (name, i, j, float(v[i, j])))
        A, B, c6, c8 = tabs
        bad = ((types < 0) | (types >= T)).nonzero()
        if bad.numel():
            i = int(bad[0, 0])
            raise ValueError("BMHPairTable: types[%d] = %d lies outside [0, %d)" % (i, int(types[i]), T))
        if grid_c is None:
            diag = torch.diagonal(c6)
            if bool((diag < 0).any()):
                raise ValueError("BMHPairTable: c6 has a negative diagonal entry, grid_c = sqrt(diag(c6)) does not exist")
            grid_c = torch.sqrt(diag)
        else:
            grid_c = torch.as_tensor(grid_c).detach()
            if grid_c.is_complex() or grid_c.shape != (T,):
                raise ValueError("BMHPairTable: grid_c must be real [T]")
            grid_c = grid_c.to(device=device, dtype=torch.float64)
            if not bool(torch.isfinite(grid_c).all()):
                raise ValueError("BMHPairTable: grid_c must be finite")
        self.num_types, self.num_points = T, types.size(0)
        self.grid_c = grid_c
        self.has_grid = bool((grid_c != 0).any())
        self.types = types.detach().to(torch.int32).contiguous()
        self.c = grid_c[types.long()].float().contiguous()
        self.table = torch.stack([A, B, c6 - torch.outer(grid_c, grid_c), c8], 2).float().contiguous()

    @classmethod
    def buckingham(cls, A, rho, C, types, grid_c=None):
        """``A e^(-r / rho) - C / r^6`` per pair of types, the parameters of LAMMPS' ``pair_style buck``: ``A``, ``rho`` and ``C``
        ``[T, T]``, ``rho > 0``.  BKS and most oxide tables truncate ``C / r^6``: pass ``grid_c = torch.zeros(T)`` and call the step
        with ``dispersion=None``."""
        A, rho, C = (_pair_table(v) for v in (A, rho, C))
        _check_rho(rho)
        return cls(A, 1.0 / rho, C, torch.zeros_like(C), types, grid_c=grid_c)

    @classmethod
    def born(cls, A, rho, sigma, C, D, types, grid_c=None):
        """``A e^((sigma - r) / rho) - C / r^6 + D / r^8`` per pair of types, the parameters of LAMMPS' ``pair_style born``, all
        ``[T, T]``, ``rho > 0``.  The prefactor ``A e^(sigma / rho)`` is formed in float64 and refused if it leaves float32
        (ValueError naming the entry); ``c8 = -D``.  LAMMPS writes ``+ D / r^8``, so that the Tosi-Fumi tables, whose
        dipole-quadrupole term ``- D / r^8`` is an attraction with a positive published ``D``, are entered there with ``D``
        NEGATED; the same negated value goes in here and comes out as the positive ``c8`` of this class."""
        A, rho, sigma, C, D = (_pair_table(v) for v in (A, rho, sigma, C, D))
        _check_rho(rho)
        pre = A * torch.exp(sigma / rho)
        big = (~torch.isfinite(pre) | (pre.abs() > _FLOAT32_MAX)).nonzero()
        if big.numel():
            i, j = int(big[0, 0]), int(big[0, 1])
            raise ValueError("BMHPairTable: A e^(sigma / rho) at [%d, %d] leaves float32" % (i, j))
        return cls(pre, 1.0 / rho, C, -D, types, grid_c=grid_c)

    def __repr__(self):
        return "BMHPairTable(%d types over %d points, device=%s)" % (self.num_types, self.num_points, self.types.device)


def _pair_table(v):
    return torch.as_tensor(v).detach().to(torch.float64).cpu()


def _check_rho(rho):
    if not bool((rho > 0).all()):
        raise ValueError("BMHPairTable: rho must be positive")


def nfft_ewald_bmh_table_step(q, table, pos, batch=None, /, coulomb=None, dispersion=None, exclusions=None, cutoff=4,
                              fractional=False):
    """``(F, U_coulomb, U_sr, W)`` of ``nfft_ewald_lj_table_step`` for a Buckingham or Born-Mayer-Huggins force field given as a
    ``BMHPairTable``.  ``q``, ``pos``, ``batch``, ``coulomb``, ``exclusions`` (an ``ExclusionList`` or
    ``None``), ``cutoff``, ``fractional``, the shapes and dtypes of the outputs, the checks and the ``no_grad`` behaviour are
    those of ``nfft_ewald_lj_table_step``; ``table`` must be a ``BMHPairTable`` (TypeError) over ``pos.size(0)`` points on the
    device of ``pos`` (ValueError).  ``dispersion`` is a ``DispersionSplitting`` with the ``r_cut``, ``bandwidth`` and ``box`` of
    ``coulomb``, or ``None``.

    With ``t_i`` the type of point ``i``, ``c_i = grid_c[t_i]``, ``dC6 = C6 - c_i c_j`` from the table, ``d`` the minimum image
    of ``x_i - x_j`` and ``r = |d|``::

        U_sr = 1/2 sum_{i != j, 0 < r < r_cut} [A e^(-B r) - dC6 / r^6 - C8 / r^8]  -  1/2 sum_i c_i psi_i
        F_i  = q_i E_i - c_i G_i + sum_j [A B e^(-B r) / r - 6 dC6 / r^8 - 8 C8 / r^10] d
        W    = W_C - W_D(c) + 1/2 sum_ij [the same bracket] d d^T

    with ``psi``, ``G`` and ``W_D`` the full lattice sums of ``nfft_ewald_dispersion`` on ``c``.  The exponential, the ``dC6``
    term and the ``C8`` term are plainly truncated at ``r_cut``, no shift and no tail correction (as LAMMPS'
    ``born/coul/long``): the pair energy jumps by ``dC6 / r_cut^6 + C8 / r_cut^8 - A e^(-B r_cut)`` at the cut.  The exponential is
    not homogeneous in the lengths, so ``tr W = U_C - 6 U_D - 6 U_delta - 8 U_8 + 1/2 sum A B r e^(-B r)`` with ``U_delta = 1/2 sum
    dC6 / r^6`` and ``U_8 = 1/2 sum C8 / r^8`` over the same pairs.

    ``dispersion=None`` puts nothing of ``r^-6`` on the grid: it needs a table whose ``grid_c`` is all zero (``table.has_grid``
    false; ValueError naming ``grid_c`` otherwise).  The far field is then the Coulomb one alone -- one adjoint transform of one
    column, the spectral pass of ``nfft_ewald_step``, one forward transform of four columns -- and the same pair walk runs
    with ``c = 0``, whose terms are exact zeros; the whole ``C6 / r^6`` is truncated at ``r_cut``.

    With ``exclusions`` the scale ``s^L`` of a listed pair multiplies ``A``, ``dC6``, ``C8`` and ``c_i c_j`` alike and ``s^C`` its
    ``q_i q_j``, inside the pair loop; the conventions at ``r = 0`` and ``r >= r_cut`` are those of ``nfft_ewald_lj_excl_step``.
    A force field with separate 1-4 parameters is not covered.

    The transforms, the spectral step, the list step and the self and background terms are those of
    ``nfft_ewald_lj_table_step`` on ``(q, c, 0)``; the pair walk is one native step of its own that reads ``(A, B)`` and
    ``(dC6, C8)`` from two copies of the table's halves in LDS (no atomics: the same bits on every call).  It works in float32:
    separations below ``1.6e-5``, or so small that ``6 dC6 / r^8`` or ``8 C8 / r^10`` exceeds ``3.4e38``, give values that are not
    numbers.  Long before that, inside the maximum of the pair energy (the Buckingham turnover), the model itself attracts
    without bound, and nothing here guards it.  A value of ``table.types`` changed on the device after construction to one
    outside ``[0, T)`` is clamped, never followed."""
    what = "nfft_ewald_bmh_table_step"
    if dispersion is None:
        if not isinstance(coulomb, EwaldSplitting):
            raise TypeError("%s: coulomb must be an EwaldSplitting" % what)
    else:
        _check_splittings(what, coulomb, dispersion)
    if not isinstance(table, BMHPairTable):
        raise TypeError("%s: table must be a BMHPairTable" % what)
    if dispersion is None and table.has_grid:
        raise ValueError("%s: dispersion=None needs a table with grid_c = 0 (this one carries r^-6 on the grid); build it with "
                         "grid_c=torch.zeros(T) or pass a DispersionSplitting" % what)
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
        alpha_c, N = coulomb.alpha, coulomb.bandwidth
        box6 = _IDENTITY6 if coulomb.box is None else coulomb.box6
        if dispersion is None:
            # the Coulomb far field alone: the walk's dispersion weights stay finite with alpha_C and meet c = 0
            c = torch.zeros_like(q)
            alpha_d = alpha_c
            band = nfft_adjoint(q, pos, batch, bandwidth=N, cutoff=int(cutoff))  # [B, N, N, N]
            spectra, far7 = ops.nfft_ewald_step_spectral(band, coulomb.coeffs, box6, alpha_c)
            far = nfft_forward(spectra, pos, batch, cutoff=int(cutoff), real_output=True)  # [n, 4]: phi, then E
            far_force = q.unsqueeze(1) * far[:, 1:]
            far8 = torch.cat([far7[:, :1], torch.zeros_like(far7[:, :1]), far7[:, 1:]], 1)
        else:
            c = table.c
            alpha_d = dispersion.alpha
            band = nfft_adjoint(torch.stack([q, c], 1), pos, batch, bandwidth=N, cutoff=int(cutoff))  # [B, N, N, N, 2]
            spectra, far8 = ops.nfft_ewald_lj_step_spectral(band, coulomb.coeffs, dispersion.coeffs, dispersion.strain_coeffs(),
                                                            box6, alpha_c)
            far = nfft_forward(spectra, pos, batch, cutoff=int(cutoff), real_output=True)  # [n, 6]: E, then G
            far_force = q.unsqueeze(1) * far[:, :3] - c.unsqueeze(1) * far[:, 3:]
        xs = torch.stack([q, c], 1)
        walk = (box6, alpha_c, alpha_d, coulomb.r_cut)
        lists, listed = (None, None, None, None), None
        if ex is not None:
            # the listed pairs come scaled out of the walk; the list step of 7s takes the smooth share of q_i q_j and c_i c_j
            # back out of the far field, which holds nothing of A, dC6 and C8
            lists = (ex.row_start, ex.col, ex.coulomb_weight, ex.dispersion_weight)
            listed = ops.nfft_ewald_lj_excl_list(pos, torch.stack([q, c, torch.zeros_like(q)], 1), batch, *lists, *walk)
        f, near8 = ops.nfft_ewald_bmh_table_near(pos, xs, table.types, table.table, batch, *lists, *walk)
        return _step_tail(far_force, far8, f, near8, listed, q, c, alpha_c, alpha_d, coulomb, batch)
