"""Bonded-pair exclusions for the Coulomb and the dispersion Ewald sums (no reference counterpart).

A force field takes the direct interaction of bonded neighbours (1-2, 1-3) out of the non-bonded sums and scales that of
1-4 neighbours.  An ``ExclusionList`` names unordered pairs ``{i, j}`` of one point set with two scale factors in
``[0, 1]``, ``s^C`` for Coulomb and ``s^D`` for dispersion (0: fully excluded); with ``w = 1 - s``, ``d_ij`` the minimum image
of ``x_i - x_j`` as the pair sweeps form it and ``r = |d_ij|`` the sums of ``nfft_ewald`` and ``nfft_ewald_dispersion`` become::

    phi_i <- phi_i - sum_{j in ex(i)} w^C_ij q_j / r           E_i <- E_i - sum w^C_ij q_j d_ij / r^3
    psi_i <- psi_i - sum_{j in ex(i)} w^D_ij c_j / r^6         G_i <- G_i - 6 sum w^D_ij c_j d_ij / r^8

Only the ONE image that the bond refers to is removed; all other images of ``j`` keep interacting with ``i``.  A listed pair
at ``r = 0`` (a Drude particle or a virtual site on its atom) was never in the pair sweep, but the far field has added the
limit of its smooth part: the correction there is ``-w^C q_j 2 alpha / sqrt(pi)`` and ``-w^D c_j alpha^6 / 6``, no field, which
makes the corrected sum continuous in ``r -> 0``.  The virials lose, per listed pair, ``w q_i q_j / r`` and
``w q_i q_j d_a d_b / r^3`` (``tr W = U`` stays) and ``w c_i c_j / r^6`` and ``6 w c_i c_j d_a d_b / r^8`` (``tr W = 6 U`` stays);
the ``r = 0`` constants enter ``U`` only.

What remains: the pair sweep does not skip listed pairs, so its float32 accumulator has held ``|q_j| / r`` (``|c_j| / r^6``)
before the correction takes it out again.  An excluded pair at the separation ``r`` leaves a rounding of about
``2^-24 |q_j| / r`` in ``phi_i``, and likewise in ``psi_i``, ``E_i`` and ``G_i``.  Measured on an MI355X:
bonds of 0.02 .. 0.05 box lengths cost 8e-8 .. 9.5e-8 of ``|phi|`` and 2.5e-8 of ``|psi|`` over a whole list, 1e-4 of ``psi_i`` at
the end of a 0.02 bond; a pair at ``r = 1e-6`` costs 7e-2 absolute per unit charge (``2^-24 / r = 6e-2``).
"""
import torch

from . import ops

COULOMB, DISPERSION = 0, 1  # `kind` of the native calls


def _scale(what, s, m):
    """a scale (scalar or ``[m]``) as the float64 ``[m]`` weights ``1 - s``; ValueError unless finite and in ``[0, 1]``"""
    s = torch.as_tensor(s, dtype=torch.float64).detach().cpu()
    if s.dim() == 0:
        s = s.expand(m)
    if s.shape != (m,):
        raise ValueError("ExclusionList: %s must be a scalar or have one entry per pair" % what)
    if not bool(torch.isfinite(s).all()) or bool(((s < 0.0) | (s > 1.0)).any()):
        raise ValueError("ExclusionList: %s must be finite and lie in [0, 1]" % what)
    return 1.0 - s


class ExclusionList:
    """The listed pairs of one topology, built once on the host: symmetrised and sorted by ``(i, j)`` into a CSR matrix.

    ``pairs`` is ``[m, 2]`` integer (``m = 0`` is legal), ``num_points`` the number ``n`` of points it indexes,
    ``coulomb_scale`` and ``dispersion_scale`` scalars or ``[m]`` in ``[0, 1]`` (AMBER 1-4: ``1 / 1.2`` and ``1 / 2``; OPLS:
    ``1 / 2`` both; 0, the default: fully excluded).  ``batch`` is the sorted point-set vector of the points, if there is
    one: both ends of a pair must lie in one point set.  ValueError for ``i == j``, an index outside ``[0, n)``, a pair
    listed twice in either order, a scale that is not finite or outside ``[0, 1]``, or a pair across two point sets.

    Attributes, on ``device``: ``row_start`` ``[n + 1]`` int32, ``col`` ``[2 m]`` int32 (row ``i`` holds the partners of ``i`` in
    ascending order), ``coulomb_weight`` and ``dispersion_weight`` ``[2 m]`` float32 holding ``1 - s``; ``num_points``,
    ``num_pairs``.  ``device="cpu"`` builds a list that can be inspected without a GPU; ``to(device)`` moves one."""

    def __init__(self, pairs, num_points, coulomb_scale=0.0, dispersion_scale=0.0, batch=None, device="cuda"):
        n = int(num_points)
        if n != num_points or n < 0 or n >= 2 ** 31:
            raise ValueError("ExclusionList: num_points must be an integer in [0, 2^31)")
        pairs = torch.as_tensor(pairs).detach().cpu()
        if pairs.numel() == 0:
            pairs = pairs.reshape(0, 2).to(torch.int64)
        if pairs.dim() != 2 or pairs.size(1) != 2 or pairs.dtype.is_floating_point or pairs.dtype.is_complex or pairs.dtype == torch.bool:
            raise ValueError("ExclusionList: pairs must be an integer [m, 2] tensor")
        pairs = pairs.to(torch.int64)
        m = pairs.size(0)
        if 2 * m >= 2 ** 31:
            raise ValueError("ExclusionList: too many pairs")
        wc, wd = _scale("coulomb_scale", coulomb_scale, m), _scale("dispersion_scale", dispersion_scale, m)
        i, j = pairs[:, 0], pairs[:, 1]
        if bool(((pairs < 0) | (pairs >= n)).any()):
            raise ValueError("ExclusionList: a pair has an index outside [0, num_points)")
        if bool((i == j).any()):
            raise ValueError("ExclusionList: a pair must have two different points (i == j)")
        lo, hi = torch.minimum(i, j), torch.maximum(i, j)
        if torch.unique(lo * n + hi).numel() != m:
            raise ValueError("ExclusionList: a pair is listed twice")
        if batch is not None:
            b = torch.as_tensor(batch).detach().cpu()
            if b.shape != (n,):
                raise ValueError("ExclusionList: batch must have one entry per point")
            if bool((b[i] != b[j]).any()):
                raise ValueError("ExclusionList: the two ends of a pair lie in different point sets")
        rows, cols = torch.cat([i, j]), torch.cat([j, i])
        order = torch.argsort(rows * n + cols)
        counts = torch.bincount(rows, minlength=n) if m else torch.zeros(n, dtype=torch.int64)
        row_start = torch.zeros(n + 1, dtype=torch.int64)
        row_start[1:] = torch.cumsum(counts, 0)
        self.num_points, self.num_pairs = n, m
        self._set(row_start.to(torch.int32), cols[order].to(torch.int32), torch.cat([wc, wc])[order].to(torch.float32),
                  torch.cat([wd, wd])[order].to(torch.float32), torch.device(device))

    def _set(self, row_start, col, wc, wd, device):
        self.device = device
        self.row_start = row_start.to(device).contiguous()
        self.col = col.to(device).contiguous()
        self.coulomb_weight = wc.to(device).contiguous()
        self.dispersion_weight = wd.to(device).contiguous()

    def to(self, device):
        """the same list on ``device`` (itself if it is there already)"""
        device = torch.device(device)
        if device == self.row_start.device:
            return self
        other = object.__new__(ExclusionList)
        other.num_points, other.num_pairs = self.num_points, self.num_pairs
        other._set(self.row_start, self.col, self.coulomb_weight, self.dispersion_weight, device)
        return other

    def weight(self, kind):
        return self.coulomb_weight if kind == COULOMB else self.dispersion_weight

    def __len__(self):
        return self.num_pairs

    def __repr__(self):
        return "ExclusionList(%d pairs over %d points, device=%s)" % (self.num_pairs, self.num_points, self.row_start.device)


def check_exclusions(what, exclusions, pos):
    """the keyword ``exclusions`` of the Ewald functions: ``None`` or an ``ExclusionList`` over ``pos.size(0)`` points
    (TypeError, ValueError), on the device of ``pos``"""
    if exclusions is None:
        return None
    if not isinstance(exclusions, ExclusionList):
        raise TypeError("%s: exclusions must be an ExclusionList or None" % what)
    if exclusions.num_points != pos.size(0):
        raise ValueError("%s: exclusions lists pairs of %d points, pos has %d" % (what, exclusions.num_points, pos.size(0)))
    return exclusions.to(pos.device)


def correction(kind, x, pos, batch, splitting, exclusions, field):
    """``(z, f or None)`` of ``ops.nfft_ewald_excl`` for the sum ``kind`` with the splitting's ``alpha`` and box: what to
    SUBTRACT from the potential and the field (``pos`` fractional with a box, as the Functions hold it)"""
    box = () if splitting.box is None else splitting.box6
    z, f = ops.nfft_ewald_excl(pos, x, batch, exclusions.row_start, exclusions.col, exclusions.weight(kind), box,
                               splitting.alpha, kind, field)
    return z, (f if field else None)


def virial_correction(kind, x, pos, batch, splitting, exclusions):
    """``[B, 7, *cols]`` float64 of ``ops.nfft_ewald_excl_virial``: what to SUBTRACT from the seven sums of the virial"""
    box = (1.0, 0.0, 1.0, 0.0, 0.0, 1.0) if splitting.box is None else splitting.box6
    return ops.nfft_ewald_excl_virial(pos, x, batch, exclusions.row_start, exclusions.col, exclusions.weight(kind), box,
                                      splitting.alpha, kind)

