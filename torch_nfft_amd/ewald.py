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

Orthorhombic and triclinic boxes: ``EwaldSplitting(..., box=A)`` with the lower-triangular matrix
``A`` whose rows are the lattice vectors.  A Cartesian point is ``x = s A`` with fractional ``s`` in ``[-1/2, 1/2)^3``, the
wave vector of the integer frequency ``k`` is ``kappa = A^-1 k``, ``V = det A``, and::

    phi_i =   sum_{j != i, 0 < r_ij < r_c} q_j erfc(alpha r_ij) / r_ij          r_ij = |d_ij|, d_ij = (ds - rint(ds)) A, ds = s_i - s_j
            + sum_{k != 0} b_k e^{2 pi i k.s_i} sum_j q_j e^{-2 pi i k.s_j}      b_k = exp(-pi^2 |kappa|^2 / alpha^2) / (pi V |kappa|^2)
            - (2 alpha / sqrt(pi)) q_i - pi Q / (alpha^2 V)
    E_i   = -grad_x phi_i                                                       (Cartesian)

``alpha``, ``r_c``, ``phi`` and ``E`` are in the box's own Cartesian units.  The transforms run on the fractional
coordinates with anisotropic coefficients; the pair sweep is ``ops.nfft_ewald_near_box``.

The virial tensor: for the homogeneous strain ``A -> A (1 + eps)`` at fixed fractional coordinates,
``W_ab = -dU / d eps_ab`` of the energy ``U = 1/2 sum_i q_i phi_i`` is::

    W_ab =   1/2 sum_i q_i sum_{j: 0 < r_ij < r_c} (-g(r_ij^2)) d_ij,a d_ij,b q_j                       g = K'(r) / r, K = erfc(alpha r) / r
           + 1/2 sum_{k != 0} b_k |S_k|^2 (delta_ab - 2 (1 / |kappa|^2 + pi^2 / alpha^2) kappa_a kappa_b)  S_k = sum_j q_j e^{-2 pi i k.s_j}
           - pi Q^2 / (2 alpha^2 V) delta_ab

``W`` is symmetric, ``tr W = U`` for the converged sum, ``W / V`` is the Coulomb part of the pressure tensor and
``dU/dA = -A^-T W`` at fixed ``s`` (``nfft_ewald_virial``, ``virial_to_box_gradient``).

``nfft_ewald_step`` returns ``(phi, E, U, W)`` of one configuration from one adjoint transform, one spectral pass, one
forward transform and one walk over the pairs, where the two calls above repeat the first and the last.
"""
import ctypes
import math

import torch
from torch.autograd.function import once_differentiable

from . import _lib, ops
from . import exclusions as _exclusions
from .nfft import nfft_adjoint, nfft_forward, nfft_fastsum

MAX_R_CUT = 1.0 / 3.0  # the pair sweep needs 3 cells of edge >= r_cut per axis


def _box_matrix(box, what="EwaldSplitting"):
    """``box`` (length 3: the edges of an orthorhombic cell; or ``[3, 3]`` lower triangular, rows = lattice vectors) as a
    float64 ``[3, 3]`` tensor on the host.  ValueError for another shape, entries that are not finite, entries above the
    diagonal that are not zero or a diagonal that is not positive; AssertionError for a tensor that requires grad."""
    if isinstance(box, torch.Tensor):
        if box.requires_grad:
            raise AssertionError("%s is not differentiable w.r.t. the box, but box requires grad" % what)
        A = box.detach().to(device="cpu", dtype=torch.float64)
    else:
        A = torch.as_tensor(box, dtype=torch.float64)
    if A.shape == (3,):
        A = torch.diag(A)
    if A.shape != (3, 3):
        raise ValueError("%s: box must have length 3 (orthorhombic) or be [3, 3] lower triangular" % what)
    if not bool(torch.isfinite(A).all()):
        raise ValueError("%s: the entries of box must be finite" % what)
    if bool((torch.triu(A, 1) != 0).any()):
        raise ValueError("%s: box must be lower triangular (rows = lattice vectors a_1 = (A00, 0, 0), "
                         "a_2 = (A10, A11, 0), a_3); see the class docstring of EwaldSplitting for a general cell" % what)
    if not bool((torch.diagonal(A) > 0).all()):
        raise ValueError("%s: the diagonal of box must be positive" % what)
    return A.contiguous()


def _box_inverse(A):
    """``A^-1`` of the lower-triangular ``A`` (lower triangular too), in closed form"""
    a00, a10, a11, a20, a21, a22 = (float(A[i, j]) for i, j in ((0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2)))
    i00, i11, i22 = 1.0 / a00, 1.0 / a11, 1.0 / a22
    return torch.tensor([[i00, 0.0, 0.0],
                         [-a10 * i00 * i11, i11, 0.0],
                         [(a10 * a21 - a11 * a20) * i00 * i11 * i22, -a21 * i11 * i22, i22]], dtype=torch.float64)


def _box_widths(A):
    """the perpendicular widths ``w_a = 1 / |column a of A^-1|`` of the cell along its three fractional axes"""
    inv = _box_inverse(A)
    return tuple(1.0 / math.sqrt(float((inv[:, a] * inv[:, a]).sum())) for a in range(3))


class _TorusSplitting:
    """What ``EwaldSplitting`` and ``DispersionSplitting`` share: the checks of ``alpha``, ``r_cut``, ``bandwidth`` and
    ``box``, the attributes ``alpha``, ``r_cut``, ``bandwidth``, ``box``, ``volume``, ``widths`` and ``cells``, and the box's
    matrices.  A subclass turns ``|kappa|^2`` into its coefficients.  Messages carry the subclass's name."""

    def _setup(self, alpha, r_cut, bandwidth, box):
        """the checks and the attributes; returns ``|kappa|^2`` ``[N, N, N]`` float64 on the host (``|k|^2`` without a box)"""
        what = type(self).__name__
        alpha, r_cut, N = float(alpha), float(r_cut), int(bandwidth)
        if N != bandwidth or N < 2 or N % 2:
            raise ValueError("%s: bandwidth must be even and >= 2" % what)
        if not (alpha > 0.0 and math.isfinite(alpha)):
            raise ValueError("%s: alpha must be positive" % what)
        self._field_coeffs = None
        if box is None:
            if not 0.0 < r_cut <= MAX_R_CUT:
                raise ValueError("%s: r_cut must lie in (0, 1/3]" % what)
            self.alpha, self.r_cut, self.bandwidth = alpha, r_cut, N
            self.box, self.volume, self.widths = None, 1.0, (1.0, 1.0, 1.0)
            self.cells = (int(_lib.load().nfft_hip_ewald_near_cells(r_cut, 1)),) * 3
            k = torch.arange(-(N // 2), N // 2, dtype=torch.float64)
            return (k * k).reshape(N, 1, 1) + (k * k).reshape(1, N, 1) + (k * k).reshape(1, 1, N)
        A = _box_matrix(box, what)
        widths = _box_widths(A)
        if not 0.0 < r_cut <= min(widths) / 3.0:
            raise ValueError("%s: r_cut must lie in (0, min w_a / 3] = (0, %.6g] for this box (perpendicular "
                             "widths %.6g, %.6g, %.6g)" % ((what, min(widths) / 3.0) + widths))
        self.alpha, self.r_cut, self.bandwidth = alpha, r_cut, N
        self.box, self.widths = A, widths
        self.volume = float(A[0, 0] * A[1, 1] * A[2, 2])
        cells = (ctypes.c_int32 * 3)()
        six = (ctypes.c_double * 6)(*self.box6)
        if _lib.load().nfft_hip_ewald_box_cells(six, r_cut, 1, cells) < 0:
            raise ValueError("%s: %s" % (what, _lib.last_error()))
        self.cells = tuple(int(c) for c in cells)
        self._on_device = {}
        kappa = self._kappa()
        return (kappa * kappa).sum(3)

    @staticmethod
    def _zero_unpaired(b):
        """the planes ``k_a = -N/2`` have no partner ``+N/2``: zeroed, so that a real input gives a real sum"""
        b[0, :, :] = 0.0
        b[:, 0, :] = 0.0
        b[:, :, 0] = 0.0
        return b

    @classmethod
    def _tolerance_box(cls, tol, r_cut, box):
        """the checks of ``from_tolerance``: (``tol``, ``r_cut``, the box matrix or ``None``, the longest lattice vector)"""
        what = cls.__name__
        tol, r_cut = float(tol), float(r_cut)
        if not 0.0 < tol < 1.0:
            raise ValueError("%s.from_tolerance: tol must lie in (0, 1)" % what)
        if box is None:
            if not 0.0 < r_cut <= MAX_R_CUT:
                raise ValueError("%s: r_cut must lie in (0, 1/3]" % what)
            return tol, r_cut, None, 1.0
        A = _box_matrix(box, what)
        if not 0.0 < r_cut <= min(_box_widths(A)) / 3.0:
            raise ValueError("%s: r_cut must lie in (0, min w_a / 3] for this box" % what)
        return tol, r_cut, A, max(math.sqrt(float((A[a] * A[a]).sum())) for a in range(3))

    @property
    def box6(self):
        """``(A00, A10, A11, A20, A21, A22)``: the box as ``ops.nfft_ewald_near_box`` takes it"""
        A = self.box
        return tuple(float(A[i, j]) for i, j in ((0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2)))

    def _kappa(self):
        """``[N, N, N, 3]`` float64 on the host: the Cartesian wave vectors ``kappa_b = sum_a (A^-1)_ba k_a`` (without a
        box: ``k`` itself)"""
        N = self.bandwidth
        inv = torch.eye(3, dtype=torch.float64) if self.box is None else _box_inverse(self.box)
        k = torch.arange(-(N // 2), N // 2, dtype=torch.float64)
        ks = (k.reshape(N, 1, 1), k.reshape(1, N, 1), k.reshape(1, 1, N))
        return torch.stack([sum(float(inv[b, a]) * ks[a] for a in range(3)).expand(N, N, N) for b in range(3)], 3)

    def _matrices(self, device):
        """(``A`` float32, ``A^-1`` float64) on ``device``"""
        key = str(device)
        if key not in self._on_device:
            self._on_device[key] = (self.box.to(torch.float32).to(device), _box_inverse(self.box).to(device))
        return self._on_device[key]


class EwaldSplitting(_TorusSplitting):
    """The three parameters of the split, the box and the far field's coefficients.

    ``alpha > 0`` is the splitting parameter, ``r_cut`` in ``(0, 1/3]`` the radius of the pair sum, ``bandwidth`` (even)
    the number ``N`` of frequencies per axis.  ``coeffs`` is ``[N, N, N]`` float32 on ``device``: ``b_k`` at index
    ``k + N/2``, evaluated in float64 on the host, ``b_0 = 0`` and the unpaired planes ``k_a = -N/2`` zeroed.
    ValueError for an odd or too small ``bandwidth``, ``alpha <= 0`` or ``r_cut`` outside ``(0, 1/3]``.

    ``box`` is ``None`` (the unit cube), a sequence of three edges ``(Lx, Ly, Lz)`` (orthorhombic) or a ``[3, 3]``
    lower-triangular matrix ``A`` whose rows are the lattice vectors ``a_1 = (A00, 0, 0)``, ``a_2 = (A10, A11, 0)``,
    ``a_3 = (A20, A21, A22)`` with a positive diagonal (the LAMMPS / GROMACS convention).  ``alpha`` and ``r_cut`` are
    then in the box's Cartesian units, ``r_cut`` at most ``min_a w_a / 3`` for the perpendicular widths
    ``w_a = 1 / |column a of A^-1|``, and ``coeffs`` holds ``exp(-pi^2 |kappa|^2 / alpha^2) / (pi V |kappa|^2)`` with
    ``kappa = A^-1 k``, ``V = det A``.  ValueError for entries above the diagonal that are not zero, a diagonal that is
    not positive or ``r_cut > min_a w_a / 3``; a ``box`` tensor that requires grad is refused (AssertionError).

    A general cell ``M`` (rows = lattice vectors, any orientation) is brought to this form by a QR factorisation of its
    transpose: ``Q, R = qr(M^T)``, signs flipped so that ``diag R > 0`` (``Q <- Q D``, ``R <- D R``, ``D = diag(sign
    R_ii)``), then ``box = R^T`` and the positions are rotated with it, ``pos <- pos Q``; fractional coordinates do not
    change.  The field comes out in the rotated frame: ``E Q^T`` is the field in the original one.

    Attributes: ``box`` (``[3, 3]`` float64 on the host, or ``None``), ``volume``, ``widths`` and ``cells`` (the cell counts
    of the pair sweep for one point set)."""
    _A_NAME = "an EwaldSplitting"

    def __init__(self, alpha, r_cut, bandwidth, box=None, device="cuda"):
        k2 = self._setup(alpha, r_cut, bandwidth, box)
        N = self.bandwidth
        if box is not None:
            b = torch.exp(-(math.pi / self.alpha) ** 2 * k2) / (math.pi * self.volume * torch.where(k2 > 0, k2, torch.ones_like(k2)))
        else:
            b = torch.exp(-(math.pi / self.alpha) ** 2 * k2) / (math.pi * k2.clamp(min=1.0))
        b[N // 2, N // 2, N // 2] = 0.0
        self._b64 = self._zero_unpaired(b)
        self.coeffs = b.to(torch.float32).to(torch.device(device)).contiguous()

    @classmethod
    def from_tolerance(cls, tol, r_cut, box=None, device="cuda"):
        """``alpha = sqrt(-ln tol) / r_cut`` and ``bandwidth`` the next even integer ``>= 2 alpha sqrt(-ln tol) / pi``:
        the two truncation factors -- ``erfc(alpha r_c) ~ e^(-alpha^2 r_c^2)`` of the pair sum at ``r_cut`` and
        ``e^(-pi^2 k^2 / alpha^2)`` of the far sum at ``k = N/2`` -- both set to ``tol``.  A rule of thumb, not a bound:
        the errors of the two sums also carry the number of charges and the prefactors ``1/r`` and ``1/(pi k^2)``.

        With a ``box`` the plane ``k_a = N/2`` lies at the distance ``(N/2) / |a_a|`` from the origin of reciprocal space,
        so ``bandwidth`` is the next even integer ``>= 2 alpha sqrt(-ln tol) max_a |a_a| / pi``.  The grid is cubic in
        ``N``: the longest lattice vector sets ``N`` for all three axes."""
        tol, r_cut, A, longest = cls._tolerance_box(tol, r_cut, box)
        s = math.sqrt(-math.log(tol))
        alpha = s / r_cut
        N = max(2, 2 * math.ceil(alpha * s * longest / math.pi))
        return cls(alpha, r_cut, N, box=A, device=device)

    @property
    def stokeslet_coeffs(self):
        """``[N, N, N]`` float32 on the device of ``coeffs``: ``c_k = 2 b_k (1 + pi^2 |kappa|^2 / alpha^2)``, the far field's
        coefficients of the periodic Stokeslet sum (``stokeslet.py``), from the float64 values on the host; zero at ``k = 0``
        and on the unpaired planes, as ``b_k`` is (built on first use)"""
        c = self.__dict__.get("_stokeslet_coeffs")
        if c is None:
            kappa = self._kappa()
            c = 2.0 * self._b64 * (1.0 + (math.pi / self.alpha) ** 2 * (kappa * kappa).sum(3))
            c = self._stokeslet_coeffs = c.to(torch.float32).to(self.coeffs.device).contiguous()
        return c

    def field_coeffs(self):
        """``[N, N, N, 4]`` complex64: ``b_k`` and, for the three axes, ``(+2 pi i k_a) b_k`` -- the coefficients of
        ``phi`` and of ``E = -grad phi`` as four columns of one forward transform (built on first use).  With a box the
        three are ``(+2 pi i kappa_b) b_k``, the Cartesian components, from the float64 values on the host."""
        if self._field_coeffs is None and self.box is not None:
            b = self._b64
            cols = [torch.complex(b, torch.zeros_like(b))]
            kappa = self._kappa()
            for a in range(3):
                cols.append(torch.complex(torch.zeros_like(b), 2.0 * math.pi * kappa[..., a] * b))
            self._field_coeffs = torch.stack(cols, 3).to(torch.complex64).to(self.coeffs.device).contiguous()
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


def _ewald(q, pos, batch, splitting, cutoff, field, exclusions=None):
    """(phi, E or None) without autograd: far field, pair sweep, self and background terms (with a box: ``pos`` fractional,
    ``E`` Cartesian).  The listed pairs of ``exclusions`` are taken out of the pair sweep's sums before anything else is added
    to them: where a listed pair's 1 / r dominates a point's sum the two are within a factor of two of each other and that
    difference is exact, and the far field, the self and the background term are not rounded at the size of 1 / r."""
    N = splitting.bandwidth
    if field:
        cols = [1] * (q.dim() - 1)
        band = nfft_adjoint(q, pos, batch, bandwidth=N, cutoff=cutoff)  # [B, N, N, N, *cols]
        band = band.unsqueeze(4) * splitting.field_coeffs().reshape([1, N, N, N, 4] + cols)
        far = nfft_forward(band, pos, batch, cutoff=cutoff, real_output=not q.is_complex())  # [n, 4, *cols]
        phi, E = far[:, 0], far[:, 1:]
    else:
        phi, E = nfft_fastsum(q, splitting.coeffs, pos, None, batch, None, cutoff=cutoff), None
    alpha = splitting.alpha
    if splitting.box is not None:
        z, f = ops.nfft_ewald_near_box(pos, q, batch, splitting.box6, alpha, splitting.r_cut, field)
    else:
        z, f = ops.nfft_ewald_near(pos, q, batch, splitting.alpha, splitting.r_cut, field)
    if exclusions is not None:
        zx, fx = _exclusions.correction(_exclusions.COULOMB, q, pos, batch, splitting, exclusions, field)
        z, f = z - zx, (f - fx if field else f)
    background = math.pi / (alpha * alpha * splitting.volume)
    phi = phi + z - (2.0 * alpha / math.sqrt(math.pi)) * q - background * _set_sums(q, batch)[1]
    return phi, (E + f if field else None)


def _symmetric_backward(evaluate, ctx, g):
    """The backward of a real symmetric operator ``q -> phi`` whose field ``E[q] = -grad phi`` comes with it
    (``evaluate(q, pos, batch, splitting, cutoff, field) -> (phi, E)``): ``dq`` is the operator applied to ``g``,
    ``dpos_i = -sum_c (g_ic E[q_c]_i + q_ic E[g_c]_i)``, times ``A^T`` with a box (``pos`` fractional, ``E`` Cartesian)."""
    q, pos, batch = ctx.saved_tensors
    need_q, need_pos = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    g = g.contiguous()
    dq = dpos = None
    if getattr(ctx, "exclusions", None) is not None:  # (symmetric weights: the corrected operator is symmetric too)
        all_pairs, exclusions = evaluate, ctx.exclusions
        evaluate = lambda *args: all_pairs(*args, exclusions)  # noqa: E731
    if need_pos:
        phi, E = evaluate(torch.stack([q, g], 1), pos, batch, ctx.splitting, ctx.cutoff, True)  # [n, (3,) 2, *cols]
        dq = phi[:, 1]
        w = g.unsqueeze(1).conj() * E[:, :, 0] + q.unsqueeze(1).conj() * E[:, :, 1]
        w = w.real if w.is_complex() else w
        dpos = -w.reshape(w.size(0), 3, math.prod(w.shape[2:])).sum(2)
        if ctx.splitting.box is not None:
            dpos = dpos @ ctx.splitting._matrices(dpos.device)[0].t()
    elif need_q:
        dq = evaluate(g, pos, batch, ctx.splitting, ctx.cutoff, False)[0]
    return dq if need_q else None, dpos, None, None, None, None


class NfftEwaldFunction(torch.autograd.Function):
    """``(phi, E)`` of ``nfft_ewald`` (``E`` empty without ``field``).  The operator ``q -> phi`` is real symmetric, so for
    ``g = dL/dphi`` the gradient in ``q`` is the operator applied to ``g``, and the gradient in the positions is
    ``dL/dpos_i = -sum_c (g_ic E[q_c]_i + q_ic E[g_c]_i)``: one field evaluation with ``q`` and ``g`` side by side as
    columns.  First order only (``once_differentiable``); ``E`` is not differentiable.  With a box ``pos`` holds the
    fractional coordinates ``s`` (``x = s A``), ``E`` is Cartesian, the formula gives ``dL/dx`` and the backward returns
    ``dL/ds = (dL/dx) A^T``."""

    @staticmethod
    def forward(ctx, q, pos, batch, splitting, cutoff, field, exclusions=None):
        if batch is not None and batch.requires_grad:
            raise AssertionError("nfft_ewald is differentiable w.r.t. q and pos only, but batch requires grad")
        ctx.splitting, ctx.cutoff, ctx.exclusions = splitting, cutoff, exclusions
        ctx.save_for_backward(q, pos, batch)
        phi, E = _ewald(q, pos, batch, splitting, cutoff, field, exclusions)
        if E is None:
            E = q.new_empty(0)
        ctx.mark_non_differentiable(E)
        return phi, E

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _):
        return _symmetric_backward(_ewald, ctx, g) + (None,)


def _check(what, q, pos, batch, splitting, differentiable=True):
    if not isinstance(splitting, EwaldSplitting):
        raise TypeError("%s: splitting must be an EwaldSplitting" % what)
    if pos.dim() != 2 or pos.size(1) != 3:
        raise ValueError("%s: the periodic 1/r sum is three-dimensional, pos must be [n, 3]" % what)
    if batch is not None and batch.requires_grad:
        if differentiable:
            raise AssertionError("%s is differentiable w.r.t. q and pos only, but batch requires grad" % what)
        raise AssertionError("%s: batch holds point-set indices and must not require grad" % what)


def _fractional(what, pos, splitting, fractional):
    """the positions as the Function takes them: as they are without a box, fractional with one"""
    if splitting.box is None:
        if fractional:
            raise ValueError("%s: fractional=True needs %s with a box" % (what, splitting._A_NAME))
        return pos
    if fractional:
        return pos
    return (pos.double() @ splitting._matrices(pos.device)[1]).float()


def nfft_ewald(q, pos, batch=None, /, splitting=None, cutoff=4, field=False, fractional=False, exclusions=None):
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
    differentiable, a second derivative raises a RuntimeError, and ``batch`` must not require grad (AssertionError).

    With ``splitting.box`` set the charges live in that box: ``pos`` is Cartesian, ``x = s A``, taken modulo the lattice
    (converted in float64, ``s = pos A^-1``, and rounded to float32), or with ``fractional=True`` the fractional
    coordinates ``s`` themselves, taken modulo 1.  ``phi`` and ``E`` are in the box's units and ``E`` is always Cartesian;
    the gradient comes back in the coordinates that were passed (``dL/ds = (dL/dx) A^T``).  Without a box ``fractional``
    must stay False (ValueError).

    ``exclusions`` is ``None`` or an ``ExclusionList`` over the ``n`` points (TypeError for anything else, ValueError for
    another point count): every listed pair ``{i, j}`` loses ``(1 - s^C_ij) q_j / r`` in ``phi_i`` and
    ``(1 - s^C_ij) q_j d_ij / r^3`` in ``E_i`` for the one image ``d_ij`` that the sweep sees (a pair at ``r = 0``:
    ``(1 - s^C_ij) q_j 2 alpha / sqrt(pi)`` and no field), by one more native call; the operator stays symmetric and the
    gradients are those of the corrected sum.  The sweep has added the pair before the correction removes it: an
    excluded pair at the separation ``r`` leaves a rounding of about ``2^-24 |q_j| / r`` in ``phi_i`` (``exclusions.py``)."""
    _check("nfft_ewald", q, pos, batch, splitting)
    exclusions = _exclusions.check_exclusions("nfft_ewald", exclusions, pos)
    pos = _fractional("nfft_ewald", pos, splitting, fractional)
    if exclusions is None:
        phi, E = NfftEwaldFunction.apply(q, pos, batch, splitting, int(cutoff), bool(field))
    else:
        phi, E = NfftEwaldFunction.apply(q, pos, batch, splitting, int(cutoff), bool(field), exclusions)
    return (phi, E) if field else phi


def nfft_ewald_energy(q, pos, batch=None, /, splitting=None, cutoff=4, fractional=False, exclusions=None):
    """``U_b = 1/2 sum_{i in point set b} q_i phi_i`` with ``phi = nfft_ewald(q, pos, batch, ...)``: ``[B, *cols]``, one
    energy per point set and column (bilinear in ``q``: no conjugate for complex charges).  Its gradient in ``pos`` is
    minus the force, ``dU/dpos_i = -q_i E_i`` summed over the columns (Cartesian ``pos`` in a box; ``fractional`` as for
    ``nfft_ewald``); ``exclusions`` as there: every listed pair loses ``(1 - s^C_ij) q_i q_j / r``."""
    _check("nfft_ewald_energy", q, pos, batch, splitting)
    if splitting.box is None and fractional:
        raise ValueError("nfft_ewald_energy: fractional=True needs an EwaldSplitting with a box")
    phi = nfft_ewald(q, pos, batch, splitting=splitting, cutoff=cutoff, fractional=fractional, exclusions=exclusions)
    return 0.5 * _set_sums(q * phi, batch)[0]


_IDENTITY6 = (1.0, 0.0, 1.0, 0.0, 0.0, 1.0)
_VOIGT = ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))  # the order of the two native reductions after the energy


def _voigt_to_matrix(six):
    """``[B, 6, *cols]`` in that order as the symmetric ``[B, 3, 3, *cols]``"""
    W = six.new_zeros((six.size(0), 3, 3) + tuple(six.shape[2:]))
    for e, (a, b) in enumerate(_VOIGT):
        W[:, a, b] = six[:, e]
        W[:, b, a] = six[:, e]
    return W


def nfft_ewald_virial(q, pos, batch=None, /, splitting=None, cutoff=4, fractional=False, exclusions=None):
    """``(U, W)``: the energy ``U_b = 1/2 sum_{i in point set b} q_i phi_i`` ``[B, *cols]`` of ``nfft_ewald_energy`` and
    the virial tensor ``W_ab = -dU / d eps_ab`` ``[B, 3, 3, *cols]`` for the homogeneous strain ``A -> A (1 + eps)`` of the
    box at fixed fractional coordinates, per point set and column, both with the dtype of ``q``.  ``W`` is symmetric and
    in the box's units (energy); ``tr W = U`` up to the truncation of the sum; ``W / splitting.volume`` is the Coulomb part
    of the pressure tensor, and ``virial_to_box_gradient(W, splitting.box)`` the gradient of ``U`` in the box's entries.

    ``q`` ``[n, *cols]`` must be real (float32): the energy is bilinear and for complex charges the far part is not
    ``|S_k|^2`` (ValueError).  ``pos``, ``batch``, ``splitting``, ``cutoff`` and ``fractional`` are those of ``nfft_ewald``;
    without a box the cell is the unit cube.

    One adjoint transform, then two native reductions -- over the frequencies of its output and over the pairs within
    ``r_cut`` -- in float64 and without atomics (they give the same bits on every call; the transform before them spreads
    with float atomics, so the whole does not); the self term ``-(alpha / sqrt(pi))
    sum q_i^2`` (in ``U`` only: it has no strain in it) and the background ``-pi Q^2 / (2 alpha^2 V)`` (in ``U`` and on the
    diagonal of ``W``) are added in float64 before the cast.  With ``exclusions`` (as for ``nfft_ewald``) a third native
    reduction of the same kind takes ``(1 - s^C_ij) q_i q_j / r`` out of ``U`` and ``(1 - s^C_ij) q_i q_j d_a d_b / r^3`` out of
    ``W`` for every listed pair (``tr W = U`` stays; a pair at ``r = 0``: ``(1 - s^C_ij) q_i q_j 2 alpha / sqrt(pi)`` in ``U`` only).

    Runs under ``torch.no_grad()``: ``U`` and ``W`` are constants to autograd.  Inputs that require grad are accepted and
    get no gradient from here (use ``nfft_ewald_energy`` for forces); ``batch`` must not require grad (AssertionError)."""
    _check("nfft_ewald_virial", q, pos, batch, splitting, differentiable=False)
    if q.is_complex():
        raise ValueError("nfft_ewald_virial: the charges must be real (the energy is bilinear in q)")
    exclusions = _exclusions.check_exclusions("nfft_ewald_virial", exclusions, pos)
    with torch.no_grad():
        q, pos = q.detach(), pos.detach()
        pos = _fractional("nfft_ewald_virial", pos, splitting, fractional)
        alpha, N = splitting.alpha, splitting.bandwidth
        box6 = _IDENTITY6 if splitting.box is None else splitting.box6
        band = nfft_adjoint(q, pos, batch, bandwidth=N, cutoff=int(cutoff))  # [B, N, N, N, *cols]
        seven = ops.nfft_ewald_virial_far(band, splitting.coeffs, box6, alpha)
        seven = seven + ops.nfft_ewald_virial_near(pos, q, batch, box6, alpha, splitting.r_cut)  # [B, 7, *cols] float64
        if exclusions is not None:
            seven = seven - _exclusions.virial_correction(_exclusions.COULOMB, q, pos, batch, splitting, exclusions)
        q64 = q.double()
        total = _set_sums(q64, batch)[0]
        background = (math.pi / (2.0 * alpha * alpha * splitting.volume)) * total * total
        U = seven[:, 0] - (alpha / math.sqrt(math.pi)) * _set_sums(q64 * q64, batch)[0] - background
        W = _voigt_to_matrix(seven[:, 1:])
        for a in range(3):
            W[:, a, a] -= background
        return U.to(q.dtype), W.to(q.dtype)


def nfft_ewald_step(q, pos, batch=None, /, splitting=None, cutoff=4, fractional=False, exclusions=None):
    """``(phi, E, U, W)``: what one constant-pressure or cell-relaxation step needs from the Coulomb sum, in one pass
    (DESIGN.md section 7q).  ``phi`` ``[n, *cols]`` and ``E = -grad phi`` ``[n, 3, *cols]`` (Cartesian, in the box's units)
    are those of ``nfft_ewald(q, pos, batch, field=True)``, ``U`` ``[B, *cols]`` and ``W`` ``[B, 3, 3, *cols]`` those of
    ``nfft_ewald_virial(q, pos, batch)``, all with the dtype of ``q``: the same definitions, self and background terms and
    float64 assembly of ``U`` and ``W`` before the cast.  The forces are ``q_i E_i``.

    ``q`` ``[n, *cols]`` must be real (float32; ValueError).  ``pos``, ``batch``, ``splitting``, ``cutoff``, ``fractional`` and
    ``exclusions`` are those of ``nfft_ewald``; without a box the cell is the unit cube.

    One adjoint transform, one native spectral pass (the four spectra of ``(phi, E)`` and the frequencies' share of ``U`` and
    ``W`` from one read), one forward transform of the four spectra, one native walk over the pairs within ``r_cut`` (ten sums
    per point and column, of which seven are reduced in float64), then the terms -- where the two separate calls do the
    adjoint transform and the walk twice.  With ``exclusions`` the listed pairs' shares are subtracted from the walk's sums
    before anything else is added to them, as in ``nfft_ewald``.  The two native steps use no atomics and give the same bits
    on every call; the transforms around them spread with float atomics, so the whole does not.

    Runs under ``torch.no_grad()``: all four outputs are constants to autograd.  Inputs that require grad are accepted and
    get no gradient from here; ``batch`` must not require grad (AssertionError)."""
    _check("nfft_ewald_step", q, pos, batch, splitting, differentiable=False)
    if q.is_complex():
        raise ValueError("nfft_ewald_step: the charges must be real (the energy is bilinear in q)")
    exclusions = _exclusions.check_exclusions("nfft_ewald_step", exclusions, pos)
    with torch.no_grad():
        q, pos = q.detach(), pos.detach()
        pos = _fractional("nfft_ewald_step", pos, splitting, fractional)
        alpha, N = splitting.alpha, splitting.bandwidth
        box6 = _IDENTITY6 if splitting.box is None else splitting.box6
        band = nfft_adjoint(q, pos, batch, bandwidth=N, cutoff=int(cutoff))  # [B, N, N, N, *cols]
        spectra, far7 = ops.nfft_ewald_step_spectral(band, splitting.coeffs, box6, alpha)
        far = nfft_forward(spectra, pos, batch, cutoff=int(cutoff), real_output=True)  # [n, 4, *cols]
        z, f, near7 = ops.nfft_ewald_step_near(pos, q, batch, box6, alpha, splitting.r_cut)
        if exclusions is not None:
            zx, fx = _exclusions.correction(_exclusions.COULOMB, q, pos, batch, splitting, exclusions, True)
            z, f = z - zx, f - fx
            near7 = near7 - _exclusions.virial_correction(_exclusions.COULOMB, q, pos, batch, splitting, exclusions)
        seven = far7 + near7
        background = math.pi / (alpha * alpha * splitting.volume)
        phi = far[:, 0] + z - (2.0 * alpha / math.sqrt(math.pi)) * q - background * _set_sums(q, batch)[1]
        E = far[:, 1:] + f
        q64 = q.double()
        total = _set_sums(q64, batch)[0]
        background = (0.5 * background) * total * total
        U = seven[:, 0] - (alpha / math.sqrt(math.pi)) * _set_sums(q64 * q64, batch)[0] - background
        W = _voigt_to_matrix(seven[:, 1:])
        for a in range(3):
            W[:, a, a] -= background
        return phi, E, U.to(q.dtype), W.to(q.dtype)


def virial_to_box_gradient(W, box):
    """``dU/dA`` at fixed fractional coordinates from the virial ``W`` ``[B, 3, 3, *cols]`` of ``nfft_ewald_virial``:
    ``tril(-A^-T W)`` ``[B, 3, 3, *cols]``, the six free entries of the lower-triangular box ``A`` (zeros above the
    diagonal).  ``box`` as ``EwaldSplitting`` takes it (three edges or ``[3, 3]`` lower triangular); ``None`` is the unit
    cube.  Pure torch, on the device and in the dtype of ``W``.

    The identity holds for any energy and its strain derivative, so the ``W`` of ``nfft_ewald_dispersion_virial`` goes
    through unchanged and gives the gradient of that function's ``U`` (the physical dispersion energy is ``-U``: negate)."""
    if W.dim() < 3 or W.size(1) != 3 or W.size(2) != 3:
        raise ValueError("virial_to_box_gradient: W must be [B, 3, 3, *cols]")
    inv = torch.eye(3, dtype=torch.float64) if box is None else _box_inverse(_box_matrix(box))
    inv = inv.to(device=W.device, dtype=W.dtype)
    g = -torch.einsum("ki,bkj...->bij...", inv, W)  # -(A^-T W)_ij = -sum_k (A^-1)_ki W_kj
    mask = torch.tril(torch.ones(3, 3, dtype=W.dtype, device=W.device))
    return g * mask.reshape((1, 3, 3) + (1,) * (W.dim() - 3))
