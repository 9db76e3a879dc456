"""Periodic Rotne-Prager-Yamakawa sum: the velocities of a periodic suspension of spheres of radius ``a`` under forces, the
mobility that Brownian and Stokesian dynamics evaluate, NFFT far field + wrapped pair sum (no reference counterpart; DESIGN.md
section 7n; Rotne and Prager, J. Chem. Phys. 50, 4831 (1969); Yamakawa, J. Chem. Phys. 53, 436 (1970); Beenakker, J. Chem. Phys.
85, 1581 (1986); Fiore, Balboa Usabiaga, Donev and Swan, J. Chem. Phys. 146, 124116 (2017)).

Notation, units and conventions are those of ``stokeslet.py``: ``u`` is in the unit where the velocity is ``u / (8 pi eta)``, the
``k = 0`` mode is dropped.  The tensor is the Stokeslet ``S`` with its finite-size correction and a regularised form for
overlapping spheres::

    R(d)    = (1 + (a^2 / 3) lap) S(d) = (1 / r + 2 a^2 / (3 r^3)) I + (1 / r^3 - 2 a^2 / r^5) d d^T        r >= 2 a
    R_ov(d) = (4 / (3 a)) ((1 - 9 r / (32 a)) I + 3 d d^T / (32 a r))                                   r <  2 a
    u_i     = sum'_{j, p} R(x_i - x_j + p) f_j + (4 / (3 a)) f_i

``R`` is C^1 at ``r = 2 a`` and the sum is symmetric positive definite for every configuration.  With ``d``, ``r``, ``m``, ``g``
and the Smith functions ``B_l = ((2 l - 1) B_(l-1) + (2 alpha^2)^(l-1) g) / r^2`` of ``stokeslet.py``, ``q = a^2 / 3``, ``tau = 2 pi kappa``::

    u_i,a  =   sum_{j: 0 < r < r_c} W1 f_j,a + W2 m d_a                                                              near
             + the Stokeslet far sum with c_k (1 - q |tau|^2)                                                        far
             + (4 / (3 a) - 4 alpha / sqrt(pi) + 40 a^2 alpha^3 / (9 sqrt(pi))) f_i,a                                 self
    G_i,ab =   sum_j D1 f_j,a d_b + D2 m d_a d_b + W2 (m delta_ab + d_a f_j,b)  +  far with the further factor 2 pi i kappa_b
    W1 = (B_0 - g) + q (2 B_1 + (8 alpha^2 - 4 alpha^4 r^2) g)                 W2 = B_1 + q (4 alpha^4 g - 2 B_2)
    D1 = W1' / r = (2 alpha^2 g - B_1) + q (-2 B_2 + (8 alpha^6 r^2 - 24 alpha^4) g)     D2 = W2' / r = -B_2 + q (2 B_3 - 8 alpha^6 g)

and for ``r < 2 a`` the weights carry ``R_ov - R`` in addition, unscreened: the overlap belongs to the pair sum alone, which is
why ``2 a <= r_cut`` is required.  The far part is the Stokeslet sum's -- one adjoint transform, its spectral pass with the table
``rpy_coeffs`` and one forward transform -- the near part is one native pair sweep (``ops.nfft_ewald_rpy_near``).
"""
import math

import torch
from torch.autograd.function import once_differentiable

from . import ops
from .ewald import EwaldSplitting, _fractional, _set_sums
from .nfft import nfft_adjoint, nfft_forward
from .stokeslet import SAFETY, _check, _matrix, _smallest, _symmetric_backward


def _radius(what, radius, r_cut):
    if radius is None:
        raise ValueError("%s: radius, the radius of the spheres, is required" % what)
    radius = float(radius)
    if not (radius > 0.0 and math.isfinite(radius)):
        raise ValueError("%s: radius must be positive" % what)
    if 2.0 * radius > r_cut:
        raise ValueError("%s: 2 radius <= r_cut is required (the overlap of two spheres belongs to the pair sum), radius %g, "
                         "r_cut %g" % (what, radius, r_cut))
    return radius


def rpy_coeffs(splitting, radius):
    """``[N, N, N]`` float32 on the device of ``splitting.coeffs``: ``c_k (1 - (a^2 / 3) |2 pi kappa|^2)`` with the ``c_k`` of
    ``EwaldSplitting.stokeslet_coeffs`` and ``a = radius``, the far field's coefficients of ``nfft_ewald_rpy``, from the float64
    values on the host; zero exactly where ``stokeslet_coeffs`` is.  Built on first use and kept on the splitting, one table
    per radius."""
    if not isinstance(splitting, EwaldSplitting):
        raise TypeError("rpy_coeffs: splitting must be an EwaldSplitting")
    radius = _radius("rpy_coeffs", radius, math.inf)
    tables = splitting.__dict__.setdefault("_rpy_coeffs", {})
    c = tables.get(radius)
    if c is None:
        k2 = (splitting._kappa() ** 2).sum(3)
        c = 2.0 * splitting._b64 * (1.0 + (math.pi / splitting.alpha) ** 2 * k2) * (1.0 - radius * radius / 3.0 * 4.0 * math.pi ** 2 * k2)
        c = c.to(torch.float32).to(splitting.coeffs.device)
        c = tables[radius] = torch.where(splitting.stokeslet_coeffs == 0, torch.zeros_like(c), c).contiguous()
    return c


def self_coefficient(alpha, radius):
    """``4 / (3 a) - 4 alpha / sqrt(pi) + 40 a^2 alpha^3 / (9 sqrt(pi))``: the sphere's own mobility less what the far sum holds of it"""
    return 4.0 / (3.0 * radius) - 4.0 * alpha / math.sqrt(math.pi) + 40.0 * radius ** 2 * alpha ** 3 / (9.0 * math.sqrt(math.pi))


def _rpy(f, pos, batch, splitting, radius, cutoff, order):
    """``[n, 3 or 12, *cols]``: u and at ``order = 2`` the nine entries of G, row-major, of the forces ``f`` ``[n, 3, *cols]``,
    without autograd: far field, pair sweep, self term (with a box: ``pos`` fractional; ``f``, ``u`` and ``G`` Cartesian)"""
    N, alpha = splitting.bandwidth, splitting.alpha
    box = () if splitting.box is None else splitting.box6
    band = nfft_adjoint(f, pos, batch, bandwidth=N, cutoff=cutoff)  # [B, N, N, N, 3, *cols]
    spectra = ops.nfft_ewald_stokeslet_spectral(band, rpy_coeffs(splitting, radius), box, order)  # [B, N, N, N, 3 or 12, *cols]
    out = nfft_forward(spectra, pos, batch, cutoff=cutoff, real_output=True)
    out = out + ops.nfft_ewald_rpy_near(pos, f, batch, box, alpha, splitting.r_cut, radius, order)
    out[:, :3] += self_coefficient(alpha, radius) * f
    return out


class NfftEwaldRpyFunction(torch.autograd.Function):
    """``(u, G)`` of ``nfft_ewald_rpy`` (``G`` empty without ``gradient``).  The operator ``f -> u`` is real symmetric, so the
    backward is that of ``NfftEwaldStokesletFunction``: ``df = u[g]`` and ``dL/dpos`` from one evaluation of order 2 with ``f`` and
    ``g`` side by side.  First order only (``once_differentiable``); ``G`` is not differentiable."""

    @staticmethod
    def forward(ctx, f, pos, batch, splitting, radius, cutoff, gradient):
        if batch is not None and batch.requires_grad:
            raise AssertionError("nfft_ewald_rpy is differentiable w.r.t. f and pos only, but batch requires grad")
        ctx.splitting, ctx.radius, ctx.cutoff = splitting, radius, cutoff
        ctx.save_for_backward(f, pos, batch)
        out = _rpy(f, pos, batch, splitting, radius, cutoff, 2 if gradient else 1)
        G = _matrix(out[:, 3:]).clone() if gradient else f.new_empty(0)
        ctx.mark_non_differentiable(G)
        return out[:, :3].clone(), G

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _):
        f, pos, batch = ctx.saved_tensors
        df, dpos = _symmetric_backward(lambda x, order: _rpy(x, pos, batch, ctx.splitting, ctx.radius, ctx.cutoff, order), f, g,
                                       ctx.splitting, *ctx.needs_input_grad[:2])
        return df, dpos, None, None, None, None, None


def nfft_ewald_rpy(f, pos, batch=None, /, splitting=None, radius=None, cutoff=4, gradient=False, fractional=False):
    """The periodic Rotne-Prager-Yamakawa sum ``u_i = sum'_{j, p} R(x_i - x_j + p) f_j + (4 / (3 a)) f_i`` of the forces ``f``
    ``[n, 3, *cols]`` (float32, Cartesian) on spheres of the radius ``a = radius`` at ``pos`` ``[n, 3]``, over the spheres of i's
    point set (``batch``: sorted point-set indices) and all their periodic images, with zero mean flow; ``R`` is the tensor of
    the module's docstring, its overlap form for ``r < 2 a`` included.  The velocity is ``u / (8 pi eta)``: ``f -> u`` is the
    mobility matrix times ``8 pi eta``, symmetric positive definite for every configuration.  Coincident spheres do not see
    each other in the pair sum.

    Returns ``u`` ``[n, 3, *cols]``; with ``gradient=True`` ``(u, G)``, ``G_ab = d u_a / d x_b`` ``[n, 3, 3, *cols]``.  ``splitting``
    is an ``EwaldSplitting`` (TypeError otherwise; ``rpy_splitting`` chooses one for a tolerance); ``radius`` is required, positive
    and at most ``splitting.r_cut / 2`` (ValueError).  Every other argument, check and refusal is that of
    ``nfft_ewald_stokeslet``.

    Differentiable once in ``f`` and ``pos`` through ``u``; ``G`` is not differentiable, a second derivative raises a
    RuntimeError, and ``batch`` must not require grad (AssertionError).  The gradient comes back in the coordinates that were
    passed."""
    _check("nfft_ewald_rpy", f, pos, batch, splitting, "Rotne-Prager-Yamakawa")
    radius = _radius("nfft_ewald_rpy", radius, splitting.r_cut)
    pos = _fractional("nfft_ewald_rpy", pos, splitting, fractional)
    u, G = NfftEwaldRpyFunction.apply(f, pos, batch, splitting, radius, int(cutoff), bool(gradient))
    return (u, G) if gradient else u


def nfft_ewald_rpy_power(f, pos, batch=None, /, splitting=None, radius=None, cutoff=4, fractional=False):
    """``P_b = 1/2 sum_{i in point set b} f_i . u_i`` with ``u = nfft_ewald_rpy(f, pos, batch, ...)``: ``[B, *cols]``, one value per
    point set and column, positive for every configuration and every force that is not zero (``P / (4 pi eta)`` is the rate at
    which the forces work on the fluid).  Its gradient in ``pos`` is ``dP/dpos_i,b = sum_a f_i,a G_i,ab`` summed over the columns."""
    _check("nfft_ewald_rpy_power", f, pos, batch, splitting, "Rotne-Prager-Yamakawa")
    u = nfft_ewald_rpy(f, pos, batch, splitting=splitting, radius=radius, cutoff=cutoff, fractional=fractional)
    return 0.5 * _set_sums((f * u).sum(1), batch)[0]


# ---- a splitting for a tolerance ---------------------------------------------------------------------------------------
def _peak(k, x):
    """``sup_{t >= x} (2 / sqrt(pi)) t^k e^(-t^2)``: the function rises up to ``t = sqrt(k / 2)``"""
    t = max(x, math.sqrt(0.5 * k))
    return 2.0 / math.sqrt(math.pi) * t ** k * math.exp(-t * t)


def near_tail(x, rho):
    """An upper bound of what one pair at the distance ``r >= r_c`` still contributes to u and to G, relative to the unscreened
    tensor and its gradient at that distance: ``x = alpha r_c``, ``rho = a^2 / (3 r_c^2) <= 1/12``.  ``stokeslet.near_tail`` with
    the ``a^2`` terms of the four weights, each term bounded on its own: ``r W1``, ``r^3 W2``, ``r^3 D1`` and ``r^5 D2`` are sums of
    ``erfc x`` and of ``x^k e^(-x^2)``, taken at their largest beyond ``x`` (``_peak``), so that the bound does not rise.  For u the
    two eigenvalues ``W1`` and ``W1 + r^2 W2 = 2 B_0 + q (4 alpha^2 g - 4 B_1)`` stand against ``(1 + 2 rho) / r`` and
    ``(2 - 4 rho) / r``; for G the four terms ``r^3 |D1| + (1 + sqrt 3) r^3 |W2| + r^5 |D2|`` against the same expression at
    ``alpha = 0``, ``(1 + 6 rho) + (1 + sqrt 3) (1 - 6 rho) + (3 - 30 rho)``."""
    e1, e3, e5, e7 = (_peak(k, x) for k in (1, 3, 5, 7))
    b0 = math.erfc(x)
    b1 = b0 + e1  # r^3 B_1
    b2 = 3.0 * b1 + 2.0 * e3  # r^5 B_2
    b3 = 5.0 * b2 + 4.0 * e5  # r^7 B_3
    across = (max(b0, e1) + rho * (2.0 * b1 + 8.0 * e3 + 4.0 * e5)) / (1.0 + 2.0 * rho)
    along = (2.0 * b0 + 4.0 * rho * (b1 + e3)) / (2.0 - 4.0 * rho)
    d1 = max(2.0 * e3, b1) + rho * (2.0 * b2 + 8.0 * e7 + 24.0 * e5)
    w2 = b1 + rho * (4.0 * e5 + 2.0 * b2)
    d2 = b2 + rho * (2.0 * b3 + 8.0 * e7)
    s3 = math.sqrt(3.0)
    G = (d1 + (1.0 + s3) * w2 + d2) / ((1.0 + 6.0 * rho) + (1.0 + s3) * (1.0 - 6.0 * rho) + (3.0 - 30.0 * rho))
    return max(across, along, G)


def far_tail(y, s):
    """``stokeslet.far_tail`` with the factor ``|1 - a^2 |tau|^2 / 3| <= 1 + (4 / 3) s^2 t^2`` under the integral, ``s = alpha a``,
    ``t = pi kappa / alpha``: for u ``(2 / sqrt(pi)) int_y^inf (1 + t^2) (1 + c t^2) e^(-t^2) dt`` and for G the same with the further
    ``2 t``, ``c = 4 s^2 / 3``, both in closed form and both falling for ``y >= 1.5``."""
    c = 4.0 * s * s / 3.0
    e = math.exp(-y * y) / math.sqrt(math.pi)
    ec = math.erfc(y)
    u = 1.5 * ec + y * e + c * (1.25 * ec + (2.5 * y + y ** 3) * e)
    G = 2.0 * e * ((2.0 + y * y) + c * (y ** 4 + 3.0 * y * y + 3.0))
    return max(u, G)


def rpy_splitting(tol, r_cut, radius, box=None, device="cuda"):
    """An ``EwaldSplitting`` for ``nfft_ewald_rpy`` with spheres of the radius ``radius`` whose two truncation tails, of u and
    of G, are at most ``tol``: ``stokeslet_splitting`` with the tails of this sum's own kernels, ``near_tail`` and ``far_tail`` of
    this module (the far one depends on ``alpha a`` and is taken at the ``alpha`` that the near one gives), the same ``SAFETY``
    and the same ValueErrors, and one more for ``radius <= 0`` or ``2 radius > r_cut``."""
    tol, r_cut, A, longest = EwaldSplitting._tolerance_box(tol, r_cut, box)
    radius = _radius("rpy_splitting", radius, r_cut)
    rho = radius * radius / (3.0 * r_cut * r_cut)
    alpha = _smallest(lambda x: near_tail(x, rho), tol / SAFETY) / r_cut
    y = _smallest(lambda t: far_tail(t, alpha * radius), tol / SAFETY)
    N = max(2, 2 * math.ceil(alpha * y * longest / math.pi))
    return EwaldSplitting(alpha, r_cut, N, box=A, device=device)
