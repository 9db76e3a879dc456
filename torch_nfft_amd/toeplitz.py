"""The normal operator ``A^H W A`` of the NFFT as a Toeplitz product, and an iterative inverse built on it
(no reference counterpart).

With ``A = nfft_forward`` on fixed points and ``W = diag(weights)`` real,
``(A^H W A)[k, k'] = sum_i w_i exp(2 pi i (k - k').pos_i) = t[k - k']`` is a d-level Toeplitz matrix.  It embeds in a
circulant of size ``M = 2N`` per axis -- the oversampled grid of the transforms -- so one application is the forward
FFT stage, a pointwise product with a precomputed real grid ``K`` and the adjoint FFT stage: no points, no plan, no
spreading and no gather, at a cost independent of the number of points.  The window error enters once, through ``t``,
instead of twice as in ``nfft_adjoint(w * nfft_forward(x))``.

``nfft_toeplitz_kernel`` builds ``K`` once per (points, weights); ``nfft_normal`` applies it (linear, self-adjoint,
differentiable in ``x`` to any order); ``nfft_inverse`` runs conjugate gradients on ``A^H W A x = A^H W y``.
"""
import torch

from . import ops
from .nfft import nfft_adjoint


def nfft_toeplitz_kernel(pos, batch=None, weights=None, bandwidth=16, cutoff=3):
    """Kernel grid ``K`` ``[B, 2N, ..., 2N]`` float32 of the normal operator ``A^H W A`` at bandwidth ``N`` for the points
    ``pos`` ``[n, d]`` (point sets ``batch``) and real weights ``[n]`` (``None``: ones).

    Internally ``t = nfft_adjoint(weights, pos, batch, bandwidth=2N, cutoff)`` followed by one real FFT of size ``2N`` per
    axis, so it inherits that transform's limits and needs its workspace (a ``(4N)^d`` grid): in 3-D the transform's own
    FFT passes and matrix-core spreading cover grids up to ``1024^3``, i.e. ``N <= 256``; beyond that the set-up falls back
    to the general routes.  ``K`` takes ``4 (2N)^d`` bytes per point set (512 MiB at ``N = 256`` in 3-D).  ``cutoff`` sets
    the accuracy of ``t`` and thereby of the operator.  No gradient flows into ``pos`` or ``weights`` through ``K``.
    The adjoint goes through the point-plan cache like any other, so its bandwidth-``2N`` plan takes one of the cache's two
    entries until later transforms replace it (``ops.plan_cache_clear()`` frees it at once)."""
    for name, t in (("pos", pos), ("weights", weights), ("batch", batch)):
        if t is not None and t.requires_grad:
            raise AssertionError("nfft_toeplitz_kernel is not differentiable, but %s requires grad" % name)
    if weights is None:
        weights = torch.ones(pos.size(0), dtype=torch.float32, device=pos.device)
    if weights.is_complex():
        raise ValueError("nfft_toeplitz_kernel: weights must be real")
    if weights.dim() != 1 or weights.size(0) != pos.size(0):
        raise RuntimeError("Input mismatch: weights must have shape [n]")
    with torch.no_grad():
        t = ops.nfft_adjoint(pos, weights.to(torch.float32), batch, 2 * int(bandwidth), cutoff, 0)
        return ops.nfft_toeplitz_kernel(t)


class NfftNormalFunction(torch.autograd.Function):
    """y = T x with T = A^H W A given by its kernel grid: linear in x and self-adjoint, so the backward is T applied to
    dy (its real part for a real x) -- through this Function itself, hence differentiable to any order."""

    @staticmethod
    def forward(ctx, x, kernel):
        if kernel.requires_grad:
            raise AssertionError("nfft_normal is differentiable w.r.t. x only, but kernel requires grad")
        ctx.save_for_backward(kernel)
        ctx.real_input = not x.is_complex()
        return ops.nfft_normal(kernel, x)

    @staticmethod
    def backward(ctx, dy):
        kernel, = ctx.saved_tensors
        dx = NfftNormalFunction.apply(dy, kernel)
        return (dx.real if ctx.real_input else dx), None


def nfft_normal(x, kernel):
    """``A^H W A x`` for ``x`` ``[B, N, ..., N, *cols]`` (float32 or complex64) and ``kernel`` from
    ``nfft_toeplitz_kernel`` at the same bandwidth: ``[B, N, ..., N, *cols]`` complex64."""
    return NfftNormalFunction.apply(x, kernel)


def nfft_inverse(y, pos, batch=None, bandwidth=16, cutoff=3, weights=None, iterations=10, x0=None):
    """Least-squares inverse NFFT: ``iterations`` steps of conjugate gradients on ``A^H W A x = A^H W y`` for samples
    ``y`` ``[n, *cols]`` at the points ``pos``.  The right-hand side is one ``nfft_adjoint``, every iteration one
    ``nfft_normal``; the step sizes stay 0-d device tensors (no host synchronisation) and the iteration count is fixed.
    All columns and point sets share one Krylov iteration.  Returns ``(x, residuals)``: ``x`` ``[B, N, ..., N, *cols]``
    complex64 and the norms ``|A^H W y - A^H W A x_k|`` of the recurrence residual after each iteration, ``[iterations]``
    float32 on the device."""
    kernel = nfft_toeplitz_kernel(pos, batch, weights, bandwidth, cutoff)
    if weights is not None:
        y = y * weights.reshape([-1] + [1] * (y.dim() - 1))
    b = nfft_adjoint(y, pos, batch, bandwidth, cutoff)
    tiny = torch.finfo(torch.float32).tiny
    if x0 is None:
        x = torch.zeros_like(b)
        r = b
    else:
        x = x0.to(b.dtype)
        r = b - nfft_normal(x, kernel)
    p = r
    rs = torch.vdot(r.flatten(), r.flatten()).real
    residuals = []
    for _ in range(int(iterations)):
        tp = nfft_normal(p, kernel)
        alpha = rs / torch.vdot(p.flatten(), tp.flatten()).real.clamp_min(tiny)
        x = x + alpha * p
        r = r - alpha * tp
        rs_new = torch.vdot(r.flatten(), r.flatten()).real
        residuals.append(rs_new.sqrt())
        p = r + (rs_new / rs.clamp_min(tiny)) * p
        rs = rs_new
    res = torch.stack(residuals) if residuals else torch.zeros(0, dtype=torch.float32, device=b.device)
    return x, res
