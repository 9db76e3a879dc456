"""Public API: ``nfft_adjoint`` / ``nfft_forward`` / ``nfft_fastsum`` with the reference's signatures and
autograd behaviour (reference: ``torch_nfft/nfft.py:11-179``).

Adjoint and forward are each other's transposes, so each one's backward w.r.t. the coefficients is the other
(``nfft.py:22-28, 48-54``).  Not in the reference: both transforms are also differentiable w.r.t. the points ``pos``.
Both gradients come from one native gather of the window's derivative (``ops.nfft_forward_grad_points``):
``y = nfft_forward(x, pos)`` weights the derivative of its own output by ``dy``; ``y = nfft_adjoint(x, pos)`` gives
``dpos_i = Re(x_i conj(grad F(pos_i)))`` with ``F = nfft_forward(dy)``.  ``batch`` gets no gradient.  Under
``create_graph=True`` the backward passes are built from differentiable pieces -- the other transform and the gather
``_PointGradFunction`` -- so both transforms can be differentiated twice in ``x`` and ``pos``; the gather's own backward is
one native call (``ops.nfft_forward_grad_points_backward``), and a third derivative raises.

``nfft_fastsum`` is differentiable w.r.t. ``x``, ``sources`` and ``targets`` (not ``coeffs`` or the batch vectors).  With
``band = c * A_s(x)`` its forward pass's band spectrum (saved only when ``targets`` needs a gradient: ``B C N^d`` complex
values), ``dtargets`` is the gather of ``forward_t(band)`` weighted by ``dy`` and ``dsources_j = Re(conj(x_j) grad H(s_j))``
with ``H = forward_s(conj(c) * A_t(dy))``; one native backward call (``ops.nfft_fastsum_backward``).  For real ``c``,
``H`` is also ``dx`` and one gather returns both; for complex ``c``, ``dx`` stays the swapped fastsum.
"""
import math

import torch
from torch.autograd.function import once_differentiable

from . import ops


def _real_columns(t, n):
    """[n, Cr] float32 view of a coefficient array: the real columns, or re / im interleaved for complex data."""
    t = t.contiguous()
    r = torch.view_as_real(t) if t.is_complex() else t
    return r.reshape(n, math.prod(r.shape[1:]))  # (explicit column count: also for n = 0)


class _PointGradFunction(torch.autograd.Function):
    """G(pos, xhat, w)[i, a] = sum_cr w[i, cr] d Fr[i, cr] / d pos[i, a], Fr the real columns of nfft_forward(xhat, pos):
    the first-order point gradient of both transforms as a differentiable function of pos, xhat and w."""

    @staticmethod
    def forward(ctx, pos, xhat, batch, cutoff, real_output, w):
        ctx.save_for_backward(pos, xhat, batch, w)
        ctx.cutoff = cutoff
        ctx.real_output = real_output
        return ops.nfft_forward_grad_points(pos, xhat, batch, cutoff, real_output, w)

    @staticmethod
    @once_differentiable
    def backward(ctx, v):
        pos, xhat, batch, w = ctx.saved_tensors
        need_p, need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[5]
        dx, dw, dp = ops.nfft_forward_grad_points_backward(pos, xhat, batch, ctx.cutoff, ctx.real_output, w,
                                                           v.contiguous(), need_x, need_w, need_p)
        return dp if need_p else None, dx if need_x else None, None, None, None, dw if need_w else None


class NfftAdjointFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pos, batch, bandwidth, cutoff, real_output):
        y = ops.nfft_adjoint(pos, x, batch, bandwidth, cutoff, 1 if real_output else 0)
        ctx.pos_grad = ctx.needs_input_grad[1]
        if ctx.pos_grad:  # (x only for the gradient w.r.t. the points)
            ctx.save_for_backward(pos, batch, x)
        else:
            ctx.save_for_backward(pos, batch)
        ctx.cutoff = cutoff
        ctx.real_input = not x.is_complex()
        return y

    @staticmethod
    def backward(ctx, dy):
        pos, batch = ctx.saved_tensors[:2]
        dx = dpos = None
        if torch.is_grad_enabled():  # create_graph: differentiable pieces
            if ctx.needs_input_grad[0] or not ctx.pos_grad:
                dx = NfftForwardFunction.apply(dy, pos, batch, ctx.cutoff, ctx.real_input)
            if ctx.pos_grad:
                x = ctx.saved_tensors[2]
                dpos = _PointGradFunction.apply(pos, dy, batch, ctx.cutoff, ctx.real_input, _real_columns(x, pos.size(0)))
            return dx, dpos, None, None, None, None
        if ctx.needs_input_grad[0] or not ctx.pos_grad:
            dx = ops.nfft_forward(pos, dy, batch, ctx.cutoff, 1 if ctx.real_input else 0)
        if ctx.pos_grad:
            x = ctx.saved_tensors[2]
            w = _real_columns(x, pos.size(0))
            dpos = ops.nfft_forward_grad_points(pos, dy, batch, ctx.cutoff, 1 if ctx.real_input else 0, w)
        return dx, dpos, None, None, None, None


def nfft_adjoint(x, pos, batch=None, bandwidth=16, cutoff=3, real_output=False):
    """y[b, k+N/2, ...] ~= sum_{i in point set b} x[i, ...] exp(+2 pi i k.pos[i]),  k in [-N/2, N/2)^d."""
    return NfftAdjointFunction.apply(x, pos, batch, bandwidth, cutoff, real_output)


class NfftForwardFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pos, batch, cutoff, real_output):
        y = ops.nfft_forward(pos, x, batch, cutoff, 1 if real_output else 0)
        ctx.pos_grad = ctx.needs_input_grad[1]
        if ctx.pos_grad:  # (x only for the gradient w.r.t. the points)
            ctx.save_for_backward(pos, batch, x)
        else:
            ctx.save_for_backward(pos, batch)
        ctx.cutoff = cutoff
        ctx.bandwidth = x.size(1)
        ctx.real_input = not x.is_complex()
        ctx.real_output = bool(real_output)
        return y

    @staticmethod
    def backward(ctx, dy):
        pos, batch = ctx.saved_tensors[:2]
        dx = dpos = None
        if torch.is_grad_enabled():  # create_graph: differentiable pieces
            if ctx.needs_input_grad[0] or not ctx.pos_grad:
                dx = NfftAdjointFunction.apply(dy, pos, batch, ctx.bandwidth, ctx.cutoff, ctx.real_input)
            if ctx.pos_grad:
                x = ctx.saved_tensors[2]
                dpos = _PointGradFunction.apply(pos, x, batch, ctx.cutoff, ctx.real_output, _real_columns(dy, pos.size(0)))
            return dx, dpos, None, None, None
        if ctx.needs_input_grad[0] or not ctx.pos_grad:
            dx = ops.nfft_adjoint(pos, dy, batch, ctx.bandwidth, ctx.cutoff, 1 if ctx.real_input else 0)
        if ctx.pos_grad:
            x = ctx.saved_tensors[2]
            w = _real_columns(dy, pos.size(0))
            dpos = ops.nfft_forward_grad_points(pos, x, batch, ctx.cutoff, 1 if ctx.real_output else 0, w)
        return dx, dpos, None, None, None


def nfft_forward(x, pos, batch=None, cutoff=3, real_output=False):
    """y[i, ...] ~= sum_k x[batch[i], k+N/2, ...] exp(-2 pi i k.pos[i]),  N = x.size(1)."""
    return NfftForwardFunction.apply(x, pos, batch, cutoff, real_output)


class NfftFastsumFunction(torch.autograd.Function):
    """y = K x with the trigonometric kernel matrix K_ij = sum_l coeffs[l] exp(2 pi i l.(source_j - target_i)).
    Linear in x; its transpose swaps sources and targets (reference: nfft.py:62-88).  Not in the reference: gradients
    w.r.t. sources and targets."""

    @staticmethod
    def forward(ctx, x, coeffs, sources, targets, source_batch, target_batch, cutoff):
        # (reference: nfft.py:67-74 refuses everything but x)
        for name, t in (("coeffs", coeffs), ("source_batch", source_batch), ("target_batch", target_batch)):
            if t is not None and t.requires_grad:
                raise AssertionError("nfft_fastsum is differentiable w.r.t. x, sources and targets only, but %s requires "
                                     "grad" % name)
        ctx.points_grad = ctx.needs_input_grad[2] or ctx.needs_input_grad[3]
        band = None
        if ctx.needs_input_grad[3]:  # (the band spectrum only for the gradient w.r.t. the targets)
            y, band = ops.nfft_fastsum_band(sources, targets, x, coeffs, source_batch, target_batch, cutoff)
        else:
            y = ops.nfft_fastsum(sources, targets, x, coeffs, source_batch, target_batch, cutoff)
        if ctx.points_grad:
            ctx.save_for_backward(sources, targets, coeffs, source_batch, target_batch, x, band)
        else:
            ctx.save_for_backward(sources, targets, coeffs, source_batch, target_batch)
        ctx.cutoff = cutoff
        return y

    @staticmethod
    def backward(ctx, dy):
        sources, targets, coeffs, source_batch, target_batch = ctx.saved_tensors[:5]
        if not ctx.points_grad:
            dx = ops.nfft_fastsum(targets, sources, dy, coeffs, target_batch, source_batch, ctx.cutoff)
            return dx, None, None, None, None, None, None
        x, band = ctx.saved_tensors[5:]
        need_x, need_s, need_t = ctx.needs_input_grad[0], ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        fused_x = need_x and not coeffs.is_complex()  # real coefficients: dx and dsources share one gather
        dx, ds, dt = ops.nfft_fastsum_backward(sources, targets, x, dy.contiguous(), coeffs, band, source_batch,
                                               target_batch, ctx.cutoff, fused_x, need_s, need_t)
        if need_x and not fused_x:
            dx = ops.nfft_fastsum(targets, sources, dy, coeffs, target_batch, source_batch, ctx.cutoff)
        # (targets is sources: both gradients go to the one tensor, and autograd sums them)
        return dx if need_x else None, None, ds if need_s else None, dt if need_t else None, None, None, None


def nfft_fastsum(x, coeffs, sources, targets=None, source_batch=None, target_batch=None, /, batch=None, cutoff=3):
    """Fast multiplication with a trigonometric kernel matrix (reference: nfft.py:91-179).

    ``y = nfft_fastsum(x, coeffs, sources[, targets][, source_batch, target_batch][, batch=...][, cutoff=...])``;
    ``coeffs`` is a ``[N]*d`` tensor holding b_l at index ``l + N/2``; a real ``x`` gives a real ``y``."""
    if targets is None:
        targets = sources
        target_batch = source_batch
    if batch is not None:
        source_batch = batch
        target_batch = batch
    return NfftFastsumFunction.apply(x, coeffs, sources, targets, source_batch, target_batch, cutoff)
