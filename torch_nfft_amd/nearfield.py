"""Fast summation for kernels that are singular or too narrow for the grid: regularised far field + near field
(no reference counterpart).

``nfft_fastsum`` is exact only for kernels that are smooth on the whole torus.  Following Potts, Steidl and Nieslony
(2004; NFFT3's ``fastsum``), a kernel ``K(r)`` is replaced by ``K_R``: inside the radius ``eps_I`` by the even polynomial
``T_I(r) = sum_{k<p} a_k (r / eps_I)^(2k)`` whose derivatives of order ``0 .. p-1`` at ``eps_I`` are those of ``K``, and
on ``(1/2 - eps_B, 1/2)`` by the polynomial ``T_B`` of degree ``2p - 2`` that takes over ``K``'s derivatives at the left
end and is flat to order ``p - 1`` at ``1/2``, so that the periodic continuation is ``p - 1`` times differentiable.
``K_R`` is summed with the NFFT, and ``K - K_R = K - T_I`` is added directly over the pairs closer than ``eps_I`` -- the
near field, one native call (``ops.nfft_nearfield``).

``RegularizedKernel`` does the set-up in float64 on the host: every kernel is written once as a torch expression in ``r``
and the derivatives come from ``torch.autograd.grad`` on it.  ``nfft_fastsum_nearfield`` is the sum itself,
``nfft_fastsum_nearfield_gradient`` its gradient at the targets (the field of the potential).
"""
import math

import torch

from . import ops
from .coeffs import interpolated_kernel_coeffs
from .nfft import nfft_adjoint, nfft_fastsum, nfft_forward


# name -> (kernel id of include/nfft_hip.h, K(r, c) as a torch expression, singular at 0, c must be positive)
KERNELS = {
    "one_over_modulus": (0, lambda r, c: 1.0 / r, True, False),
    "one_over_square": (1, lambda r, c: 1.0 / (r * r), True, False),
    "logarithm": (2, lambda r, c: torch.log(r), True, False),
    "thinplate_spline": (3, lambda r, c: r * r * torch.log(r), False, False),
    "multiquadric": (4, lambda r, c: torch.sqrt(r * r + c * c), False, False),
    "inverse_multiquadric": (5, lambda r, c: 1.0 / torch.sqrt(r * r + c * c), False, True),
    "gaussian": (6, lambda r, c: torch.exp(-(r * r) / (c * c)), False, True),
    "laplacian_rbf": (7, lambda r, c: torch.exp(-r / c), False, True),
}


def _falling(n, j):
    """n (n-1) ... (n-j+1)"""
    out = 1.0
    for i in range(j):
        out *= n - i
    return out


def _horner(coeffs, t):
    out = torch.full_like(t, float(coeffs[-1]))
    for a in reversed(coeffs[:-1]):
        out = out * t + float(a)
    return out


class RegularizedKernel:
    """``K_R`` of a radial kernel and what both halves of the sum need from it.

    ``name`` is one of ``KERNELS`` (``one_over_modulus`` 1/r, ``one_over_square`` 1/r^2, ``logarithm`` log r,
    ``thinplate_spline`` r^2 log r, ``multiquadric`` sqrt(r^2 + c^2), ``inverse_multiquadric``, ``gaussian``
    exp(-r^2/c^2), ``laplacian_rbf`` exp(-r/c)); ``c`` the shape parameter where one appears.  ``p`` (1..8) is the
    smoothness of the regularisation, ``eps_I`` the near-field radius (default ``p / N``), ``eps_B`` the width of the
    boundary layer (default ``max(1/16, p / N)``; 0: no boundary piece, ``K`` is sampled as it is).

    ``coeffs``      ``[N]*dim`` float32: ``interpolated_kernel_coeffs`` of ``K_R`` on ``radial_interpolation_grid`` (real:
                    the samples are even); with ``device="cpu"`` the same recipe as a float64 FFT on the host
    ``max_radius``  ``1/4 - eps_B/2``: every source and target must lie within it
    ``near_poly``   ``a_0 .. a_{p-1}`` float64
    ``near_gradient_poly``  ``[p - 1]`` float64: ``T_I'(r) / r = sum_k near_gradient_poly[k] (r / eps_I)^(2k)``
    ``kern(r)``     ``K_R(r)`` in float64; ``kernel`` / ``inner`` / ``boundary`` are its three pieces
    """

    def __init__(self, name, c=1.0, dim=3, bandwidth=64, p=4, eps_I=None, eps_B=None, device="cuda"):
        if name not in KERNELS:
            raise ValueError("RegularizedKernel: unknown kernel %r (one of %s)" % (name, ", ".join(sorted(KERNELS))))
        self.kernel_id, self._fn, self.singular, needs_c = KERNELS[name]
        N, p = int(bandwidth), int(p)
        if dim not in (1, 2, 3):
            raise ValueError("RegularizedKernel: dim must be 1, 2 or 3")
        if N < 2 or N % 2:
            raise ValueError("RegularizedKernel: bandwidth must be even and >= 2")
        if not 1 <= p <= 8:
            raise ValueError("RegularizedKernel: p must be in 1..8")
        c = float(c)
        if not (c > 0.0 if needs_c else c >= 0.0):
            raise ValueError("RegularizedKernel: the shape parameter c must be positive")
        eps_I = p / N if eps_I is None else float(eps_I)
        eps_B = max(1.0 / 16.0, p / N) if eps_B is None else float(eps_B)
        if not eps_B >= 0.0:
            raise ValueError("RegularizedKernel: eps_B must be >= 0")
        if not 0.0 < eps_I < 0.5 - eps_B:
            raise ValueError("RegularizedKernel: eps_I must lie in (0, 1/2 - eps_B)")
        self.name, self.c, self.dim, self.bandwidth, self.p = name, c, int(dim), N, p
        self.eps_I, self.eps_B = eps_I, eps_B
        self.max_radius = 0.25 - eps_B / 2
        self.near_poly = self._inner_coefficients()
        # d/dr sum_k a_k (r / eps_I)^(2k) = r (2 / eps_I^2) sum_{k >= 1} k a_k (r / eps_I)^(2 (k - 1))
        self.near_gradient_poly = self.near_poly[1:] * torch.arange(1, p, dtype=torch.float64) * (2.0 / (eps_I * eps_I))
        self._bnd_poly = self._boundary_coefficients() if eps_B > 0.0 else None
        self.coeffs = self._coefficients(torch.device(device))

    # ---- the three pieces of K_R, float64 torch expressions -------------------------------------------------------
    def kernel(self, r):
        return self._fn(r, self.c)

    def inner(self, r):
        """T_I(r) = sum_k a_k (r / eps_I)^(2k)"""
        u = r / self.eps_I
        return _horner(self.near_poly.tolist(), u * u)

    def boundary(self, r):
        """T_B(r) on [1/2 - eps_B, 1/2], a polynomial in s = (r - (1/2 - eps_B)) / eps_B"""
        return _horner(self._bnd_poly.tolist(), (r - (0.5 - self.eps_B)) / self.eps_B)

    def __call__(self, r):
        r = torch.as_tensor(r, dtype=torch.float64)
        near = r < self.eps_I
        far = (r > 0.5 - self.eps_B) if self._bnd_poly is not None else torch.zeros_like(near)
        mid = 0.5 * (self.eps_I + 0.5 - self.eps_B)  # (keeps the unused branch of K finite)
        out = self.kernel(torch.where(near | far, torch.full_like(r, mid), r))
        out = torch.where(near, self.inner(r), out)
        if self._bnd_poly is not None:
            out = torch.where(far, self.boundary(r.clamp(max=0.5)), out)
        return out

    # ---- set-up ---------------------------------------------------------------------------------------------------
    def _scaled_derivatives(self, r0, h):
        """[h^j K^(j)(r0) for j < p] by repeated autograd on the kernel's expression"""
        r = torch.tensor(float(r0), dtype=torch.float64, requires_grad=True)
        y = self.kernel(r)
        out = []
        for j in range(self.p):
            out.append(float(y.detach()) * h ** j)
            if j + 1 < self.p:
                if not y.requires_grad:
                    out.extend([0.0] * (self.p - j - 1))
                    break
                y, = torch.autograd.grad(y, r, create_graph=True)
        return torch.tensor(out, dtype=torch.float64)

    def _inner_coefficients(self):
        # d^j/dr^j (r/eps)^(2k) at eps = falling(2k, j) / eps^j: rows scaled by eps^j
        p = self.p
        A = torch.tensor([[_falling(2 * k, j) for k in range(p)] for j in range(p)], dtype=torch.float64)
        return torch.linalg.solve(A, self._scaled_derivatives(self.eps_I, self.eps_I))

    def _boundary_coefficients(self):
        # q(s) = sum_{k <= 2p-2} b_k s^k: q^(j)(0) = eps_B^j K^(j)(1/2 - eps_B) for j < p, q^(j)(1) = 0 for 1 <= j < p
        p = self.p
        d = self._scaled_derivatives(0.5 - self.eps_B, self.eps_B)
        low = torch.tensor([float(d[j]) / math.factorial(j) for j in range(p)], dtype=torch.float64)
        if p == 1:
            return low
        A = torch.tensor([[_falling(k, j) for k in range(p, 2 * p - 1)] for j in range(1, p)], dtype=torch.float64)
        rhs = torch.tensor([-sum(float(low[k]) * _falling(k, j) for k in range(p)) for j in range(1, p)], dtype=torch.float64)
        return torch.cat([low, torch.linalg.solve(A, rhs)])

    def grid_samples(self):
        """K_R at the radii of ``radial_interpolation_grid``: |k/N - 1/2| for k in [0, N)^dim, float64 on the host"""
        N = self.bandwidth
        ax = torch.arange(N, dtype=torch.float64) / N - 0.5
        r2 = torch.zeros([N] * self.dim, dtype=torch.float64)
        for a in range(self.dim):
            shape = [1] * self.dim
            shape[a] = N
            r2 = r2 + (ax * ax).reshape(shape)
        return self(torch.sqrt(r2))

    def _coefficients(self, device):
        vals = self.grid_samples()
        if device.type == "cuda":
            with torch.cuda.device(device):
                b = interpolated_kernel_coeffs(vals.to(device=device, dtype=torch.float32))
            return b.real.contiguous()
        dims = list(range(self.dim))  # the same recipe on the host (set-up without a GPU)
        b = torch.fft.fftshift(torch.fft.fftn(torch.fft.ifftshift(vals, dim=dims), dim=dims), dim=dims) / vals.numel()
        return b.real.to(torch.float32).contiguous()


class NfftNearfieldFunction(torch.autograd.Function):
    """z = (K - T_I) restricted to pairs closer than eps_I, applied to x.  Linear in x; its transpose is itself with sources
    and targets swapped, so the backward goes through this Function and can be differentiated again."""

    @staticmethod
    def forward(ctx, x, kern, sources, targets, source_batch, target_batch):
        for name, t in (("sources", sources), ("targets", targets), ("source_batch", source_batch),
                        ("target_batch", target_batch)):
            if t is not None and t.requires_grad:
                raise AssertionError("the near field is differentiable w.r.t. x only, but %s requires grad" % name)
        ctx.kern = kern
        ctx.save_for_backward(sources, targets, source_batch, target_batch)
        return ops.nfft_nearfield(sources, targets, x, source_batch, target_batch, kern.kernel_id, kern.c, kern.eps_I,
                                  kern.near_poly.tolist())

    @staticmethod
    def backward(ctx, dz):
        sources, targets, source_batch, target_batch = ctx.saved_tensors
        dx = NfftNearfieldFunction.apply(dz, ctx.kern, targets, sources, target_batch, source_batch)
        return dx, None, None, None, None, None


class _NearfieldPointGradient(torch.autograd.Function):
    """(ds, dt) of ``ops.nfft_nearfield_point_gradient`` as a node of the graph, so that a second derivative through the
    point gradients is refused instead of being silently absent."""

    @staticmethod
    def forward(ctx, x, dz, kern, sources, targets, source_batch, target_batch, need_sources, need_targets):
        ds, dt = ops.nfft_nearfield_point_gradient(sources, targets, x, dz, source_batch, target_batch, kern.kernel_id,
                                                   kern.c, kern.eps_I, kern.near_gradient_poly.tolist(), need_sources,
                                                   need_targets)
        if not need_sources:
            ctx.mark_non_differentiable(ds)
        if not need_targets:
            ctx.mark_non_differentiable(dt)
        return ds, dt

    @staticmethod
    def backward(ctx, *grads):
        raise RuntimeError("second derivatives with respect to the near field's points are not implemented: the point "
                           "gradients of nfft_nearfield / nfft_fastsum_nearfield are first-order (differentiating them "
                           "again needs K''(r))")


class NfftNearfieldPointsFunction(torch.autograd.Function):
    """``NfftNearfieldFunction`` for points that require grad (``point_gradients=True``).  The
    forward is the same near-field call.  In the backward ``ds`` and ``dt`` come from one call of
    ``ops.nfft_nearfield_point_gradient`` (first-order: differentiating them again raises a RuntimeError), and ``dx`` is
    the near field of ``dz`` with the sides swapped -- through this Function again, so that it stays differentiable in
    ``dz`` and, to first order, in the points.  Shared points (``targets is sources``) take one symmetric sweep; the
    total arrives as the sources' gradient, zeros as the targets', and autograd adds the two."""

    @staticmethod
    def forward(ctx, x, kern, sources, targets, source_batch, target_batch):
        for name, t in (("source_batch", source_batch), ("target_batch", target_batch)):
            if t is not None and t.requires_grad:
                raise AssertionError("the near field is not differentiable w.r.t. %s" % name)
        ctx.kern = kern
        ctx.shared = targets is sources
        ctx.save_for_backward(x, sources, targets, source_batch, target_batch)
        return ops.nfft_nearfield(sources, targets, x, source_batch, target_batch, kern.kernel_id, kern.c, kern.eps_I,
                                  kern.near_poly.tolist())

    @staticmethod
    def backward(ctx, dz):
        x, sources, targets, source_batch, target_batch = ctx.saved_tensors
        if ctx.shared:
            targets = sources
        dx = ds = dt = None
        if ctx.needs_input_grad[0]:
            dx = NfftNearfieldPointsFunction.apply(dz, ctx.kern, targets, sources, target_batch, source_batch)
        need_s, need_t = ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        if need_s or need_t:
            ds, dt = _NearfieldPointGradient.apply(x, dz, ctx.kern, sources, targets, source_batch, target_batch, need_s,
                                                   need_t)
            ds, dt = (ds if need_s else None), (dt if need_t else None)
        return dx, None, ds, dt, None, None


def _near_function(what, point_gradients, kern, sources, targets, source_batch, target_batch):
    """The Function of the near field: today's unless ``point_gradients`` and a point requires grad"""
    for name, t in (("sources", sources), ("targets", targets), ("source_batch", source_batch),
                    ("target_batch", target_batch)):
        if t is None or not t.requires_grad:
            continue
        if name.endswith("_batch"):
            raise AssertionError("%s is not differentiable w.r.t. the batch vectors, but %s requires grad" % (what, name))
        if not point_gradients:
            raise AssertionError("%s is differentiable w.r.t. x only, but %s (pass point_gradients=True) requires grad"
                                 % (what, name))
    if point_gradients and (sources.requires_grad or targets.requires_grad):
        _needs_smooth_join("%s with point_gradients=True" % what, kern)
        return NfftNearfieldPointsFunction
    return NfftNearfieldFunction


def nfft_nearfield(x, kern, sources, targets=None, source_batch=None, target_batch=None, /, batch=None, *,
                   point_gradients=False):
    """``z_i = sum_{j: |t_i - s_j| < eps_I, same point set} (K(r_ij) - T_I(r_ij)) x_j``: the near field of
    ``nfft_fastsum_nearfield`` on its own (same argument conventions, ``point_gradients`` included)."""
    if targets is None:
        targets = sources
        target_batch = source_batch
    if batch is not None:
        source_batch = batch
        target_batch = batch
    fn = _near_function("the near field", point_gradients, kern, sources, targets, source_batch, target_batch)
    return fn.apply(x, kern, sources, targets, source_batch, target_batch)


def nfft_fastsum_nearfield(x, kern, sources, targets=None, source_batch=None, target_batch=None, /, batch=None, cutoff=3,
                           *, point_gradients=False):
    """Fast summation with a ``RegularizedKernel``:  ``y_i = sum_j K(|t_i - s_j|) x_j`` over the sources of target i's
    point set (for a kernel that is singular at 0 without the pairs ``s_j = t_i``), as
    ``nfft_fastsum(x, kern.coeffs, ...)`` plus the near field.

    The argument conventions are those of ``nfft_fastsum`` (``targets=None``: shared points; a real ``x`` gives a real
    ``y``), in torus coordinates: every source and target must lie within ``kern.max_radius`` of the origin (not
    checked).  Differentiable in ``x`` (the near field to any order, the far field once, like ``nfft_fastsum``).
    By default ``sources``, ``targets`` and the batch vectors must not require grad (AssertionError); the gradient at the
    targets is a function of its own, ``nfft_fastsum_nearfield_gradient``.

    ``point_gradients=True`` (keyword only) lets ``sources`` and ``targets`` require grad: the far part is
    ``nfft_fastsum``'s own gradient in the points, the near part one contracting pair sweep (one
    symmetric sweep for shared points, whose ``.grad`` then holds the sum of both roles).  It is opt-in because callers and
    tests rely on the refusal above; with no point requiring grad the result is bitwise the default's.  It needs
    ``kern.p >= 2`` (ValueError), is first-order in the points (a second derivative through them raises a RuntimeError), and
    the batch vectors still must not require grad."""
    if targets is None:
        targets = sources
        target_batch = source_batch
    if batch is not None:
        source_batch = batch
        target_batch = batch
    fn = _near_function("nfft_fastsum_nearfield", point_gradients, kern, sources, targets, source_batch, target_batch)
    far = nfft_fastsum(x, kern.coeffs, sources, targets, source_batch, target_batch, cutoff=cutoff)
    return far + fn.apply(x, kern, sources, targets, source_batch, target_batch)


def _refuse_point_gradients(what, sources, targets, source_batch, target_batch):
    for name, t in (("sources", sources), ("targets", targets), ("source_batch", source_batch),
                    ("target_batch", target_batch)):
        if t is not None and t.requires_grad:
            raise AssertionError("%s is differentiable w.r.t. x only, but %s requires grad" % (what, name))


class NfftNearfieldGradientFunction(torch.autograd.Function):
    """``transpose=False``: G = the gradient of the near field at the targets applied to x, ``[n_t, dim, *cols]``;
    ``transpose=True``: G^T applied to ``[n_t, dim, *cols]``, ``[n_s, *cols]``.  Both are linear in x and each is the
    other's backward, so either can be differentiated in x to any order."""

    @staticmethod
    def forward(ctx, x, kern, sources, targets, source_batch, target_batch, transpose):
        _refuse_point_gradients("the near field's gradient", sources, targets, source_batch, target_batch)
        ctx.kern, ctx.transpose = kern, transpose
        ctx.save_for_backward(sources, targets, source_batch, target_batch)
        return ops.nfft_nearfield_gradient(sources, targets, x, source_batch, target_batch, kern.kernel_id, kern.c,
                                           kern.eps_I, kern.near_gradient_poly.tolist(), transpose)

    @staticmethod
    def backward(ctx, dz):
        sources, targets, source_batch, target_batch = ctx.saved_tensors
        dx = NfftNearfieldGradientFunction.apply(dz, ctx.kern, sources, targets, source_batch, target_batch,
                                                 not ctx.transpose)
        return dx, None, None, None, None, None, None


def _needs_smooth_join(what, kern):
    if kern.p < 2:
        raise ValueError("%s needs a RegularizedKernel with p >= 2: with p = 1 K_R is only continuous at eps_I" % what)


def nfft_nearfield_gradient(x, kern, sources, targets=None, source_batch=None, target_batch=None, /, batch=None):
    """``G_i = sum_{j: 0 < |t_i - s_j| < eps_I, same point set} (K'(r_ij) - T_I'(r_ij)) (t_i - s_j) / r_ij  x_j``,
    ``[n_t, dim, *cols]``: the gradient of ``nfft_nearfield`` at the targets, the near part of
    ``nfft_fastsum_nearfield_gradient`` on its own (same argument conventions; a pair with ``r = 0`` contributes zero)."""
    _needs_smooth_join("nfft_nearfield_gradient", kern)
    if targets is None:
        targets = sources
        target_batch = source_batch
    if batch is not None:
        source_batch = batch
        target_batch = batch
    return NfftNearfieldGradientFunction.apply(x, kern, sources, targets, source_batch, target_batch, False)


def _far_gradient_coeffs(kern):
    """``[N]*dim + [dim]`` complex64: ``(-2 pi i l_a) kern.coeffs`` for every axis a, the unpaired plane ``l_a = -N/2`` of
    axis a zeroed (the derivative of a real trigonometric interpolant has no Nyquist term)"""
    N, dim = kern.bandwidth, kern.dim
    freq = torch.arange(-(N // 2), N // 2, dtype=torch.float32, device=kern.coeffs.device)
    freq[0] = 0.0
    out = []
    for a in range(dim):
        shape = [1] * dim
        shape[a] = N
        out.append(torch.complex(torch.zeros_like(kern.coeffs), kern.coeffs * (-2.0 * math.pi * freq).reshape(shape)))
    return torch.stack(out, dim)


def _far_gradient(x, kern, sources, targets, source_batch, target_batch, cutoff):
    """forward_t(c' * adjoint_s(x)) with the dim gradient coefficient arrays as further columns: [n_t, dim, *cols]"""
    N, dim = kern.bandwidth, kern.dim
    band = nfft_adjoint(x, sources, source_batch, bandwidth=N, cutoff=cutoff)  # [B] + [N]*dim + cols
    band = band.unsqueeze(1 + dim) * _far_gradient_coeffs(kern).reshape([1] + [N] * dim + [dim] + [1] * (x.dim() - 1))
    return nfft_forward(band, targets, target_batch, cutoff=cutoff, real_output=not x.is_complex())


def nfft_fastsum_nearfield_gradient(x, kern, sources, targets=None, source_batch=None, target_batch=None, /, batch=None,
                                    cutoff=3):
    """The field of ``nfft_fastsum_nearfield``'s potential: ``G_i = grad_{t_i} y_i = sum_j K'(r_ij) (t_i - s_j) / r_ij  x_j``
    over the sources of target i's point set, ``[n_t, dim, *cols]`` with the dtype of ``x``.

    The far part is the gradient of the trigonometric polynomial of ``K_R``: ``nfft_forward`` at the targets of
    ``nfft_adjoint(x)`` at the sources times ``(-2 pi i l_a) kern.coeffs``, the ``dim`` axes as further columns; the near
    part is ``nfft_nearfield_gradient``.  Arguments as for ``nfft_fastsum_nearfield``; ``kern.p >= 2`` (ValueError).
    Differentiable in ``x`` (the near part to any order, the far part as far as the two transforms are); ``sources``,
    ``targets`` and the batch vectors must not require grad (AssertionError)."""
    _needs_smooth_join("nfft_fastsum_nearfield_gradient", kern)
    if targets is None:
        targets = sources
        target_batch = source_batch
    if batch is not None:
        source_batch = batch
        target_batch = batch
    _refuse_point_gradients("nfft_fastsum_nearfield_gradient", sources, targets, source_batch, target_batch)
    far = _far_gradient(x, kern, sources, targets, source_batch, target_batch, cutoff)
    return far + NfftNearfieldGradientFunction.apply(x, kern, sources, targets, source_batch, target_batch, False)
