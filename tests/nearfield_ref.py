"""Float64 restatement of the fast summation with a regularised kernel -- TEST INFRASTRUCTURE ONLY.

Written independently of ``torch_nfft_amd/nearfield.py``: the kernels are stated again, their derivatives at the joins come
from mpmath's numerical differentiation at 40 digits (not from autograd), the inner polynomial is solved for in the
monomials ``r^(2k)`` and the boundary polynomial in the monomials ``(r - 1/2)^k``, ``k = 0, p .. 2p-2`` (those whose
derivatives of order ``1 .. p-1`` vanish at 1/2), both by mpmath's LU at 40 digits.

``Restatement(name, c, p, eps_I, eps_B)``: ``near_poly`` (``a_k`` of ``T_I = sum a_k (r/eps_I)^(2k)``), the pieces
``kernel`` / ``inner`` / ``boundary`` and the piecewise ``K_R`` as float64 torch expressions, ``coeffs(N, dim)``.
``near_sum`` is the brute-force near field, ``dense_sum`` the direct sum ``sum K(r) x``, ``exact_algorithm`` the
trigonometric sum with the float64 coefficients of ``K_R`` plus the near sum.
"""
import mpmath
import numpy as np
import torch

from oracle import ndft

SINGULAR = ("one_over_modulus", "one_over_square", "logarithm")
NAMES = ("one_over_modulus", "one_over_square", "logarithm", "thinplate_spline", "multiquadric", "inverse_multiquadric",
         "gaussian", "laplacian_rbf")


def kernel_value(name, r, c, m):
    """K(r) with the functions of ``m`` (torch, numpy or mpmath)"""
    if name == "one_over_modulus":
        return 1 / r
    if name == "one_over_square":
        return 1 / r ** 2
    if name == "logarithm":
        return m.log(r)
    if name == "thinplate_spline":
        return r ** 2 * m.log(r)
    if name == "multiquadric":
        return m.sqrt(r ** 2 + c ** 2)
    if name == "inverse_multiquadric":
        return 1 / m.sqrt(r ** 2 + c ** 2)
    if name == "gaussian":
        return m.exp(-r ** 2 / c ** 2)
    if name == "laplacian_rbf":
        return m.exp(-r / c)
    raise KeyError(name)


def _falling(n, j):
    out = 1
    for i in range(j):
        out *= n - i
    return out


class Restatement:
    def __init__(self, name, c=1.0, p=4, eps_I=0.125, eps_B=0.0625):
        self.name, self.c, self.p, self.eps_I, self.eps_B = name, float(c), int(p), float(eps_I), float(eps_B)
        with mpmath.workdps(40):
            mc = mpmath.mpf(self.c)

            def K(r):
                return kernel_value(name, r, mc, mpmath)

            e = mpmath.mpf(self.eps_I)
            # T_I(r) = sum alpha_k r^(2k):  d^j/dr^j at eps_I equal to K^(j)(eps_I)
            A = mpmath.matrix(p, p)
            rhs = mpmath.matrix(p, 1)
            for j in range(p):
                rhs[j] = mpmath.diff(K, e, j)
                for k in range(p):
                    A[j, k] = _falling(2 * k, j) * e ** (2 * k - j) if 2 * k >= j else 0
            alpha = mpmath.lu_solve(A, rhs)
            self.near_poly = np.array([float(alpha[k] * e ** (2 * k)) for k in range(p)])
            self.left_derivatives = None
            self.bnd = None
            if self.eps_B > 0:
                left = mpmath.mpf(0.5) - mpmath.mpf(self.eps_B)
                powers = [0] + list(range(p, 2 * p - 1))
                A = mpmath.matrix(p, p)
                rhs = mpmath.matrix(p, 1)
                t = left - mpmath.mpf(0.5)
                for j in range(p):
                    rhs[j] = mpmath.diff(K, left, j)
                    for col, k in enumerate(powers):
                        A[j, col] = _falling(k, j) * t ** (k - j) if k >= j else 0
                beta = mpmath.lu_solve(A, rhs)
                self.bnd = [(k, float(beta[col])) for col, k in enumerate(powers)]

    def kernel(self, r):
        return kernel_value(self.name, r, self.c, torch)

    def inner(self, r):
        u = (r / self.eps_I) ** 2
        return sum(float(a) * u ** k for k, a in enumerate(self.near_poly))

    def boundary(self, r):
        t = r - 0.5
        return sum(b * t ** k for k, b in self.bnd)

    def __call__(self, r):
        r = torch.as_tensor(r, dtype=torch.float64)
        out = torch.empty_like(r)
        near = r < self.eps_I
        far = (r > 0.5 - self.eps_B) if self.bnd is not None else torch.zeros_like(near)
        mid = ~(near | far)
        out[near] = self.inner(r[near])
        out[mid] = self.kernel(r[mid])
        if self.bnd is not None:
            out[far] = self.boundary(r[far].clamp(max=0.5))
        return out

    def coeffs(self, N, dim):
        """b_l of the trigonometric interpolant of K_R on the grid k/N - 1/2, [N]*dim float64 (index l + N/2)"""
        ax = np.arange(N, dtype=np.float64) / N - 0.5
        r2 = np.zeros((N,) * dim)
        for a in range(dim):
            shape = [1] * dim
            shape[a] = N
            r2 = r2 + (ax * ax).reshape(shape)
        vals = self(torch.from_numpy(np.sqrt(r2))).numpy()
        b = np.fft.fftshift(np.fft.fftn(np.fft.ifftshift(vals))) / vals.size
        assert np.abs(b.imag).max() <= 1e-12 * np.abs(b.real).max()  # (even samples)
        return b.real.copy()


def _distances(sources, targets, source_batch, target_batch):
    s = np.asarray(sources, dtype=np.float64)
    t = np.asarray(targets, dtype=np.float64)
    r = np.sqrt(((t[:, None, :] - s[None, :, :]) ** 2).sum(-1))
    same = np.ones(r.shape, dtype=bool)
    if source_batch is not None:
        same = np.asarray(target_batch)[:, None] == np.asarray(source_batch)[None, :]
    return r, same


def _kernel_matrix(name, c, r):
    """K(r) elementwise in float64; at r = 0 the singular kernels give 0 (self term left out), the others K(0)"""
    zero = r == 0
    K = kernel_value(name, np.where(zero, 1.0, r), c, np)
    if name in SINGULAR or name == "thinplate_spline":
        return np.where(zero, 0.0, K)
    return np.where(zero, kernel_value(name, np.zeros(()), c, np), K)


def near_sum(name, c, near_poly, eps_I, x, sources, targets=None, source_batch=None, target_batch=None):
    """z_i = sum_{j: r_ij < eps_I, same set} (K(r_ij) - T_I(r_ij)) x_j by brute force; the pair test is made on the float32
    positions' float32 distance the way the device makes it only up to rounding -- pairs at r ~ eps_I weigh ~ 0"""
    if targets is None:
        targets, target_batch = sources, source_batch
    r, same = _distances(sources, targets, source_batch, target_batch)
    u = (r / eps_I) ** 2
    T = sum(float(a) * u ** k for k, a in enumerate(near_poly))
    W = np.where(same & (r < eps_I), _kernel_matrix(name, c, r) - T, 0.0)
    x = np.asarray(x)
    xc = x.reshape(x.shape[0], -1).astype(np.complex128 if np.iscomplexobj(x) else np.float64)
    return (W @ xc).reshape((W.shape[0],) + x.shape[1:])


def dense_sum(name, c, x, sources, targets=None, source_batch=None, target_batch=None):
    """y_i = sum_j K(|t_i - s_j|) x_j over the sources of i's point set (without coincident pairs for singular kernels)"""
    if targets is None:
        targets, target_batch = sources, source_batch
    r, same = _distances(sources, targets, source_batch, target_batch)
    W = np.where(same, _kernel_matrix(name, c, r), 0.0)
    x = np.asarray(x)
    xc = x.reshape(x.shape[0], -1).astype(np.complex128 if np.iscomplexobj(x) else np.float64)
    return (W @ xc).reshape((W.shape[0],) + x.shape[1:])


def exact_algorithm(ref, N, x, sources, targets=None, source_batch=None, target_batch=None):
    """The algorithm in exact arithmetic: the trigonometric sum with K_R's float64 coefficients + the near sum"""
    dim = np.asarray(sources).shape[1]
    far = ndft.ndft_fastsum(np.asarray(x), ref.coeffs(N, dim), np.asarray(sources), None if targets is None else np.asarray(targets),
                            source_batch, target_batch)
    return far + near_sum(ref.name, ref.c, ref.near_poly, ref.eps_I, x, sources, targets, source_batch, target_batch)


def ball_points(rng, n, dim, radius):
    """n float32 points uniform in the ball of the given radius"""
    v = rng.standard_normal((n, dim))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return (v * radius * rng.random((n, 1)) ** (1.0 / dim) * 0.999).astype(np.float32)
