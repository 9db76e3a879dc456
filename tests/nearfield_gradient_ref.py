"""Float64 restatement of the gradient of the fast summation with a regularised kernel at the targets -- TEST
INFRASTRUCTURE ONLY.  Builds on ``tests/nearfield_ref.py`` and is independent of ``torch_nfft_amd/nearfield.py``.

For ``y_i = sum_j K(|t_i - s_j|) x_j`` the field is ``G_i = sum_j K'(r_ij) (t_i - s_j) / r_ij  x_j``.

``kernel_slope``              ``K'(r) / r`` in closed form for the eight kernels
``inner_slope``               ``T_I'(r) / r = (2 / eps_I^2) sum_{k >= 1} k a_k u^(k-1)``, ``u = (r / eps_I)^2``
``near_gradient``             ``sum_{j: 0 < r_ij < eps_I} (K' - T_I')(r_ij) / r_ij  (t_i - s_j) x_j`` by brute force, ``[n_t, dim, *cols]``
``near_gradient_transpose``   its transpose applied to ``v`` ``[n_t, dim, *cols]``: ``[n_s, *cols]``
``dense_gradient``            the field of the direct sum in closed form (coincident pairs contribute zero)
``exact_algorithm_gradient``  the algorithm in exact arithmetic: the gradient of the trigonometric sum with the float64
                              coefficients of ``K_R`` (the unpaired plane ``l_a = -N/2`` of axis a zeroed) + ``near_gradient``
``exact_algorithm_gradient_transpose``  the transpose of that map applied to ``v`` ``[n_t, dim, *cols]``

The pair test is ``r < eps_I`` on the float32 positions taken to float64, as in ``nearfield_ref.near_sum``; pairs with
``r = 0`` give zero for every kernel (their difference vector is zero).
"""
import numpy as np

from oracle import ndft


def kernel_slope(name, r, c):
    """K'(r) / r for r > 0 (numpy float64)"""
    if name == "one_over_modulus":
        return -1.0 / r ** 3
    if name == "one_over_square":
        return -2.0 / r ** 4
    if name == "logarithm":
        return 1.0 / r ** 2
    if name == "thinplate_spline":
        return 2.0 * np.log(r) + 1.0
    if name == "multiquadric":
        return 1.0 / np.sqrt(r ** 2 + c ** 2)
    if name == "inverse_multiquadric":
        return -1.0 / np.sqrt(r ** 2 + c ** 2) ** 3
    if name == "gaussian":
        return -2.0 / c ** 2 * np.exp(-r ** 2 / c ** 2)
    if name == "laplacian_rbf":
        return -np.exp(-r / c) / (c * r)
    raise KeyError(name)


def inner_slope(near_poly, eps_I, r):
    """T_I'(r) / r for T_I(r) = sum_k a_k (r / eps_I)^(2k)"""
    u = (r / eps_I) ** 2
    return 2.0 / eps_I ** 2 * sum(k * float(a) * u ** (k - 1) for k, a in enumerate(near_poly) if k >= 1)


def _differences(sources, targets, source_batch, target_batch):
    s = np.asarray(sources, dtype=np.float64)
    t = np.asarray(targets, dtype=np.float64)
    d = t[:, None, :] - s[None, :, :]
    r = np.sqrt((d ** 2).sum(-1))
    same = np.ones(r.shape, dtype=bool)
    if source_batch is not None:
        same = np.asarray(target_batch)[:, None] == np.asarray(source_batch)[None, :]
    return d, r, same


def _columns(x, lead):
    x = np.asarray(x)
    return x.reshape(x.shape[:lead] + (-1,)).astype(np.complex128 if np.iscomplexobj(x) else np.float64), x.shape[lead:]


def _near_weights(name, c, near_poly, eps_I, sources, targets, source_batch, target_batch):
    """[n_t, n_s, dim]: g(r_ij) (t_i - s_j) over the pairs 0 < r_ij < eps_I of one point set"""
    d, r, same = _differences(sources, targets, source_batch, target_batch)
    pair = same & (r < eps_I) & (r > 0)
    rs = np.where(pair, r, 1.0)
    g = np.where(pair, kernel_slope(name, rs, c) - inner_slope(near_poly, eps_I, rs), 0.0)
    return g[:, :, None] * d


def near_gradient(name, c, near_poly, eps_I, x, sources, targets=None, source_batch=None, target_batch=None):
    if targets is None:
        targets, target_batch = sources, source_batch
    W = _near_weights(name, c, near_poly, eps_I, sources, targets, source_batch, target_batch)
    xc, cols = _columns(x, 1)
    return np.einsum("ija,jc->iac", W, xc).reshape(W.shape[0:1] + W.shape[2:3] + cols)


def near_gradient_transpose(name, c, near_poly, eps_I, v, sources, targets=None, source_batch=None, target_batch=None):
    if targets is None:
        targets, target_batch = sources, source_batch
    W = _near_weights(name, c, near_poly, eps_I, sources, targets, source_batch, target_batch)
    vc, cols = _columns(v, 2)
    return np.einsum("ija,iac->jc", W, vc).reshape(W.shape[1:2] + cols)


def dense_gradient(name, c, x, sources, targets=None, source_batch=None, target_batch=None):
    """G_i = sum_{j in i's point set, r_ij > 0} K'(r_ij) / r_ij (t_i - s_j) x_j"""
    if targets is None:
        targets, target_batch = sources, source_batch
    d, r, same = _differences(sources, targets, source_batch, target_batch)
    pair = same & (r > 0)
    g = np.where(pair, kernel_slope(name, np.where(pair, r, 1.0), c), 0.0)
    xc, cols = _columns(x, 1)
    return np.einsum("ija,jc->iac", g[:, :, None] * d, xc).reshape(d.shape[0:1] + d.shape[2:3] + cols)


def _slopes(coeffs, keep_nyquist):
    """[N]*dim + [dim] complex128: (-2 pi i l_a) b_l, without the unpaired plane l_a = -N/2 of axis a"""
    N, dim = coeffs.shape[0], coeffs.ndim
    freq = np.arange(-(N // 2), N // 2, dtype=np.float64)
    if not keep_nyquist:
        freq[0] = 0.0
    out = []
    for a in range(dim):
        shape = [1] * dim
        shape[a] = N
        out.append(coeffs * (-2j * np.pi * freq).reshape(shape))
    return np.stack(out, -1)


def far_gradient(coeffs, x, sources, targets=None, source_batch=None, target_batch=None, keep_nyquist=False):
    """The gradient at the targets of ndft_fastsum(x, coeffs, ...): axis a multiplies b_l by -2 pi i l_a"""
    if targets is None:
        targets, target_batch = sources, source_batch
    x = np.asarray(x)
    coeffs = np.asarray(coeffs, dtype=np.float64)
    dim = coeffs.ndim
    band = ndft.ndft_adjoint(x.reshape(x.shape[0], -1), np.asarray(sources), source_batch, N=coeffs.shape[0])  # [B, N.., C]
    band = band[..., None, :] * _slopes(coeffs, keep_nyquist)[None, ..., None]  # [B, N.., dim, C]
    G = ndft.ndft_forward(band, np.asarray(targets), target_batch).reshape((len(targets), dim) + x.shape[1:])
    return G if np.iscomplexobj(x) else G.real


def far_gradient_transpose(coeffs, v, sources, targets=None, source_batch=None, target_batch=None, keep_nyquist=False):
    """The transpose of far_gradient applied to v [n_t, dim, *cols]: sum_i sum_a sum_l (-2 pi i l_a) b_l
    e^(2 pi i l.(s_j - t_i)) v[i, a] -- the two transforms at the negated points, so that the signs of the phases swap"""
    if targets is None:
        targets, target_batch = sources, source_batch
    v = np.asarray(v)
    coeffs = np.asarray(coeffs, dtype=np.float64)
    dim = coeffs.ndim
    band = ndft.ndft_adjoint(v.reshape(v.shape[0], dim, -1), -np.asarray(targets, dtype=np.float64), target_batch,
                             N=coeffs.shape[0])  # [B, N.., dim, C]
    band = (band * _slopes(coeffs, keep_nyquist)[None, ..., None]).sum(-2)
    out = ndft.ndft_forward(band, -np.asarray(sources, dtype=np.float64), source_batch).reshape((len(sources),) + v.shape[2:])
    return out if np.iscomplexobj(v) else out.real


def exact_algorithm_gradient(ref, N, x, sources, targets=None, source_batch=None, target_batch=None, keep_nyquist=False):
    dim = np.asarray(sources).shape[1]
    far = far_gradient(ref.coeffs(N, dim), x, sources, targets, source_batch, target_batch, keep_nyquist)
    return far + near_gradient(ref.name, ref.c, ref.near_poly, ref.eps_I, x, sources, targets, source_batch, target_batch)


def exact_algorithm_gradient_transpose(ref, N, v, sources, targets=None, source_batch=None, target_batch=None):
    dim = np.asarray(sources).shape[1]
    far = far_gradient_transpose(ref.coeffs(N, dim), v, sources, targets, source_batch, target_batch)
    return far + near_gradient_transpose(ref.name, ref.c, ref.near_poly, ref.eps_I, v, sources, targets, source_batch,
                                         target_batch)
