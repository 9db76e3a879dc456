"""Float64 restatement of the gradient of the fast summation with a regularised kernel WITH RESPECT TO THE POINTS -- TEST
INFRASTRUCTURE ONLY.  Builds on ``tests/nearfield_gradient_ref.py`` (its weights ``g(r_ij) (t_i - s_j)`` and its far
gradient) and is independent of ``torch_nfft_amd/nearfield.py``.

For ``y_i = sum_j K(|t_i - s_j|) x_j`` and ``L = sum_i <dy_i, y_i>`` (the real pairing over the real columns: real and
imaginary parts of complex values are columns)

    dL/dt_i = sum_j K'(r_ij) / r_ij (t_i - s_j) <dy_i, x_j>          dL/ds_j = sum_i K'(r_ij) / r_ij (s_j - t_i) <x_j, dy_i>

``near_point_gradients``     the near part: the pairs ``0 < r_ij < eps_I`` with ``K' - T_I'`` in place of ``K'``; ``(ds, dt)``
``dense_point_gradients``    the two sums above in closed form (coincident pairs contribute zero)
``far_point_gradients``      the gradient of the trigonometric sum with the float64 coefficients of ``K_R``, the unpaired
                             planes ``l_a = -N/2`` KEPT by default: what ``nfft_fastsum`` differentiates (real x only)
``exact_algorithm_point_gradients``   far + near
``cell_offset_pairs``        the mask of the pairs whose source lies in the neighbour cell ``offset`` of the target's cell

For shared points (``targets=None``) the gradient of point k is ``ds[k] + dt[k]``.
"""
import numpy as np

import nearfield_gradient_ref as ng


def _real_columns(x):
    """[n, Cr] float64: trailing axes flattened, real and imaginary parts as columns"""
    x = np.asarray(x)
    xc = x.reshape(x.shape[0], -1)
    if np.iscomplexobj(x):
        return np.concatenate([xc.real, xc.imag], axis=1).astype(np.float64)
    return xc.astype(np.float64)


def _contract(W, x, dy):
    """W [n_t, n_s, dim] (weights times t_i - s_j) -> (ds [n_s, dim], dt [n_t, dim])"""
    S = _real_columns(dy) @ _real_columns(x).T  # [n_t, n_s]: <dy_i, x_j>
    return -np.einsum("ija,ij->ja", W, S), np.einsum("ija,ij->ia", W, S)


def cell_offset_pairs(sources, targets, G, offset):
    """[n_t, n_s] bool: the source's cell is the target's cell + offset (cells of edge 1 / (2 G) over [-1/4, 1/4]^dim)"""
    def cell(p):
        return np.clip(np.floor((np.asarray(p, dtype=np.float32) + np.float32(0.25)) * np.float32(2 * G)), 0, G - 1).astype(np.int64)
    cs, ct = cell(sources), cell(sources if targets is None else targets)
    return ((cs[None, :, :] - ct[:, None, :]) == np.asarray(offset)[None, None, :]).all(-1)


def near_point_gradients(name, c, near_poly, eps_I, x, dy, sources, targets=None, source_batch=None, target_batch=None,
                         skip=None):
    """(ds, dt) of L = <dy, near_sum(x)>; ``skip`` [n_t, n_s] bool: pairs left out (what a missed cell would do)"""
    if targets is None:
        targets, target_batch = sources, source_batch
    W = ng._near_weights(name, c, near_poly, eps_I, sources, targets, source_batch, target_batch)
    if skip is not None:
        W = np.where(skip[:, :, None], 0.0, W)
    return _contract(W, x, dy)


def dense_point_gradients(name, c, x, dy, sources, targets=None, source_batch=None, target_batch=None):
    if targets is None:
        targets, target_batch = sources, source_batch
    d, r, same = ng._differences(sources, targets, source_batch, target_batch)
    pair = same & (r > 0)
    g = np.where(pair, ng.kernel_slope(name, np.where(pair, r, 1.0), c), 0.0)
    return _contract(g[:, :, None] * d, x, dy)


def far_point_gradients(coeffs, x, dy, sources, targets=None, source_batch=None, target_batch=None, keep_nyquist=True):
    """(ds, dt) of L = <dy, Re ndft_fastsum(x, coeffs)> for real x and dy"""
    x, dy = np.asarray(x), np.asarray(dy)
    assert not np.iscomplexobj(x) and not np.iscomplexobj(dy)
    dim = np.asarray(sources).shape[1]
    xc, dyc = _real_columns(x), _real_columns(dy)
    G = ng.far_gradient(coeffs, xc, sources, targets, source_batch, target_batch, keep_nyquist)  # [n_t, dim, Cr]
    dt = np.einsum("iac,ic->ia", G, dyc)
    ds = np.zeros((len(sources), dim))
    for a in range(dim):
        v = np.zeros((len(dyc), dim, dyc.shape[1]))
        v[:, a, :] = dyc
        Gt = ng.far_gradient_transpose(coeffs, v, sources, targets, source_batch, target_batch, keep_nyquist)  # [n_s, Cr]
        ds[:, a] = -(Gt * xc).sum(1)
    return ds, dt


def exact_algorithm_point_gradients(ref, N, x, dy, sources, targets=None, source_batch=None, target_batch=None,
                                    keep_nyquist=True):
    dim = np.asarray(sources).shape[1]
    fs, ft = far_point_gradients(ref.coeffs(N, dim), x, dy, sources, targets, source_batch, target_batch, keep_nyquist)
    ns, nt = near_point_gradients(ref.name, ref.c, ref.near_poly, ref.eps_I, x, dy, sources, targets, source_batch,
                                  target_batch)
    return fs + ns, ft + nt
