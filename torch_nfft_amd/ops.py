"""Operator layer: thin Python names for the native ``torch.ops.torch_nfft.*`` operators.

The eight operators of the reference (``csrc/core.cpp:43-121, 176-184``: names, positional argument order
``(pos, x, batch, ...)``, error messages, the input checks of ``csrc/cuda/core_cuda.cu:38-115``) are registered
from C++ by ``core.so`` (``csrc/core.cpp`` of this package), which the package ``__init__`` loads with
``torch.ops.load_library`` exactly like the reference's ``torch_nfft/__init__.py:11``.  This module only gives
them Python names, adds the ``device=`` convenience of the coefficient helpers and exposes the point-plan cache
controls.  All arithmetic happens in ``libnfft_hip.so`` behind the C ABI of ``include/nfft_hip.h``.

Point-plan reuse.  The tile-sorted copy of the points depends only on
``(pos, batch, N, m)``; adjoint <-> forward pairs on the same points (autograd backward, a forward fed by an
adjoint, fastsum) reuse it instead of re-binning.  The cache lives in ``core.so``: two entries, keyed on tensor
identity + version counter, stream-aware (a plan built on one stream is waited for and recorded on the consuming
stream).  Writes that bypass the version counter -- ``pos.data.copy_()``, kernels of other libraries, DLPack aliases --
are invisible to the KEY, so every plan carries a checksum of the ``pos`` / ``batch`` it was built from and every hit
re-checks it (one streaming pass, ~25 us for 10^7 points): a stale plan raises "stale point plan" at the next operator or
``check_status()`` instead of returning a transform of points that are no longer there (``plan_cache_verify(False)`` for
callers who never write that way).  The same switches govern the remembered ENDS of the batch vector
(``B = batch[-1] + 1`` otherwise costs a blocking read-back of ~35 us in every operator call, as in the reference's
``check_point_input``, core_cuda.cu:60): same key (identity + version counter), same limitation.

Not in the reference, for gradients with respect to the points: ``nfft_forward_grad_points`` (both transforms) and its
backward ``nfft_forward_grad_points_backward`` (their second derivatives), ``nfft_fastsum_band``
and ``nfft_fastsum_backward`` (the fast summation).  They take their plans
from the same cache with the same problems, so a backward pass right after its forward pass plans nothing.
``nfft_toeplitz_kernel`` and ``nfft_normal`` (the normal operator ``A^H W A`` as a Toeplitz product)
use no plan at all.  ``nfft_nearfield`` (the near-field pair sum of the fast summation for singular kernels; DESIGN.md
section 7d) orders the points by cells of its own and uses no plan either.
"""
import torch

_ops = torch.ops.torch_nfft


def plan_cache_enabled(flag):
    _ops._plan_cache(1 if flag else 2)


def plan_cache_clear():
    _ops._plan_cache(0)


def plan_cache_verify(flag):
    """Verify a cached plan's seal (the checksum of the points it was built from) on every hit (default on)."""
    _ops._plan_cache(5 if flag else 6)


def plan_cache_stats():
    return {"hits": int(_ops._plan_cache(3)), "misses": int(_ops._plan_cache(4))}


def check_status(synchronize=True):
    """Raises ``RuntimeError`` if a kernel on the current device has reported a fault since the last look (a bounded
    wait of the streamed interpolation kernel ran out; a batch index outside ``[0, B)``).  The operators are
    asynchronous, so such a fault otherwise surfaces in the NEXT operator call on the device; with ``synchronize``
    (default) the current stream is drained first and the work enqueued so far is covered.  The reference aborts the
    process on a device error (``csrc/cuda/cuda_utils.cu:5-16``)."""
    _ops._check_status(1 if synchronize else 0)


def nfft_adjoint(pos, x, batch, N, m, real_output):
    """torch_nfft::nfft_adjoint(Tensor pos, Tensor x, Tensor? batch, int N, int m, int real_output) -> Tensor
    (csrc/core.cpp:43-55; driver core_cuda.cu:144-336)."""
    return _ops.nfft_adjoint(pos, x, batch, int(N), int(m), 1 if real_output else 0)


def nfft_forward(pos, x, batch, m, real_output):
    """torch_nfft::nfft_forward(Tensor pos, Tensor x, Tensor? batch, int m, int real_output) -> Tensor
    (csrc/core.cpp:94-105; driver core_cuda.cu:340-531)."""
    return _ops.nfft_forward(pos, x, batch, int(m), 1 if real_output else 0)


def nfft_forward_grad_points(pos, x, batch, m, real_output, w):
    """torch_nfft::_nfft_forward_grad_points(Tensor pos, Tensor x, Tensor? batch, int m, int real_output, Tensor w)
    -> Tensor [n, dim] (not in the reference): ``dpos[i, a] = sum_cr w[i, cr] d Fr[i, cr] / d pos[i, a]``, where ``Fr``
    are the real columns of ``nfft_forward(pos, x, batch, m, real_output)`` (``2 C`` interleaved re / im without
    ``real_output``) and ``w`` is ``[n, Cr]`` float32.  One native call (``nfft_hip_forward_grad_points_planned``) on the
    cached point plan."""
    return _ops._nfft_forward_grad_points(pos, x, batch, int(m), 1 if real_output else 0, w)


def nfft_forward_grad_points_backward(pos, x, batch, m, real_output, w, v, need_xhat, need_w, need_pos):
    """torch_nfft::_nfft_forward_grad_points_backward(Tensor pos, Tensor xhat, Tensor? batch, int m, int real_output,
    Tensor w, Tensor v, int need_xhat, int need_w, int need_pos) -> (Tensor dxhat, Tensor dw, Tensor dpos) (not in the
    reference): the gradients of ``<v, nfft_forward_grad_points(pos, x, batch, m, real_output, w)>`` for ``v`` [n, dim]
    float32 -- ``dxhat`` like ``x``, ``dw`` [n, Cr], ``dpos`` [n, dim]; what was not asked for comes back empty.  One native
    call (``nfft_hip_forward_grad_points_backward_planned``) on the cached point plan."""
    return _ops._nfft_forward_grad_points_backward(pos, x, batch, int(m), 1 if real_output else 0, w, v,
                                                   1 if need_xhat else 0, 1 if need_w else 0, 1 if need_pos else 0)


def nfft_fastsum(sources, targets, x, coeffs, source_batch, target_batch, m):
    """torch_nfft::nfft_fastsum(Tensor sources, Tensor targets, Tensor x, Tensor coeffs, Tensor? source_batch,
    Tensor? target_batch, int m) -> Tensor   (csrc/core.cpp:108-121; driver core_cuda.cu:535-852).
    One native call (``nfft_hip_fastsum_planned``): adjoint at the sources with the kernel coefficients folded
    into its last spectral pass, forward at the targets; shared points share one plan (core_cuda.cu:552-564)."""
    return _ops.nfft_fastsum(sources, targets, x, coeffs, source_batch, target_batch, int(m))


def nfft_fastsum_band(sources, targets, x, coeffs, source_batch, target_batch, m):
    """torch_nfft::_nfft_fastsum_band(...same arguments as nfft_fastsum...) -> (Tensor y, Tensor band) (not in the
    reference): ``nfft_fastsum`` (same route, bitwise the same ``y``) that also returns its band spectrum
    ``coeffs * A_s(x)``, ``[B] + [N]*d + x.shape[1:]`` complex64 -- what ``nfft_fastsum_backward`` needs for the targets'
    gradient.  One native call (``nfft_hip_fastsum_band[_planned]``)."""
    return _ops._nfft_fastsum_band(sources, targets, x, coeffs, source_batch, target_batch, int(m))


def nfft_fastsum_backward(sources, targets, x, dy, coeffs, band, source_batch, target_batch, m, need_x, need_sources,
                          need_targets):
    """torch_nfft::_nfft_fastsum_backward(Tensor sources, Tensor targets, Tensor x, Tensor dy, Tensor coeffs,
    Tensor? band, Tensor? source_batch, Tensor? target_batch, int m, int need_x, int need_sources, int need_targets)
    -> (Tensor dx, Tensor dsources, Tensor dtargets) (not in the reference): the gradients of ``nfft_fastsum`` for the
    upstream gradient ``dy``; what was not asked for comes back empty.  ``dx`` only for real ``coeffs`` (it comes from the
    same gather as ``dsources``); ``band`` from ``nfft_fastsum_band`` when ``need_targets``.  One native call
    (``nfft_hip_fastsum_backward_planned``) on the point plans the forward pass cached."""
    return _ops._nfft_fastsum_backward(sources, targets, x, dy, coeffs, band, source_batch, target_batch, int(m),
                                       1 if need_x else 0, 1 if need_sources else 0, 1 if need_targets else 0)


def nfft_toeplitz_kernel(t):
    """torch_nfft::_nfft_toeplitz_kernel(Tensor t) -> Tensor (not in the reference): the real kernel grid ``K``
    ``[B, 2N, ..., 2N]`` float32 of the normal operator ``A^H W A`` from ``t = nfft_adjoint(weights, bandwidth 2N)``
    ``[B, 2N, ..., 2N]`` complex64 (lag ``n`` at index ``n + N``).  One native call (``nfft_hip_toeplitz_kernel``;
    DESIGN.md section 7c)."""
    return _ops._nfft_toeplitz_kernel(t)


def nfft_normal(kernel, x):
    """torch_nfft::_nfft_normal(Tensor kernel, Tensor x) -> Tensor (not in the reference): ``A^H W A x`` for ``x``
    ``[B] + [N]*d + cols`` float32 or complex64 and the kernel grid of the same points; complex64.  One native call
    (``nfft_hip_toeplitz_apply``): forward FFT stage, product with ``kernel``, adjoint FFT stage -- no point plan."""
    return _ops._nfft_normal(kernel, x)


def nfft_nearfield(sources, targets, x, source_batch, target_batch, kernel, c, eps_I, poly):
    """torch_nfft::_nfft_nearfield(Tensor sources, Tensor targets, Tensor x, Tensor? source_batch, Tensor? target_batch,
    int kernel, float c, float eps_I, float[] poly) -> Tensor (not in the reference): the near field of the fast summation
    for singular kernels, ``z_i = sum_{j: |t_i - s_j| < eps_I} (K(r_ij) - T_I(r_ij)) x_j`` over the sources of target i's
    point set, with ``K`` the kernel number ``kernel`` of include/nfft_hip.h (shape parameter ``c``) and
    ``T_I(r) = sum_k poly[k] (r / eps_I)^(2k)``.  ``z`` has ``x``'s type and trailing shape.  Both point sets are ordered
    by cell with torch on the device (one stable sort each, one for shared points; no read-back), the pair sum is one
    native call (``nfft_hip_nearfield``)."""
    return _ops._nfft_nearfield(sources, targets, x, source_batch, target_batch, int(kernel), float(c), float(eps_I),
                                [float(a) for a in poly])


def nfft_nearfield_gradient(sources, targets, x, source_batch, target_batch, kernel, c, eps_I, poly, transpose):
    """torch_nfft::_nfft_nearfield_gradient(Tensor sources, Tensor targets, Tensor x, Tensor? source_batch,
    Tensor? target_batch, int kernel, float c, float eps_I, float[] poly, bool transpose) -> Tensor (not in the reference):
    the gradient of ``nfft_nearfield`` at the targets, ``G_i = sum_{j: 0 < r_ij < eps_I} g(r_ij^2) (t_i - s_j) x_j`` with
    ``g(r^2) = (K'(r) - T_I'(r)) / r`` and ``T_I'(r) / r = sum_k poly[k] (r / eps_I)^(2k)`` (``p - 1`` coefficients:
    ``RegularizedKernel.near_gradient_poly``).  ``transpose=False``: ``x`` ``[n_s, *cols]`` gives ``[n_t, dim, *cols]``;
    ``transpose=True``: ``x`` ``[n_t, dim, *cols]`` gives ``[n_s, *cols]``, ``sum_i g(r_ij^2) (t_i - s_j) . x_i``.  Cell
    ordering as for ``nfft_nearfield``; the pair sum is one native call (``nfft_hip_nearfield_gradient``; DESIGN.md section
    7e)."""
    return _ops._nfft_nearfield_gradient(sources, targets, x, source_batch, target_batch, int(kernel), float(c),
                                         float(eps_I), [float(a) for a in poly], bool(transpose))


def nfft_nearfield_point_gradient(sources, targets, x, dy, source_batch, target_batch, kernel, c, eps_I, poly, need_sources,
                                  need_targets):
    """torch_nfft::_nfft_nearfield_point_gradient(Tensor sources, Tensor targets, Tensor x, Tensor dy, Tensor? source_batch,
    Tensor? target_batch, int kernel, float c, float eps_I, float[] poly, bool need_sources, bool need_targets) ->
    (Tensor, Tensor) (not in the reference): the gradient of ``<dy, nfft_nearfield(x)>`` with respect to the points,
    ``ds[j] = sum_i g(r_ij^2) (s_j - t_i) (x_j . dy_i)`` ``[n_s, dim]`` and ``dt[i] = sum_j g(r_ij^2) (t_i - s_j) (dy_i . x_j)``
    ``[n_t, dim]`` over the pairs ``0 < r_ij < eps_I`` of one point set, ``g`` and ``poly`` as for
    ``nfft_nearfield_gradient``; the dot products run over the real columns (real and imaginary parts of complex values).
    A side that is not needed comes back empty.  Shared points (``targets`` is ``sources``, the same batch vector) with
    both sides needed take one symmetric sweep: ``ds`` is the total and ``dt`` zeros.  One native call per sweep
    (``nfft_hip_nearfield_point_gradient``)."""
    return _ops._nfft_nearfield_point_gradient(sources, targets, x, dy, source_batch, target_batch, int(kernel), float(c),
                                               float(eps_I), [float(a) for a in poly], bool(need_sources),
                                               bool(need_targets))


def nfft_ewald_near(pos, x, batch, alpha, r_cut, with_field):
    """torch_nfft::_nfft_ewald_near(Tensor pos, Tensor x, Tensor? batch, float alpha, float r_cut, bool with_field) ->
    (Tensor, Tensor) (not in the reference): the near part of the Ewald sum on the unit torus,
    ``z_i = sum_{j: 0 < r_ij < r_cut} erfc(alpha r_ij) / r_ij x_j`` over the points of i's point set with ``r_ij`` the
    length of the minimum image ``d_ij`` of ``pos_i - pos_j`` (``pos`` ``[n, 3]``, taken modulo 1), and with
    ``with_field`` ``f_i = -sum_j g(r_ij^2) d_ij x_j`` ``[n, 3, *cols]``, ``g = K'(r) / r`` of ``K = erfc(alpha r) / r``
    (empty otherwise).  ``x`` ``[n, *cols]`` float32 or complex64.  One native call (``nfft_hip_ewald_near``; DESIGN.md
    section 7g)."""
    return _ops._nfft_ewald_near(pos, x, batch, float(alpha), float(r_cut), bool(with_field))


def nfft_ewald_near_box(pos, x, batch, box, alpha, r_cut, with_field):
    """torch_nfft::_nfft_ewald_near_box(Tensor pos, Tensor x, Tensor? batch, float[] box, float alpha, float r_cut,
    bool with_field) -> (Tensor, Tensor) (not in the reference): ``nfft_ewald_near`` in the box whose lower-triangular
    matrix ``A`` (rows = lattice vectors) is ``box = (A00, A10, A11, A20, A21, A22)``.  ``pos`` ``[n, 3]`` holds FRACTIONAL
    coordinates, taken modulo 1; ``r_ij`` is the length of ``d_ij = (ds - rint(ds)) A``, ``ds = pos_i - pos_j``, so ``alpha``,
    ``r_cut`` (at most a third of the box's smallest perpendicular width), ``z`` and the Cartesian ``f`` are in the box's
    own units.  One native call (``nfft_hip_ewald_near_box``)."""
    return _ops._nfft_ewald_near_box(pos, x, batch, [float(a) for a in box], float(alpha), float(r_cut), bool(with_field))


def nfft_ewald_dispersion_near(pos, x, batch, alpha, r_cut, with_field):
    """torch_nfft::_nfft_ewald_dispersion_near(Tensor pos, Tensor x, Tensor? batch, float alpha, float r_cut,
    bool with_field) -> (Tensor, Tensor) (not in the reference): the near part of the dispersion Ewald sum on the unit
    torus, ``z_i = sum_{j: 0 < r_ij < r_cut} w(r_ij) x_j`` with ``w(r) = e^(-a^2) (1 + a^2 + a^4 / 2) / r^6``,
    ``a = alpha r``, and with ``with_field`` ``f_i = sum_j mg(r_ij) d_ij x_j`` ``[n, 3, *cols]``,
    ``mg = -w'(r) / r = e^(-a^2) (6 + 6 a^2 + 3 a^4 + a^6) / r^8`` (empty otherwise).  Points, point sets, shapes and
    types as for ``nfft_ewald_near``.  One native call (``nfft_hip_ewald_dispersion_near``)."""
    return _ops._nfft_ewald_dispersion_near(pos, x, batch, float(alpha), float(r_cut), bool(with_field))


def nfft_ewald_dispersion_near_box(pos, x, batch, box, alpha, r_cut, with_field):
    """torch_nfft::_nfft_ewald_dispersion_near_box(Tensor pos, Tensor x, Tensor? batch, float[] box, float alpha,
    float r_cut, bool with_field) -> (Tensor, Tensor) (not in the reference): ``nfft_ewald_dispersion_near`` in the box
    ``box = (A00, A10, A11, A20, A21, A22)`` on FRACTIONAL positions, as ``nfft_ewald_near_box``.  One native call
    (``nfft_hip_ewald_dispersion_near_box``)."""
    return _ops._nfft_ewald_dispersion_near_box(pos, x, batch, [float(a) for a in box], float(alpha), float(r_cut),
                                                bool(with_field))


def nfft_ewald_virial_near(pos, x, batch, box, alpha, r_cut):
    """torch_nfft::_nfft_ewald_virial_near(Tensor pos, Tensor x, Tensor? batch, float[] box, float alpha, float r_cut) ->
    Tensor (not in the reference): the pair part of the Ewald energy and of the virial tensor ``W_ab = -dU / d eps_ab``,
    ``[B, 7, *cols]`` float64 in the order energy, xx, yy, zz, yz, xz, xy::

        out[b, 0] = 1/2 sum_{i in set b} x_i sum_{j: 0 < r_ij < r_cut} erfc(alpha r_ij) / r_ij  x_j
        out[b, e] = 1/2 sum_i x_i sum_j (-g(r_ij^2)) d_ij[a] d_ij[b] x_j

    ``pos`` fractional (any real values, taken modulo 1), ``x`` ``[n, *cols]`` float32 (real charges only), ``box`` the six
    numbers of ``nfft_ewald_near_box`` (the unit cube: ``1, 0, 1, 0, 0, 1``).  One native call
    (``nfft_hip_ewald_virial_near``), no atomics: two calls give the same bits."""
    return _ops._nfft_ewald_virial_near(pos, x, batch, [float(a) for a in box], float(alpha), float(r_cut))


def nfft_ewald_virial_far(band, coeffs, box, alpha):
    """torch_nfft::_nfft_ewald_virial_far(Tensor band, Tensor coeffs, float[] box, float alpha) -> Tensor (not in the
    reference): the spectral part of the same, ``[B, 7, *cols]`` float64, from ``band`` ``[B, N, N, N, *cols]`` complex64
    (``nfft_adjoint`` of the charges) and the splitting's ``coeffs`` ``[N, N, N]`` float32::

        out[b, 0] = 1/2 sum_k b_k |band_k|^2
        out[b, e] = 1/2 sum_k b_k |band_k|^2 (delta_ab - 2 (1 / |kappa|^2 + pi^2 / alpha^2) kappa_a kappa_b),  kappa = A^-1 k

    One native call (``nfft_hip_ewald_virial_far``), one pass over ``band``, no atomics."""
    return _ops._nfft_ewald_virial_far(band, coeffs, [float(a) for a in box], float(alpha))


def nfft_ewald_step_near(pos, x, batch, box, alpha, r_cut):
    """torch_nfft::_nfft_ewald_step_near(Tensor pos, Tensor x, Tensor? batch, float[] box, float alpha, float r_cut) ->
    (Tensor, Tensor, Tensor) (not in the reference): ``(z, f, seven)`` -- ``z`` ``[n, *cols]`` and ``f`` ``[n, 3, *cols]``
    float32 of ``nfft_ewald_near_box(..., with_field=True)`` and ``seven`` ``[B, 7, *cols]`` float64 of
    ``nfft_ewald_virial_near`` -- from one walk over the pairs that keeps the ten sums of a point and column side by side.
    ``pos`` fractional (any real values, taken modulo 1), ``x`` float32 (real charges only), ``box`` six numbers (the unit
    cube: ``1, 0, 1, 0, 0, 1``).  One native call (``nfft_hip_ewald_step_near``), no atomics: two
    calls give the same bits."""
    return _ops._nfft_ewald_step_near(pos, x, batch, [float(a) for a in box], float(alpha), float(r_cut))


def nfft_ewald_step_spectral(band, coeffs, box, alpha):
    """torch_nfft::_nfft_ewald_step_spectral(Tensor band, Tensor coeffs, float[] box, float alpha) -> (Tensor, Tensor) (not
    in the reference): ``(spectra, seven)`` from one pass over ``band`` ``[B, N, N, N, *cols]`` complex64 -- ``spectra``
    ``[B, N, N, N, 4, *cols]`` complex64, ``band`` times ``b_k`` and ``(2 pi i kappa_a) b_k`` (what the product with
    ``EwaldSplitting.field_coeffs()`` gives; ``2 pi kappa`` formed in float32 from ``box``), whose forward transform is the far
    part of ``(phi, E)``, and ``seven`` ``[B, 7, *cols]`` float64 of ``nfft_ewald_virial_far``.  One native call
    (``nfft_hip_ewald_step_spectral``), no atomics."""
    return _ops._nfft_ewald_step_spectral(band, coeffs, [float(a) for a in box], float(alpha))


def nfft_ewald_lj_step_near(pos, xs, batch, box, alpha_coulomb, alpha_dispersion, r_cut):
    """torch_nfft::_nfft_ewald_lj_step_near(Tensor pos, Tensor xs, Tensor? batch, float[] box, float alpha_coulomb,
    float alpha_dispersion, float r_cut) -> (Tensor, Tensor) (not in the reference): ``(f, eight)`` of a Lennard-Jones +
    Coulomb model from one walk over the pairs ``0 < r_ij < r_cut``.  ``xs`` ``[n, 3]`` float32 holds ``(q, c, a)`` per point
    (``C6_ij = c_i c_j``, ``C12_ij = a_i a_j``).  ``f`` ``[n, 3]`` float32 is the pair part of the force,
    ``sum_j (q_i q_j mg_C - c_i c_j mg_D + 12 a_i a_j / r^14) d_ij``; ``eight`` ``[B, 8]`` float64 is ``1/2 sum q_i q_j w_C``,
    ``1/2 sum (a_i a_j / r^12 - c_i c_j w_D)`` and the six virial terms ``xx, yy, zz, yz, xz, xy`` of the same pair sum.
    ``pos`` fractional (any real values, taken modulo 1), ``box`` six numbers (the unit cube: ``1, 0, 1, 0, 0, 1``).  One native
    call (``nfft_hip_ewald_lj_step_near``), no atomics: two calls give the same bits."""
    return _ops._nfft_ewald_lj_step_near(pos, xs, batch, [float(a) for a in box], float(alpha_coulomb), float(alpha_dispersion),
                                         float(r_cut))


def nfft_ewald_lj_step_spectral(band, coeffs_coulomb, coeffs_dispersion, strain_dispersion, box, alpha_coulomb):
    """torch_nfft::_nfft_ewald_lj_step_spectral(Tensor band, Tensor coeffs_coulomb, Tensor coeffs_dispersion,
    Tensor strain_dispersion, float[] box, float alpha_coulomb) -> (Tensor, Tensor) (not in the reference): ``(spectra,
    eight)`` from one pass over ``band`` ``[B, N, N, N, 2]`` complex64, the adjoint transform of the columns ``(q, c)`` --
    ``spectra`` ``[B, N, N, N, 6]`` complex64, ``(2 pi i kappa_a) b^C_k band[.., 0]`` and ``(2 pi i kappa_a) b^D_k band[.., 1]``
    (zeros where the table is zero), whose forward transform is the far part of ``(E, G)``, and ``eight`` ``[B, 8]`` float64:
    ``1/2 sum b^C |S^q|^2``, ``-1/2 sum b^D |S^c|^2`` and the six virial terms of ``nfft_ewald_virial_far`` minus those of
    ``nfft_ewald_dispersion_virial_far``.  The three tables are ``EwaldSplitting.coeffs``, ``DispersionSplitting.coeffs`` and
    ``DispersionSplitting.strain_coeffs()``.  One native call (``nfft_hip_ewald_lj_step_spectral``), no
    atomics."""
    return _ops._nfft_ewald_lj_step_spectral(band, coeffs_coulomb, coeffs_dispersion, strain_dispersion, [float(a) for a in box],
                                             float(alpha_coulomb))


def nfft_ewald_lj_excl_near(pos, xs, batch, row_start, col, weight_coulomb, weight_lj, box, alpha_coulomb, alpha_dispersion, r_cut):
    """torch_nfft::_nfft_ewald_lj_excl_near(Tensor pos, Tensor xs, Tensor? batch, Tensor row_start, Tensor col,
    Tensor weight_coulomb, Tensor weight_lj, float[] box, float alpha_coulomb, float alpha_dispersion, float r_cut) ->
    (Tensor, Tensor) (not in the reference): ``(f, eight)`` of ``nfft_ewald_lj_step_near`` with the terms of the listed pairs
    scaled BEFORE they are added -- ``q_i q_j`` by ``s^C = 1 - weight_coulomb``, ``c_i c_j`` and ``a_i a_j`` by
    ``s^L = 1 - weight_lj``; a pair with both scales zero adds nothing.  ``row_start`` ``[n + 1]`` int32, ``col`` ``[2 m]`` int32
    and the weights ``[2 m]`` float32 are an ``ExclusionList``'s.  With an empty list the bits of ``nfft_ewald_lj_step_near``.
    One native call (``nfft_hip_ewald_lj_excl_near``), no atomics: two calls give the same bits."""
    return _ops._nfft_ewald_lj_excl_near(pos, xs, batch, row_start, col, weight_coulomb, weight_lj, [float(a) for a in box],
                                         float(alpha_coulomb), float(alpha_dispersion), float(r_cut))


def nfft_ewald_lj_excl_list(pos, xs, batch, row_start, col, weight_coulomb, weight_lj, box, alpha_coulomb, alpha_dispersion, r_cut):
    """torch_nfft::_nfft_ewald_lj_excl_list(Tensor pos, Tensor xs, Tensor? batch, Tensor row_start, Tensor col,
    Tensor weight_coulomb, Tensor weight_lj, float[] box, float alpha_coulomb, float alpha_dispersion, float r_cut) ->
    (Tensor, Tensor) (not in the reference): ``(f, eight)`` to ADD to those of ``nfft_ewald_lj_excl_near`` -- minus the share of
    the listed pairs that the far field holds (``r < r_cut``, ``r = 0`` included: ``w^C q_i q_j erf(alpha_C r) / r`` and
    ``-w^L c_i c_j (1 / r^6 - w_D)``, with their slopes) or, beyond the cut, their whole ``1 / r`` and ``1 / r^6`` terms.
    ``f`` ``[n, 3]`` float32 in row order, ``eight`` ``[B, 8]`` float64 with each pair once.  Bounded values only.  One native
    call (``nfft_hip_ewald_lj_excl_list``), no atomics: two calls give the same bits."""
    return _ops._nfft_ewald_lj_excl_list(pos, xs, batch, row_start, col, weight_coulomb, weight_lj, [float(a) for a in box],
                                         float(alpha_coulomb), float(alpha_dispersion), float(r_cut))


def nfft_ewald_lj_table_near(pos, xs, types, table, batch, row_start, col, weight_coulomb, weight_lj, box, alpha_coulomb,
                             alpha_dispersion, r_cut):
    """torch_nfft::_nfft_ewald_lj_table_near(Tensor pos, Tensor xs, Tensor types, Tensor table, Tensor? batch,
    Tensor? row_start, Tensor? col, Tensor? weight_coulomb, Tensor? weight_lj, float[] box, float alpha_coulomb,
    float alpha_dispersion, float r_cut) -> (Tensor, Tensor) (not in the reference): ``(f, eight)`` of
    ``nfft_ewald_lj_step_near`` with per-type-pair parameters.  ``xs`` ``[n, 2]`` float32 holds ``(q, c)`` with ``c`` the
    coefficient that the grid sees, ``types`` ``[n]`` int32 the points' types and ``table`` ``[T, T, 2]`` float32
    ``(C12, dC6)`` per pair of types, ``1 <= T <= 32``, with ``dC6 = C6 - c_i c_j``: the pair slope is ``q_i q_j mg_C -
    c_i c_j mg_D + 12 C12 / r^14 - 6 dC6 / r^8`` and the second energy ``1/2 sum (C12 / r^12 - dC6 / r^6 - c_i c_j w_D)``.  A type
    outside ``[0, T)`` is clamped.  The four list tensors are an ``ExclusionList``'s, all of them or all ``None``; with them
    ``q_i q_j`` of a listed pair is scaled by ``s^C`` and ``c_i c_j``, ``C12``, ``dC6`` by ``s^L`` before they are added, and an
    empty list gives the bits of the call without one.  One native call (``nfft_hip_ewald_lj_table_near``; DESIGN.md section
    7t), no atomics: two calls give the same bits."""
    return _ops._nfft_ewald_lj_table_near(pos, xs, types, table, batch, row_start, col, weight_coulomb, weight_lj,
                                          [float(a) for a in box], float(alpha_coulomb), float(alpha_dispersion), float(r_cut))


def nfft_ewald_bmh_table_near(pos, xs, types, table, batch, row_start, col, weight_coulomb, weight_lj, box, alpha_coulomb,
                              alpha_dispersion, r_cut):
    """torch_nfft::_nfft_ewald_bmh_table_near(Tensor pos, Tensor xs, Tensor types, Tensor table, Tensor? batch,
    Tensor? row_start, Tensor? col, Tensor? weight_coulomb, Tensor? weight_lj, float[] box, float alpha_coulomb,
    float alpha_dispersion, float r_cut) -> (Tensor, Tensor) (not in the reference): ``(f, eight)`` of
    ``nfft_ewald_lj_table_near`` for Buckingham / Born-Mayer-Huggins pair potentials.  Every argument is that operator's but
    ``table``, ``[T, T, 4]`` float32 ``(A, B, dC6, C8)`` per pair of types, ``1 <= T <= 32``, with ``dC6 = C6 - c_i c_j``: the pair
    slope is ``q_i q_j mg_C - c_i c_j mg_D + A B e^(-B r) / r - 6 dC6 / r^8 - 8 C8 / r^10`` and the second energy ``1/2 sum
    (A e^(-B r) - dC6 / r^6 - C8 / r^8 - c_i c_j w_D)`` over the pairs within ``r_cut``.  With a list ``q_i q_j`` of a listed pair
    is scaled by ``s^C`` and ``c_i c_j``, ``A``, ``dC6``, ``C8`` by ``s^L`` before they are added; an empty list gives the bits of
    the call without one.  One native call (``nfft_hip_ewald_bmh_table_near``), no atomics: two calls
    give the same bits."""
    return _ops._nfft_ewald_bmh_table_near(pos, xs, types, table, batch, row_start, col, weight_coulomb, weight_lj,
                                           [float(a) for a in box], float(alpha_coulomb), float(alpha_dispersion), float(r_cut))


def nfft_ewald_dispersion_virial_near(pos, x, batch, box, alpha, r_cut):
    """torch_nfft::_nfft_ewald_dispersion_virial_near(Tensor pos, Tensor x, Tensor? batch, float[] box, float alpha,
    float r_cut) -> Tensor (not in the reference): ``nfft_ewald_virial_near`` for the dispersion sum, ``[B, 7, *cols]``
    float64 in the same order, with the pair weights of ``nfft_ewald_dispersion_near``::

        out[b, 0] = 1/2 sum_{i in set b} x_i sum_{j: 0 < r_ij < r_cut} w(r_ij) x_j
        out[b, e] = 1/2 sum_i x_i sum_j mg(r_ij) d_ij[a] d_ij[b] x_j

    Arguments as there.  One native call (``nfft_hip_ewald_dispersion_virial_near``), no atomics:
    two calls give the same bits."""
    return _ops._nfft_ewald_dispersion_virial_near(pos, x, batch, [float(a) for a in box], float(alpha), float(r_cut))


def nfft_ewald_dispersion_virial_far(band, coeffs, strain_coeffs, box):
    """torch_nfft::_nfft_ewald_dispersion_virial_far(Tensor band, Tensor coeffs, Tensor strain_coeffs, float[] box) ->
    Tensor (not in the reference): the spectral part of the same, ``[B, 7, *cols]`` float64, from ``band``
    ``[B, N, N, N, *cols]`` complex64 and a ``DispersionSplitting``'s ``coeffs`` (``b_k``) and ``strain_coeffs()`` (``t_k``),
    both ``[N, N, N]`` float32::

        out[b, 0] = 1/2 sum_k b_k |band_k|^2
        out[b, e] = 1/2 sum_k |band_k|^2 (b_k delta_ab + t_k kappa_a kappa_b),  kappa = A^-1 k

    One native call (``nfft_hip_ewald_dispersion_virial_far``), one pass over ``band``, no atomics."""
    return _ops._nfft_ewald_dispersion_virial_far(band, coeffs, strain_coeffs, [float(a) for a in box])


def nfft_ewald_dipole_near(pos, xs, batch, box, alpha, r_cut, order):
    """torch_nfft::_nfft_ewald_dipole_near(Tensor pos, Tensor xs, Tensor? batch, float[] box, float alpha, float r_cut,
    int order) -> Tensor (not in the reference): the near part of the Ewald sum of charges and point dipoles.  ``xs``
    ``[n, 4, *cols]`` float32 packs ``(q, mu_x, mu_y, mu_z)``; with ``d = d_ij``, ``m = mu_j . d`` and the Smith functions
    ``B_0 = erfc(alpha r) / r``, ``B_l = ((2l - 1) B_(l-1) + (2 alpha^2)^l / (alpha sqrt(pi)) e^(-alpha^2 r^2)) / r^2`` the result
    ``[n, 4, *cols]`` (``order = 1``) holds, over the pairs ``0 < r_ij < r_cut`` of i's point set::

        phi_i  = sum_j q_j B_0 + m B_1
        E_i,a  = sum_j (q_j B_1 + m B_2) d_a - mu_j,a B_1

    and ``[n, 10, *cols]`` (``order = 2``) also ``T_i,ab = sum_j q_j (delta_ab B_1 - d_a d_b B_2) + (mu_j,a d_b + mu_j,b d_a +
    m delta_ab) B_2 - m d_a d_b B_3`` in the order xx, yy, zz, yz, xz, xy.  An empty ``box`` is the unit torus (``pos`` modulo
    1); six numbers are the box of ``nfft_ewald_near_box``: ``pos`` FRACTIONAL, ``mu``, ``E`` and ``T`` Cartesian.  One native
    call (``nfft_hip_ewald_dipole_near`` / ``_near_box``), no atomics: two calls give the same bits."""
    return _ops._nfft_ewald_dipole_near(pos, xs, batch, [float(a) for a in box], float(alpha), float(r_cut), int(order))


def nfft_ewald_dipole_spectral(band, coeffs, box, order):
    """torch_nfft::_nfft_ewald_dipole_spectral(Tensor band, Tensor coeffs, float[] box, int order) -> Tensor (not in the
    reference): from ``band`` ``[B, N, N, N, 4, *cols]`` complex64 (``nfft_adjoint`` of the packed sources) and an
    ``EwaldSplitting``'s ``coeffs`` ``[N, N, N]`` float32 the spectra ``[B, N, N, N, 4 or 10, *cols]`` complex64 whose
    ``nfft_forward`` is the far part of ``(phi, E)`` and, at ``order = 2``, of the six entries of ``T``: with
    ``R = b_k (band_q + 2 pi i kappa . band_mu)``, ``kappa = A^-1 k`` (an empty ``box``: ``kappa = k``), the rows are ``R``,
    ``2 pi i kappa_a R`` and ``4 pi^2 kappa_a kappa_b R``.  One native call (``nfft_hip_ewald_dipole_spectral``; DESIGN.md
    section 7l), one read and one write."""
    return _ops._nfft_ewald_dipole_spectral(band, coeffs, [float(a) for a in box], int(order))


def nfft_ewald_stokeslet_near(pos, f, batch, box, alpha, r_cut, order):
    """torch_nfft::_nfft_ewald_stokeslet_near(Tensor pos, Tensor f, Tensor? batch, float[] box, float alpha, float r_cut,
    int order) -> Tensor (not in the reference): the near part of the periodic Stokeslet sum.  ``f`` ``[n, 3, *cols]`` float32
    holds Cartesian forces; with ``d = d_ij``, ``m = d . f_j``, the Smith functions ``B_0, B_1, B_2`` of
    ``nfft_ewald_dipole_near`` and ``g = (2 alpha / sqrt(pi)) e^(-alpha^2 r^2)`` the result ``[n, 3, *cols]`` (``order = 1``) holds,
    over the pairs ``0 < r_ij < r_cut`` of i's point set::

        u_i,a  = sum_j (B_0 - g) f_j,a + B_1 m d_a

    and ``[n, 12, *cols]`` (``order = 2``) also ``G_i,ab = sum_j (2 alpha^2 g - B_1) f_j,a d_b + B_1 (d_a f_j,b + m delta_ab) -
    B_2 m d_a d_b = d u_a / d x_b`` as rows ``3 + 3 a + b``.  An empty ``box`` is the unit torus (``pos`` modulo 1); six numbers
    are the box of ``nfft_ewald_near_box``: ``pos`` FRACTIONAL, ``f``, ``u`` and ``G`` Cartesian.  One native call
    (``nfft_hip_ewald_stokeslet_near`` / ``_near_box``), no atomics: two calls give the same bits."""
    return _ops._nfft_ewald_stokeslet_near(pos, f, batch, [float(a) for a in box], float(alpha), float(r_cut), int(order))


def nfft_ewald_stokeslet_spectral(band, coeffs, box, order):
    """torch_nfft::_nfft_ewald_stokeslet_spectral(Tensor band, Tensor coeffs, float[] box, int order) -> Tensor (not in the
    reference): from ``band`` ``[B, N, N, N, 3, *cols]`` complex64 (``nfft_adjoint`` of the forces) and
    ``EwaldSplitting.stokeslet_coeffs`` ``[N, N, N]`` float32 the spectra ``[B, N, N, N, 3 or 12, *cols]`` complex64 whose
    ``nfft_forward`` is the far part of ``u`` and, at ``order = 2``, of the nine entries of ``G``: with ``tau = 2 pi kappa``,
    ``kappa = A^-1 k`` (an empty ``box``: ``kappa = k``), ``U = c_k (band - tau (tau . band) / |tau|^2)``, the rows are ``U_a`` and
    ``-i tau_b U_a`` at ``3 + 3 a + b``.  One native call (``nfft_hip_ewald_stokeslet_spectral``), one
    read and one write."""
    return _ops._nfft_ewald_stokeslet_spectral(band, coeffs, [float(a) for a in box], int(order))


def nfft_ewald_rpy_near(pos, f, batch, box, alpha, r_cut, radius, order):
    """torch_nfft::_nfft_ewald_rpy_near(Tensor pos, Tensor f, Tensor? batch, float[] box, float alpha, float r_cut, float radius,
    int order) -> Tensor (not in the reference): the near part of the periodic Rotne-Prager-Yamakawa sum for spheres of the
    radius ``a = radius``.  Arguments, shapes and rows are those of ``nfft_ewald_stokeslet_near``; with ``q = a^2 / 3`` and
    ``B_3 = (5 B_2 + 4 alpha^4 g) / r^2`` the sums over the pairs ``0 < r_ij < r_cut`` are::

        u_i,a  = sum_j W1 f_j,a + W2 m d_a
        G_i,ab = sum_j D1 f_j,a d_b + D2 m d_a d_b + W2 (m delta_ab + d_a f_j,b)
        W1 = (B_0 - g) + q (2 B_1 + (8 alpha^2 - 4 alpha^4 r^2) g)             W2 = B_1 + q (4 alpha^4 g - 2 B_2)
        D1 = (2 alpha^2 g - B_1) + q (-2 B_2 + (8 alpha^6 r^2 - 24 alpha^4) g)     D2 = -B_2 + q (2 B_3 - 8 alpha^6 g)

    and for overlapping spheres, ``r < 2 a``, these plus the difference of the overlap form ``(4 / (3 a)) ((1 - 9 r / (32 a)) I +
    3 d d^T / (32 a r))`` and the unscreened tensor.  ``radius`` must be positive with ``2 radius <= r_cut`` ("Input mismatch").
    Coincident points do not see each other.  One native call (``nfft_hip_ewald_rpy_near`` / ``_near_box``; DESIGN.md section
    7n), no atomics: two calls give the same bits."""
    return _ops._nfft_ewald_rpy_near(pos, f, batch, [float(a) for a in box], float(alpha), float(r_cut), float(radius), int(order))


def nfft_ewald_excl(pos, x, batch, row_start, col, weight, box, alpha, kind, with_field):
    """torch_nfft::_nfft_ewald_excl(Tensor pos, Tensor x, Tensor? batch, Tensor row_start, Tensor col, Tensor weight,
    float[] box, float alpha, int kind, bool with_field) -> (Tensor, Tensor) (not in the reference): what the listed pairs of an
    ``ExclusionList`` -- its CSR arrays ``row_start`` ``[n + 1]`` int32, ``col`` ``[2 m]`` int32, ``weight`` ``[2 m]`` float32 -- take
    out of the Coulomb sum (``kind = 0``) or the dispersion sum (``kind = 1``)::

        z_i   = sum_{k in row i} weight_k K0(r) x[col_k]          K0 = 1 / r,   1 / r^6
        f_i,a = sum_{k in row i} weight_k K1(r) d_a x[col_k]      K1 = 1 / r^3, 6 / r^8

    with ``d`` the minimum image of ``pos_i - pos_col`` as the pair sweeps form it (the same bits) and, at ``r = 0``,
    ``K0 = 2 alpha / sqrt(pi)`` or ``alpha^6 / 6`` and no field.  ``x``, ``z`` and ``f`` as for ``nfft_ewald_near``; ``box`` is
    ``()`` for the unit torus or the six numbers of ``nfft_ewald_near_box`` (``pos`` FRACTIONAL).  The caller subtracts.  One
    native call (``nfft_hip_ewald_excl`` / ``_box``), no atomics: two calls give the same bits."""
    return _ops._nfft_ewald_excl(pos, x, batch, row_start, col, weight, [float(a) for a in box], float(alpha), int(kind),
                                 bool(with_field))


def nfft_ewald_excl_virial(pos, x, batch, row_start, col, weight, box, alpha, kind):
    """torch_nfft::_nfft_ewald_excl_virial(Tensor pos, Tensor x, Tensor? batch, Tensor row_start, Tensor col, Tensor weight,
    float[] box, float alpha, int kind) -> Tensor (not in the reference): ``[B, 7, *cols]`` float64, the listed pairs' share of
    ``nfft_ewald_virial_near`` (``kind = 0``) or ``nfft_ewald_dispersion_virial_near`` (``kind = 1``) in their order, each pair
    once: ``sum weight K0(r) x_i x_j`` and ``sum weight K1(r) d_a d_b x_i x_j`` (at ``r = 0`` the energy only).  Real ``x``;
    ``box`` six numbers, ``pos`` FRACTIONAL.  One native call (``nfft_hip_ewald_excl_virial``), no
    atomics: two calls give the same bits."""
    return _ops._nfft_ewald_excl_virial(pos, x, batch, row_start, col, weight, [float(a) for a in box], float(alpha), int(kind))


def nfft_ewald_yukawa_near(pos, x, batch, box, alpha, r_cut, screening, with_field):
    """torch_nfft::_nfft_ewald_yukawa_near(Tensor pos, Tensor x, Tensor? batch, float[] box, float alpha, float r_cut,
    float screening, bool with_field) -> (Tensor, Tensor) (not in the reference): the near part of the Ewald sum of the screened
    Coulomb potential ``e^(-lambda r) / r``, ``lambda = screening``, ``beta = lambda / (2 alpha)``::

        z[i]    = sum_{j: 0 < r_ij < r_cut} w(r_ij) x[j]                 w  = (P + M) / (2 r)
        f[i, a] = sum_{j: 0 < r_ij < r_cut} mg(r_ij) d_ij[a] x[j]        mg = -w'(r) / r = (w + lambda (M - P) / 2 + g) / r^2
        P = e^(lambda r) erfc(alpha r + beta),  M = e^(-lambda r) erfc(alpha r - beta),  g = (2 alpha / sqrt(pi)) e^(-alpha^2 r^2 - beta^2)

    ``f`` is minus the gradient, ``[n, 3, *cols]``, and empty unless ``with_field``.  ``box`` is ``()`` for the unit torus
    (``nfft_ewald_near``'s arguments and positions) or the six numbers of ``nfft_ewald_near_box`` (``pos`` FRACTIONAL).
    ``screening`` must be finite, ``>= 0`` and at most ``50 / r_cut`` ("Input mismatch"); at 0 the weights are the Coulomb
    ones.  One native call (``nfft_hip_ewald_yukawa_near`` / ``_near_box``), no atomics: two calls give
    the same bits."""
    return _ops._nfft_ewald_yukawa_near(pos, x, batch, [float(a) for a in box], float(alpha), float(r_cut), float(screening),
                                        bool(with_field))


def nfft_ewald_yukawa_virial_near(pos, x, batch, box, alpha, r_cut, screening):
    """torch_nfft::_nfft_ewald_yukawa_virial_near(Tensor pos, Tensor x, Tensor? batch, float[] box, float alpha, float r_cut,
    float screening) -> Tensor (not in the reference): ``nfft_ewald_virial_near`` for the screened Coulomb sum, ``[B, 7, *cols]``
    float64 in the same order, with the pair weights of ``nfft_ewald_yukawa_near``::

        out[b, 0] = 1/2 sum_{i in set b} x_i sum_{j: 0 < r_ij < r_cut} w(r_ij) x_j
        out[b, e] = 1/2 sum_i x_i sum_j mg(r_ij) d_ij[a] d_ij[b] x_j               (xx, yy, zz, yz, xz, xy)

    Arguments as there (``box`` always six numbers), ``screening`` as above.  One native call
    (``nfft_hip_ewald_yukawa_virial_near``), no atomics: two calls give the same bits."""
    return _ops._nfft_ewald_yukawa_virial_near(pos, x, batch, [float(a) for a in box], float(alpha), float(r_cut),
                                               float(screening))


class _on_device:
    """The coefficient operators create their output on the current device (like the reference, which has no
    device argument); ``device=`` selects it for the duration of the call."""

    def __init__(self, device):
        self.ctx = torch.cuda.device(torch.device(device)) if device is not None else None

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()

    def __exit__(self, *exc):
        if self.ctx is not None:
            self.ctx.__exit__(*exc)


def gaussian_analytic_coeffs(sigma, N, dim, device=None):
    """torch_nfft::gaussian_analytic_coeffs(float sigma, int N, int dim) -> Tensor  (core_cuda.cu:855-877)."""
    with _on_device(device):
        return _ops.gaussian_analytic_coeffs(float(sigma), int(N), int(dim))


def gaussian_interpolated_coeffs(sigma, N, dim, p, eps, device=None):
    """torch_nfft::gaussian_interpolated_coeffs(float sigma, int N, int dim, int p, float eps) -> Tensor
    (core_cuda.cu:880-941)."""
    with _on_device(device):
        return _ops.gaussian_interpolated_coeffs(float(sigma), int(N), int(dim), int(p), float(eps))


def interpolation_grid(N, dim, device=None):
    """torch_nfft::interpolation_grid(int N, int dim) -> Tensor [N]*dim + [dim]  (core_cuda.cu:944-966)."""
    with _on_device(device):
        return _ops.interpolation_grid(int(N), int(dim))


def radial_interpolation_grid(N, dim, device=None):
    """torch_nfft::radial_interpolation_grid(int N, int dim) -> Tensor [N]*dim  (core_cuda.cu:969-991)."""
    with _on_device(device):
        return _ops.radial_interpolation_grid(int(N), int(dim))


def interpolated_kernel_coeffs(grid_values):
    """torch_nfft::interpolated_kernel_coeffs(Tensor grid_values) -> Tensor  (core_cuda.cu:994-1064)."""
    return _ops.interpolated_kernel_coeffs(grid_values)
