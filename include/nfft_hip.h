/* nfft_hip.h -- C ABI of the MI355X-native NFFT forward/adjoint hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no torch types.  Every
 * entry point names the interface of the reference (dominikbuenger/torch_nfft)
 * it replaces.  All pointers are DEVICE pointers unless stated otherwise; all
 * work is enqueued on `stream` (a hipStream_t passed as void*) and the calls
 * return without synchronising the device.  Temporaries come from a
 * caller-provided workspace (the host side hands in memory from its caching
 * allocator), so no entry point allocates or frees device memory.
 *
 * Data layouts (reference: docs/source/theory/dataformat.rst:19-63):
 *   pos    float32 [n, dim]            points on the torus, nominally in [-1/2, 1/2)
 *   batch  int64   [n] or NULL         sorted point-set index of every point
 *   x      spatial coefficients  [n, C]            float32 (real) or complex64
 *   xhat   spectral coefficients [B, N^dim, C]     float32 (real) or complex64;
 *          frequency k in [-N/2, N/2) is stored at index k + N/2 on every axis
 * Complex data is interleaved (re, im) float32 pairs, i.e. torch.complex64.
 *
 * Return value: 0 on success, otherwise one of the NFFT_HIP_E* codes;
 * nfft_hip_last_error() returns a human-readable message for the calling thread.
 */
#ifndef NFFT_HIP_H
#define NFFT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NFFT_HIP_OK 0
#define NFFT_HIP_EINVAL 1     /* "Input mismatch" (reference: CHECK_INPUT, csrc/cuda/cuda_utils.cu:3) */
#define NFFT_HIP_EWORKSPACE 2 /* workspace missing or too small */
#define NFFT_HIP_EFFT 3       /* rocFFT plan creation/execution failed (reference: "Failed to create CUFFT plan", core_cuda.cu:255-268) */
#define NFFT_HIP_EHIP 4       /* HIP runtime error (reference aborts the process, cuda_utils.cu:7-14; we report) */
#define NFFT_HIP_EKERNEL 5    /* a kernel of an earlier call on this device reported a fault (nfft_hip_check_status) */

#define NFFT_HIP_ABI_VERSION 7

int nfft_hip_abi_version(void);
const char *nfft_hip_last_error(void);

/* Faults that only a running kernel can detect -- a bounded wait inside the streamed interpolation kernel ran out,
 * a batch index outside [0, batch_size) in the middle of the batch vector, a cached plan whose points have changed
 * (nfft_hip_plan_verify) -- are raised in a host-mapped status block
 * of the device and turned into an error by the NEXT entry point called on that device: it returns NFFT_HIP_EKERNEL
 * (NFFT_HIP_EINVAL for the batch vector) without running, and clears the flag.  nfft_hip_check_status looks at the
 * block on demand; with synchronize != 0 it first waits for `stream`, so that a fault of the work just enqueued is
 * seen.  Replaces CHECK_ERRORS of the reference (csrc/cuda/cuda_utils.cu:5-16: cudaDeviceSynchronize, print,
 * exit()) for the failures a kernel can only report itself. */
int nfft_hip_check_status(void *stream, int synchronize);

/* Problem description shared by the entry points below.
 * Mirrors the arguments of the reference operators (csrc/core.cpp:43-105):
 *   dim           pos.size(1), 1..3                       (core_cuda.cu:50-51)
 *   num_points    pos.size(0)
 *   num_columns   x.numel() / num_points  resp.  x.numel() / (B * N^dim)   (core_cuda.cu:84, 108-113)
 *   batch_size    batch[-1] + 1, or 1 when batch is NULL  (core_cuda.cu:60-65) -- read back by the HOST side
 *   N             bandwidth (even, >= 2);  m  window cutoff, 1 <= m, 2m+2 <= 2N
 *   flags         hints about the point geometry (0 = none).  They never change results, only which kernels run; a
 *                 point plan must be used with the flags it was built with.
 */
#define NFFT_HIP_POINTS_IN_QUARTER_BALL 1 /* every point lies within radius 1/4 of the origin -- the fastsum geometry
                                           * (test/test_fastsum.py:17-18, torch_nfft/kernel.py:77): the points occupy at
                                           * most 1/8 of the grid, so their local density is 8x the average */
typedef struct nfft_hip_problem {
    int32_t dim;
    int32_t flags;
    int64_t num_points;
    int64_t num_columns;
    int64_t batch_size;
    int64_t N;
    int64_t m;
} nfft_hip_problem;

/* Bytes of workspace needed by nfft_hip_adjoint / nfft_hip_forward for this problem
 * (creates and caches the rocFFT plans on the current device; returns < 0 on error).
 * x_is_complex / real_output as in the calls below. */
int64_t nfft_hip_adjoint_workspace_bytes(const nfft_hip_problem *p, int x_is_complex, int real_output);
int64_t nfft_hip_forward_workspace_bytes(const nfft_hip_problem *p, int x_is_complex, int real_output);

/* Adjoint NFFT:  y[b, k+N/2, c] ~= sum_{i: batch[i]=b} x[i,c] exp(+2 pi i k.pos[i]).
 * Replaces nfft_adjoint_cuda (csrc/cuda/core_cuda.cu:144-336), i.e. the operator
 * torch_nfft::nfft_adjoint(pos, x, batch, N, m, real_output) (csrc/core.cpp:43-55, 177).
 *   x  [n, C] float32 (x_is_complex = 0) or complex64 (x_is_complex = 1)
 *   y  [B, N^dim, C] complex64, or float32 holding the real part when real_output != 0;
 *      every element is written (the caller need not zero it). */
int nfft_hip_adjoint(const nfft_hip_problem *p, const float *pos, const void *x, int x_is_complex,
                     const int64_t *batch, int real_output, void *y,
                     void *workspace, int64_t workspace_bytes, void *stream);

/* Forward NFFT:  y[i,c] ~= sum_k xhat[batch[i], k+N/2, c] exp(-2 pi i k.pos[i]).
 * Replaces nfft_forward_cuda (csrc/cuda/core_cuda.cu:340-531), i.e. the operator
 * torch_nfft::nfft_forward(pos, x, batch, m, real_output) (csrc/core.cpp:94-105, 178).
 *   xhat [B, N^dim, C] float32 or complex64;  y [n, C] complex64 or float32 (real part). */
int nfft_hip_forward(const nfft_hip_problem *p, const float *pos, const void *xhat, int x_is_complex,
                     const int64_t *batch, int real_output, void *y,
                     void *workspace, int64_t workspace_bytes, void *stream);

/* 0 when the library runs this problem WITHOUT a point plan: problems whose oversampled grid ((2N)^dim cells, 2N a power
 * of two, at most 4096 cells) fits one workgroup's LDS and whose point sets are small run nfft_hip_adjoint / nfft_hip_forward as one
 * kernel each -- workspace may be NULL for them, and building a plan for the *_planned entry points would only add five
 * launches.  1 otherwise (callers that transform the same points repeatedly then build the plan once).  No reference
 * counterpart: the reference recomputes shifts and window values in every call (core_cuda.cu:188-211). */
int nfft_hip_plan_needed(const nfft_hip_problem *p);

/* The same two transforms on an existing point plan (nfft_hip_plan_points below): the plan depends only on
 * (pos, batch, dim, N, m) -- with them num_points and batch_size, from which the tiling is chosen -- and on whether
 * num_columns is 1 or larger (sparse 3-D problems: the spreading kernel's tiling of the plan differs), and can be shared by
 * any number of adjoint / forward calls on the same points with column counts of the same class -- pass the same
 * nfft_hip_problem to the plan and to its users.  The
 * reference re-derives shifts and psi in every call but reuses them when sources.is_same(targets)
 * (core_cuda.cu:552-564).  The workspace sizes are those of the un-planned calls. */
int nfft_hip_adjoint_planned(const nfft_hip_problem *p, const void *plan, const void *x, int x_is_complex,
                             int real_output, void *y, void *workspace, int64_t workspace_bytes, void *stream);
int nfft_hip_forward_planned(const nfft_hip_problem *p, const void *plan, const void *xhat, int x_is_complex,
                             int real_output, void *y, void *workspace, int64_t workspace_bytes, void *stream);

/* Gradient of a forward transform with respect to the points (no counterpart: the reference has no gradient w.r.t. pos).
 * With Fr[i, cr] the real columns of y = nfft_hip_forward(xhat) at the points (Cr = C with real_output, else 2C:
 * re, im interleaved),
 *     dpos[i, a] = sum_cr w[i, cr] * d Fr[i, cr] / d pos[i, a],
 * evaluated the way the transform itself is: the same deconvolved, FFT'd grid, gathered with the derivative of the
 * window.  Autograd uses it for both transforms: for y = forward(xhat, pos), xhat and w = the real view of dy; for
 * y = adjoint(x, pos), xhat = dy with real_output = !x_is_complex and w = the real view of x.
 *   w     float32 [n, Cr] in caller order;  dpos  float32 [n, dim], every element is written
 * Always runs on a point plan (nfft_hip_plan_points, same problem), also for problems whose transforms need none
 * (nfft_hip_plan_needed == 0).  Deterministic: no atomics, the same inputs give bitwise the same dpos.
 * Workspace: the forward transform's plus, when Cr > 1, Cr * n * dim floats of per-plane partial gradients. */
int64_t nfft_hip_forward_grad_workspace_bytes(const nfft_hip_problem *p, int x_is_complex, int real_output);
int nfft_hip_forward_grad_points_planned(const nfft_hip_problem *p, const void *plan, const void *xhat,
                                         int x_is_complex, int real_output, const float *w, float *dpos,
                                         void *workspace, int64_t workspace_bytes, void *stream);
/* The forward transform and its weighted point gradient in one pass: y as nfft_hip_forward_planned writes it (same layout,
 * same normalisation; [n, C] float32 with real_output, else complex64) and dpos as nfft_hip_forward_grad_points_planned,
 * from one gather that stores the value it has in registers anyway.  Same workspace
 * (nfft_hip_forward_grad_workspace_bytes).  y agrees with the forward transform's to rounding, not bit for bit: the
 * transform may gather with another kernel. */
int nfft_hip_forward_value_grad_points_planned(const nfft_hip_problem *p, const void *plan, const void *xhat,
                                               int x_is_complex, int real_output, const float *w, void *y, float *dpos,
                                               void *workspace, int64_t workspace_bytes, void *stream);
/* The backward of that gradient, for second derivatives (double backward of both transforms).  With
 * G[i, a] = sum_cr w[i, cr] d Fr[i, cr] / d pos[i, a] as nfft_hip_forward_grad_points_planned computes it and an upstream
 * v float32 [n, dim] (caller order), any subset of
 *     dxhat  d<v, G>/d xhat = sum_a 2 pi i k_a adjoint(pos, omega v_a),  omega = w_re + i w_im (w with real_output);
 *            xhat's layout and type (the real part for real xhat)
 *     dw     float32 [n, Cr]:  dw[i, cr] = sum_a v[i, a] d Fr[i, cr] / d pos[i, a]
 *     dpos   float32 [n, dim]: dpos[i, b] = sum_cr w[i, cr] sum_a v[i, a] d^2 Fr[i, cr] / d pos[i, a] d pos[i, b]
 * NULL outputs are skipped.  dw and dpos come from one gather of the window's first and second derivatives on the forward
 * transform's grid, deterministic like the first-order gather; dxhat from the derivative spreading of w and the
 * adjoint's FFT stage on 1-D, 2-D and narrow 3-D tilings, else from dim adjoints of omega v_a on the same plan.
 * No points or no columns: zeros.  w may be NULL when only dw is asked for.  Workspace: the query below. */
int64_t nfft_hip_forward_grad_points_backward_workspace_bytes(const nfft_hip_problem *p, int x_is_complex, int real_output);
int nfft_hip_forward_grad_points_backward_planned(const nfft_hip_problem *p, const void *plan, const void *xhat,
                                                  int x_is_complex, int real_output, const float *w, const float *v,
                                                  void *dxhat, float *dw, float *dpos, void *workspace,
                                                  int64_t workspace_bytes, void *stream);

/* ---- stage-level entry points (used by the parity tests and by bench.py to time
 * the spreading kernel on its own; the two calls above are built from them) ---- */

/* Size in bytes of a point plan (tile-sorted copy of the points) for this problem. */
int64_t nfft_hip_plan_bytes(const nfft_hip_problem *p);

/* Bin the points into grid tiles.  Replaces compute_shifts_kernel + compute_psi_kernel
 * (csrc/cuda/spatial_window_operations.cu:38-97, launched at core_cuda.cu:188-211): instead of
 * materialising shifts and 2m+2 window values per point and axis in HBM, the points are
 * counting-sorted by tile and the window is re-evaluated in registers by the consumers. */
int nfft_hip_plan_points(const nfft_hip_problem *p, const float *pos, const int64_t *batch,
                         void *plan, int64_t plan_bytes, void *stream);

/* Verification of a plan that is kept across calls.  nfft_hip_plan_points leaves a 64-bit checksum of pos (and batch) in
 * the plan -- its seal, formed by the pass that counts the points, at no extra cost; nfft_hip_plan_verify recomputes it
 * from the arrays as they are NOW (one streaming pass, ~25 us for 10^7 3-D points) and raises a device fault when it
 * differs: the next entry point on the device returns NFFT_HIP_EINVAL ("stale point plan"), nfft_hip_check_status sees
 * it on demand.  A cache of plans keyed on buffer identity (core.so's: tensor address + version counter) cannot see a
 * write that bypasses its key; the reference has no such state -- it recomputes shifts and psi in every call
 * (csrc/cuda/core_cuda.cu:188-211) -- so a drop-in must not return a transform of points that are no longer there
 * without saying so. */
int nfft_hip_plan_verify(const nfft_hip_problem *p, const float *pos, const int64_t *batch, void *plan, void *stream);

/* Spreading (adjoint gridding):  grid[(b*Cr + cr), u] += xr[i, cr] * prod_k psi_k(i, u_k)
 * over real columns cr (a complex x is viewed as 2C real columns).  Replaces
 * real_/complex_adjoint_window_convolution_kernel (spatial_window_operations.cu:103-211).
 *   grid  float32 [B*Cr, (2N)^dim] real planes; every cell is written by this call.
 *   scratch  nfft_hip_spread_scratch_bytes(p, Cr) bytes: the tile-ordered copy of xr (n * Cr floats, or one per plan
 *            entry when the problem is sparse enough for the owner-computes kernel, whose plan enters a point into
 *            every tile its window touches), one word per plane (its largest |x|, the operand scale of the
 *            matrix-core kernel) and the ticket counters of the kernel's persistent launch. */
int64_t nfft_hip_spread_scratch_bytes(const nfft_hip_problem *p, int64_t real_columns);
int nfft_hip_spread(const nfft_hip_problem *p, const void *plan, const float *xr, int64_t real_columns,
                    float *grid, float *scratch, void *stream);

/* Interpolation (forward gather):  yr[i, cr] = sum_u grid[(b*Cr + cr), u] * prod_k psi_k(i, u_k).
 * Replaces complex_/real_forward_window_convolution_kernel (spatial_window_operations.cu:214-332).
 * There is no workspace for ticket counters here: on an unbalanced (clustered) plan the persistent launch deals its
 * work list round robin, where nfft_hip_forward hands it out dynamically. */
int nfft_hip_interpolate(const nfft_hip_problem *p, const void *plan, const float *grid,
                         int64_t real_columns, float *yr, void *stream);

/* ---- fast summation and kernel coefficients ----
 * nfft_fastsum of the reference (csrc/cuda/core_cuda.cu:535-852) is adjoint(sources) -> spectral multiply ->
 * forward(targets); its spectral step (spectral_window_operations.cu:269-402: g_hat *= coeffs * phi_hat_inv^2 on
 * the band, 0 elsewhere) is, on the band spectrum that nfft_hip_adjoint returns and nfft_hip_forward consumes,
 * the plain product below.  yhat [B, N^dim, C] complex64 in place; coeffs [N^dim] float32 or complex64. */
int nfft_hip_spectral_multiply(void *yhat, const void *coeffs, int coeffs_are_complex, int64_t batch_size,
                               int64_t band_size, int64_t num_columns, void *stream);

/* One-call fast summation:  y[j, c] = Re?[ sum_k coeffs[k] (sum_i x[i, c] e^{+2 pi i k.s_i}) e^{-2 pi i k.t_j} ].
 * Replaces nfft_fastsum_cuda (csrc/cuda/core_cuda.cu:535-852), i.e. the operator
 * torch_nfft::nfft_fastsum(sources, targets, x, coeffs, source_batch, target_batch, m) (csrc/core.cpp:108-121, 179):
 * spreading of the sources -> inverse FFT -> product with coeffs * phi_hat_inv^2 on the band
 * (spectral_window_operations.cu:269-402; here folded into the last spectral pass of the adjoint half) -> FFT ->
 * interpolation at the targets.
 *   src / tgt   the two point sets: same dim, N, m, batch_size and num_columns, their own num_points
 *   x  [n_s, C] float32 or complex64;  coeffs [N^dim] float32 or complex64 (index l + N/2 on every axis)
 *   y  [n_t, C] float32 when x is real (the real part, core_cuda.cu:817-821), complex64 otherwise
 * When `targets == sources` (same pointer, same batch pointer, same count) one point plan serves both halves, as in
 * the reference (core_cuda.cu:552-564).  The _planned variant takes existing point plans (the same pointer twice
 * for shared points).  Workspace: nfft_hip_fastsum_workspace_bytes(src, tgt, x_is_complex, shared_points, planned). */
int64_t nfft_hip_fastsum_workspace_bytes(const nfft_hip_problem *src, const nfft_hip_problem *tgt, int x_is_complex,
                                         int shared_points, int planned);
int nfft_hip_fastsum(const nfft_hip_problem *src, const float *sources, const int64_t *source_batch,
                     const nfft_hip_problem *tgt, const float *targets, const int64_t *target_batch, const void *x,
                     int x_is_complex, const void *coeffs, int coeffs_are_complex, void *y, void *workspace,
                     int64_t workspace_bytes, void *stream);
/* (The fastsum drivers treat both point sets as NFFT_HIP_POINTS_IN_QUARTER_BALL whatever `flags` says: plans handed
 * to the _planned variant must have been built with that flag set.) */
int nfft_hip_fastsum_planned(const nfft_hip_problem *src, const void *source_plan, const nfft_hip_problem *tgt,
                             const void *target_plan, const void *x, int x_is_complex, const void *coeffs,
                             int coeffs_are_complex, void *y, void *workspace, int64_t workspace_bytes, void *stream);
/* The same fast summation that also returns its band spectrum band = coeffs * A_s(x), [B, N^dim, C] complex64 with the
 * coefficients multiplied in (y = forward_t(band)): what the gradient with respect to the targets needs.  Same workspace
 * (nfft_hip_fastsum_workspace_bytes), same route and the same computation of y as nfft_hip_fastsum[_planned] (equal up to
 * the order of the spreading atomics, which varies from call to call on most routes); band is written whenever y is (no
 * targets or no columns: neither is). */
int nfft_hip_fastsum_band(const nfft_hip_problem *src, const float *sources, const int64_t *source_batch,
                          const nfft_hip_problem *tgt, const float *targets, const int64_t *target_batch, const void *x,
                          int x_is_complex, const void *coeffs, int coeffs_are_complex, void *y, void *band,
                          void *workspace, int64_t workspace_bytes, void *stream);
int nfft_hip_fastsum_band_planned(const nfft_hip_problem *src, const void *source_plan, const nfft_hip_problem *tgt,
                                  const void *target_plan, const void *x, int x_is_complex, const void *coeffs,
                                  int coeffs_are_complex, void *y, void *band, void *workspace, int64_t workspace_bytes,
                                  void *stream);

/* Backward of the fast summation y = fastsum(x, c, sources, targets) (no reference counterpart), with dy the upstream
 * gradient in y's layout and torch's convention, and the real views of DESIGN.md section 7a:
 *   dtargets[i] = sum_cr dy[i, cr] d Fr[i, cr] / d t_i,  F = forward_t(band)            (band: nfft_hip_fastsum_band's)
 *   dsources[j] = Re(conj(x_j) grad H(s_j)),             H = forward_s(coeffs * A_t(dy))
 *   dx          = H(s_j) (its real part when x is real)
 * `coeffs` is the array of the sources' grid: conj(c) for the gradient of the forward pass with coefficients c (c itself
 * when c is real; then dx is the forward pass's x gradient, the swapped fastsum, to rounding).  One adjoint at the targets
 * (the coefficients folded into its roll-off), one forward FFT stage at the sources and one gather -- the value-writing one
 * when dx is wanted too; one forward FFT stage at the targets and one gradient gather.  Each of dx, dsources, dtargets may
 * be NULL.  dsources [n_s, dim], dtargets [n_t, dim] float32.  Both problems are treated as NFFT_HIP_POINTS_IN_QUARTER_BALL
 * and take the forward pass's plans.  No columns or an empty side: zero gradients.  Deterministic (no atomics after the
 * adjoint's spreading).  Workspace: nfft_hip_fastsum_grad_workspace_bytes. */
int64_t nfft_hip_fastsum_grad_workspace_bytes(const nfft_hip_problem *src, const nfft_hip_problem *tgt, int x_is_complex);
int nfft_hip_fastsum_backward_planned(const nfft_hip_problem *src, const void *source_plan, const nfft_hip_problem *tgt,
                                      const void *target_plan, const void *x, int x_is_complex, const void *dy,
                                      const void *coeffs, int coeffs_are_complex, const void *band, void *dx,
                                      float *dsources, float *dtargets, void *workspace, int64_t workspace_bytes,
                                      void *stream);

/* ---- Toeplitz normal operator A^H W A (no reference counterpart) ----
 * With A = nfft_hip_forward on a fixed point set and W = diag(w) real weights,
 *     (A^H W A)[k, k'] = sum_i w_i e^{2 pi i (k - k').pos_i} = t[k - k']
 * is a dim-level Toeplitz matrix.  It embeds in a circulant of size M = 2N per axis, so one application is the forward
 * FFT stage (band -> grid M^dim, no roll-off), a pointwise product with a real grid K and the adjoint FFT stage (grid ->
 * band, no roll-off): no points, no plan, no spreading and no gather, at a cost independent of the number of points.
 *
 * Set-up, once per (points, weights):  t = nfft_hip_adjoint of the weights at bandwidth 2N (real x = w, one column),
 * [B, (2N)^dim] complex64 with lag n at index n + N;  nfft_hip_toeplitz_kernel turns it into
 *     K[b, j] = M^-dim sum_n t[b, n] e^{-2 pi i n.j / M},   j in [0, M)^dim,   float32 [B, M^dim]
 * (lags with a component -N never occur in k - k' and are dropped; the Hermitian part of t is taken, so K is real).
 * p is the bandwidth-N problem: dim, N and batch_size are read, m must be valid, num_points / num_columns are ignored. */
int64_t nfft_hip_toeplitz_kernel_workspace_bytes(const nfft_hip_problem *p);
int nfft_hip_toeplitz_kernel(const nfft_hip_problem *p, const void *t, float *K, void *workspace, int64_t workspace_bytes,
                             void *stream);
/* Application:  y = A^H W A xhat  for xhat [B, N^dim, C] float32 (x_is_complex = 0) or complex64;  y [B, N^dim, C] is
 * always complex64, every element is written.  K must be 16-byte aligned.  p->num_points is ignored (0 is valid),
 * p->num_columns = C; p->m is not used beyond validation.  The planes of the grid (two per column: re, im) run through
 * the FFT stages of the transforms in chunks (NFFT_HIP_CHUNK_BYTES); chunked and unchunked results are bitwise equal,
 * and so are repeated calls (no atomics anywhere). */
int64_t nfft_hip_toeplitz_workspace_bytes(const nfft_hip_problem *p);
int nfft_hip_toeplitz_apply(const nfft_hip_problem *p, const float *K, const void *xhat, int x_is_complex, void *y,
                            void *workspace, int64_t workspace_bytes, void *stream);

/* ---- near field of the fast summation for singular kernels (no reference counterpart) ----
 * The fast summation is exact only for kernels that are smooth on the torus.  For K(r) = 1/r, log r, ... the host side
 * sums a regularised kernel K_R with nfft_hip_fastsum -- K replaced inside the radius eps_I by the even polynomial
 * T_I(r) = sum_{k < poly_terms} poly[k] (r / eps_I)^(2k) that matches its derivatives at eps_I -- and this entry point adds
 *     z[i, c] = sum_{j in the point set of i, |t_i - s_j| < eps_I} (K(r_ij) - T_I(r_ij)) xr[j, c],   r_ij = |t_i - s_j|
 * (Euclidean, not periodic: the points lie in the quarter ball).  A pair with r = 0 contributes K(0) - poly[0] for the
 * kernels that are finite at 0 and -poly[0] for 1/r, 1/r^2 and log r: the singular self term is left out of the sum.
 *
 * Both point sets come ORDERED BY CELL: cells_per_axis^dim cubes of edge 1 / (2 cells_per_axis) >= eps_I over
 * [-1/4, 1/4]^dim, cell index c_0 + G c_1 + G^2 c_2 with c_a = clamp(floor((pos_a + 1/4) 2 G), 0, G - 1), key =
 * point set * G^dim + cell; the caller sorts by key (stably) and passes
 *   sources [n_s, dim] float32, xr [n_s, Cr] float32 (real columns; re, im interleaved for complex data) in that order
 *   source_start / target_start  int32 [batch_size * G^dim + 1]: index of the first point with key >= entry
 *   targets [n_t, dim] float32 in that order, target_index int64 [n_t]: the row of z that sorted target i writes
 *   z [n_t, Cr] float32: row target_index[i] is written for every target whose key lies in the table
 * nfft_hip_nearfield_cells proposes cells_per_axis: the most cells with edge >= eps_I, at most 2^20 in all point sets.
 * No atomics: a target's pairs are added in the order of the sorted sources, two calls give the same bits.  No targets or
 * no columns: nothing is done; no sources: z is zeroed.  Workspace: the work items (blocks of targets of one cell). */
#define NFFT_HIP_KERNEL_ONE_OVER_MODULUS 0     /* 1 / r */
#define NFFT_HIP_KERNEL_ONE_OVER_SQUARE 1      /* 1 / r^2 */
#define NFFT_HIP_KERNEL_LOGARITHM 2            /* log r */
#define NFFT_HIP_KERNEL_THINPLATE_SPLINE 3     /* r^2 log r */
#define NFFT_HIP_KERNEL_MULTIQUADRIC 4         /* sqrt(r^2 + c^2) */
#define NFFT_HIP_KERNEL_INVERSE_MULTIQUADRIC 5 /* 1 / sqrt(r^2 + c^2) */
#define NFFT_HIP_KERNEL_GAUSSIAN 6             /* exp(-r^2 / c^2) */
#define NFFT_HIP_KERNEL_LAPLACIAN_RBF 7        /* exp(-r / c) */
typedef struct nfft_hip_nearfield_problem {
    int32_t dim;            /* 1..3 */
    int32_t kernel;         /* NFFT_HIP_KERNEL_* */
    int32_t poly_terms;     /* p, 1..8 */
    int32_t cells_per_axis; /* G >= 1 with 1 / (2 G) >= eps_I */
    int64_t num_sources;
    int64_t num_targets;
    int64_t num_columns;    /* real columns Cr */
    int64_t batch_size;
    double c;               /* shape parameter (> 0 for the last three kernels, >= 0 for the multiquadric) */
    double eps_I;
    double poly[8];         /* a_0 .. a_{p-1} */
} nfft_hip_nearfield_problem;
int64_t nfft_hip_nearfield_cells(int32_t dim, double eps_I, int64_t batch_size);
int64_t nfft_hip_nearfield_workspace_bytes(const nfft_hip_nearfield_problem *p);
int nfft_hip_nearfield(const nfft_hip_nearfield_problem *p, const float *sources, const float *xr,
                       const int32_t *source_start, const float *targets, const int64_t *target_index,
                       const int32_t *target_start, float *z, void *workspace, int64_t workspace_bytes, void *stream);

/* ---- gradient of that near field at the targets, and its transpose ----
 * With g(r^2) = (K'(r) - T_I'(r)) / r and the pairs of nfft_hip_nearfield without those at r = 0 (they weigh exactly zero),
 *   transpose = 0:  out[i, a, c] = sum_j g(r_ij^2) (t_i - s_j)[a] xr[j, c]        out [n_t, dim, Cr], xr [n_s, Cr]
 *   transpose = 1:  out[j, c]    = sum_i g(r_ij^2) sum_a (t_i - s_j)[a] xr[i, a, c]   out [n_s, Cr], xr [n_t, dim, Cr]
 * K'(r) / r is evaluated in closed form from r^2 for the kernel p->kernel;  T_I'(r) / r = sum_{k < poly_terms - 1}
 * gradient_poly[k] (r / eps_I)^(2k) with gradient_poly[k] = (2 / eps_I^2) (k + 1) a_{k+1}: poly_terms - 1 DOUBLES that the
 * host derives from the a_k of T_I.  p->poly_terms counts the terms of T_I and must be >= 2 (with one term K_R is only
 * continuous and g does not vanish at eps_I); p->poly is validated as for nfft_hip_nearfield and not read.
 *
 * The arguments keep the roles they have in nfft_hip_nearfield, named by what the kernel does with them: `sources`, `xr`,
 * `source_start` and p->num_sources are the STREAMED side, `targets`, `target_index`, `target_start` and p->num_targets the
 * OUTPUT side (row target_index[i] of `out` is written for the sorted output point i).  For transpose = 1 the caller
 * therefore passes the sum's targets (with their values, rows in cell order) as the streamed side and the sum's sources
 * as the output side; the library takes the difference vector with the sign above in both modes.  Ordering by cell,
 * start tables, determinism, empty sides and the workspace are those of nfft_hip_nearfield. */
int64_t nfft_hip_nearfield_gradient_workspace_bytes(const nfft_hip_nearfield_problem *p);
int nfft_hip_nearfield_gradient(const nfft_hip_nearfield_problem *p, int32_t transpose, const double *gradient_poly,
                                const float *sources, const float *xr, const int32_t *source_start, const float *targets,
                                const int64_t *target_index, const int32_t *target_start, float *out, void *workspace,
                                int64_t workspace_bytes, void *stream);

/* ---- gradient of that near field with respect to the points ----
 * For z = nfft_hip_nearfield(xr) and a loss L with dy = dL/dz [n_t, Cr], the pairs and g of nfft_hip_nearfield_gradient:
 *   dL/dt_i[a] = sum_j g(r_ij^2) (t_i - s_j)[a] sum_c dy[i, c] xr[j, c]
 *   dL/ds_j[a] = sum_i g(r_ij^2) (s_j - t_i)[a] sum_c xr[j, c] dy[i, c]
 * Both are one sum, named by what the kernel does with its arguments: with the STREAMED side `streamed` (positions),
 * `streamed_values` [p->num_sources, Cr], `streamed_start` and the OUTPUT side `output`, `output_values`
 * [p->num_targets, Cr], `output_index`, `output_start`, all rows in cell order,
 *   symmetric = 0:  out[output_index[i], a] = sum_j g(r_ij^2) (output_i - streamed_j)[a]
 *                                             sum_c output_values[i, c] streamed_values[j, c]
 * so the targets' gradient passes the sum's sources with xr as the streamed side and its targets with dy as the output
 * side, and the sources' gradient passes them the other way round (targets with dy streamed, sources with xr the output
 * side).  The difference vector is "output - streamed" in both: no sign to turn.
 *   symmetric = 1:  the two sides are ONE point set in one cell order (p->num_sources == p->num_targets, the same
 *                   positions and start table on both sides); the inner sum becomes
 *                   sum_c output_values[i, c] streamed_values[j, c] + streamed_values[i, c] output_values[j, c]
 *                   and out is the sum of the two gradients of point i (dy as output_values, xr as streamed_values).
 * out is [p->num_targets, dim] float32.  gradient_poly, p->poly_terms (>= 2), p->poly, ordering by cell, start tables,
 * determinism and the workspace are those of nfft_hip_nearfield_gradient.  No output points or no columns: nothing is
 * done; no streamed points: out is zeroed. */
int64_t nfft_hip_nearfield_point_gradient_workspace_bytes(const nfft_hip_nearfield_problem *p);
int nfft_hip_nearfield_point_gradient(const nfft_hip_nearfield_problem *p, int32_t symmetric, const double *gradient_poly,
                                      const float *streamed, const float *streamed_values, const int32_t *streamed_start,
                                      const float *output, const float *output_values, const int64_t *output_index,
                                      const int32_t *output_start, float *out, void *workspace, int64_t workspace_bytes,
                                      void *stream);

/* ---- near part of the Ewald sum for the periodic 1/r (no reference counterpart) ----
 * The Coulomb sum over all images of the unit box is split with erf / erfc: the smooth part is summed on the whole torus
 * with nfft_hip_fastsum (coefficients exp(-pi^2 |k|^2 / alpha^2) / (pi |k|^2), set up by the host side), and this entry
 * point adds the short-ranged rest for ONE point set on both sides (targets are the sources), 3-D only:
 *     z[i, c]     =  sum_{j in the point set of i, 0 < r_ij < r_cut} erfc(alpha r_ij) / r_ij  xr[j, c]
 *     field[i, a, c] = -sum_j g(r_ij^2) d_ij[a] xr[j, c]   (with_field = 1; field [n, 3, Cr]; not touched otherwise)
 * with g = K'(r) / r = -erfc(alpha r) / r^3 - (2 alpha / sqrt(pi)) exp(-alpha^2 r^2) / r^2.  The sum is PERIODIC: d_ij is
 * the minimum image of points_i - points_j, d -= rint(d) on every axis, and r_ij its length.  Coincident points (r = 0,
 * the point itself among them) weigh zero.  The points must already be reduced to [-1/2, 1/2)^3.
 *
 * The points come ORDERED BY CELL: cells_per_axis^3 cubes of edge 1 / cells_per_axis >= r_cut over the whole torus, cell
 * index c_0 + G c_1 + G^2 c_2 with c_a = min(floor((pos_a + 1/2) G), G - 1), key = point set * G^3 + cell; the caller
 * sorts by key (stably) and passes
 *   points [n, 3] float32, xr [n, Cr] float32 (real columns; re, im interleaved for complex data) in that order
 *   start  int32 [batch_size * G^3 + 1]: index of the first point with key >= entry
 *   index  int64 [n]: the row of z (and of field) that sorted point i writes
 * G >= 3 is required, so that the 27 wrapped neighbours of a cell are 27 distinct cells; hence r_cut <= 1/3.
 * nfft_hip_ewald_near_cells proposes cells_per_axis: floor(1 / r_cut), lowered until batch_size * G^3 <= 2^20; -1 with
 * "Input mismatch..." unless 0 < r_cut <= 1/3 (or if no G >= 3 fits that many point sets).
 * No atomics: a point's pairs are added in the order of the sorted points (row by row of the wrapped walk), two calls
 * give the same bits.  No points or no columns: nothing is done.  Workspace: the work items, as for nfft_hip_nearfield. */
typedef struct nfft_hip_ewald_problem {
    int32_t cells_per_axis; /* G >= 3 with 1 / G >= r_cut */
    int32_t with_field;     /* 0: z only; 1: z and field */
    int64_t num_points;
    int64_t num_columns;    /* real columns Cr */
    int64_t batch_size;
    double alpha;           /* splitting parameter, > 0 */
    double r_cut;           /* in (0, 1/3] */
} nfft_hip_ewald_problem;
int64_t nfft_hip_ewald_near_cells(double r_cut, int64_t batch_size);
int64_t nfft_hip_ewald_near_workspace_bytes(const nfft_hip_ewald_problem *p);
int nfft_hip_ewald_near(const nfft_hip_ewald_problem *p, const float *points, const float *xr, const int32_t *start,
                        const int64_t *index, float *z, float *field, void *workspace, int64_t workspace_bytes,
                        void *stream);

/* ---- the same pair sum in an orthorhombic or triclinic box (no reference counterpart) ----
 * The box is the lower-triangular matrix A whose rows are the lattice vectors,
 *     a_1 = (A00, 0, 0), a_2 = (A10, A11, 0), a_3 = (A20, A21, A22),   box[6] = A00, A10, A11, A20, A21, A22,
 * with a positive diagonal.  The points are FRACTIONAL, s in [-1/2, 1/2)^3 with Cartesian x = s A, and
 *     d_ij = (ds - rint(ds)) A,  ds = s_i - s_j,   r_ij = |d_ij|,
 * so alpha, r_cut, z and field (Cartesian components) are in the box's own units; the sums are those of
 * nfft_hip_ewald_near.  The perpendicular width of the box along fractional axis a is w_a = 1 / |column a of A^-1|.
 *
 * The points come ORDERED BY CELL: cells[0] x cells[1] x cells[2] cells of fractional edge 1 / cells[a] with
 * w_a / cells[a] >= r_cut, cell index c_0 + G_0 (c_1 + G_1 c_2) with c_a = min(floor((s_a + 1/2) G_a), G_a - 1),
 * key = point set * G_0 G_1 G_2 + cell; points, xr, start (int32 [batch_size * G_0 G_1 G_2 + 1]) and index as for
 * nfft_hip_ewald_near.  Every G_a >= 3 is required, hence r_cut <= min_a w_a / 3: then an image with |d| < r_cut has
 * |ds_a| <= |d| / w_a < 1/3 on every axis, so the componentwise rint finds it, it is the only one, and it lies in one of
 * the 27 wrapped neighbour cells.
 * nfft_hip_ewald_box_cells proposes cells_out[a] = floor(w_a / r_cut), then lowers the largest entry first until
 * batch_size * G_0 G_1 G_2 <= 2^20; it returns 0, or -1 with "Input mismatch..." for a non-positive diagonal, entries that
 * are not finite, r_cut outside (0, min_a w_a / 3] or if no grid with every G_a >= 3 fits that many point sets.
 * No atomics, two calls give the same bits; no points or no columns: nothing is done.  Workspace: the work items. */
typedef struct nfft_hip_ewald_box_problem {
    int32_t cells[3];    /* G_a >= 3 with w_a / G_a >= r_cut */
    int32_t with_field;  /* 0: z only; 1: z and field */
    int64_t num_points;
    int64_t num_columns; /* real columns Cr */
    int64_t batch_size;
    double alpha;        /* splitting parameter, > 0 */
    double r_cut;        /* in (0, min_a w_a / 3] */
    double box[6];       /* A00, A10, A11, A20, A21, A22 */
} nfft_hip_ewald_box_problem;
int64_t nfft_hip_ewald_box_cells(const double *box, double r_cut, int64_t batch_size, int32_t *cells_out);
int64_t nfft_hip_ewald_near_box_workspace_bytes(const nfft_hip_ewald_box_problem *p);
int nfft_hip_ewald_near_box(const nfft_hip_ewald_box_problem *p, const float *points, const float *xr,
                            const int32_t *start, const int64_t *index, float *z, float *field, void *workspace,
                            int64_t workspace_bytes, void *stream);

/* ---- near part of the dispersion Ewald sum, the periodic 1/r^6 (no reference counterpart) ----
 * The sum of c_j / r^6 over all images is split with a = alpha r: the smooth part is summed on the whole torus with
 * nfft_hip_fastsum (coefficients pi^(3/2) alpha^3 f(b) / (3 V), b = pi |kappa| / alpha, f(b) = (1 - 2 b^2) exp(-b^2) +
 * 2 sqrt(pi) b^3 erfc(b), k = 0 included, set up by the host side), and these two entry points add the short-ranged rest:
 *     z[i, c]        = sum_{j in the point set of i, 0 < r_ij < r_cut} exp(-a^2) (1 + a^2 + a^4 / 2) / r_ij^6  xr[j, c]
 *     field[i, a, c] = sum_j exp(-a^2) (6 + 6 a^2 + 3 a^4 + a^6) / r_ij^8  d_ij[a] xr[j, c]   (with_field = 1; minus the gradient)
 * on the unit torus and in a box.  Problem structs, arguments, the order of the points, validation, error codes and
 * determinism are EXACTLY those of nfft_hip_ewald_near and nfft_hip_ewald_near_box, and so is the workspace: there are no
 * cell or workspace functions of their own, nfft_hip_ewald_near_cells / nfft_hip_ewald_near_workspace_bytes and
 * nfft_hip_ewald_box_cells / nfft_hip_ewald_near_box_workspace_bytes serve both sweeps.  In float32 1 / r^8 overflows below
 * r ~ 1.6e-5: closer pairs give inf. */
int nfft_hip_ewald_dispersion_near(const nfft_hip_ewald_problem *p, const float *points, const float *xr,
                                   const int32_t *start, const int64_t *index, float *z, float *field, void *workspace,
                                   int64_t workspace_bytes, void *stream);
int nfft_hip_ewald_dispersion_near_box(const nfft_hip_ewald_box_problem *p, const float *points, const float *xr,
                                       const int32_t *start, const int64_t *index, float *z, float *field, void *workspace,
                                       int64_t workspace_bytes, void *stream);

/* ---- virial tensor of the Ewald sum (no reference counterpart) ----
 * For the homogeneous strain A -> A (1 + eps) at fixed fractional coordinates the virial W_ab = -dU / d eps_ab of the
 * energy U = 1/2 sum_i q_i phi_i is a pair sum, a sum over the frequencies and a background term.  These two entry points
 * give the first two, each with its share of the energy in front: seven numbers per point set and column, in the order
 *     energy, xx, yy, zz, yz, xz, xy,
 * in float64 [batch_size, 7, columns].  The background term -pi Q^2 / (2 alpha^2 V) delta_ab and the self term are the
 * caller's.  Real data only: the energy is bilinear, and for complex charges it is not |S_k|^2 that enters.
 *
 * nfft_hip_ewald_virial_near: points, xr and start as for nfft_hip_ewald_near_box (fractional, reduced to [-1/2, 1/2)^3,
 * ordered by cell; with_field is not used and must be 0 or 1),
 *     out[b, 0, c] = 1/2 sum_{i in set b} xr[i, c] sum_{j: 0 < r_ij < r_cut} erfc(alpha r_ij) / r_ij  xr[j, c]
 *     out[b, e, c] = 1/2 sum_i xr[i, c] sum_j (-g(r_ij^2)) d_ij[a] d_ij[b] xr[j, c]
 * with g and d_ij as above.  The unit cube is the box 1, 0, 1, 0, 0, 1.  num_columns < 2^21 and batch_size * num_columns
 * < 2^31 are required.  With no points the output is set to zero; with no
 * columns nothing is done.
 *
 * nfft_hip_ewald_virial_far: band [batch_size, N, N, N, num_columns] complex64 (the adjoint transform of the charges,
 * index k + N/2), coeffs [N, N, N] float32 (b_k; cells with b_k = 0 are skipped), box_inverse[6] = the lower triangle
 * I00, I10, I11, I20, I21, I22 of A^-1 (kappa = A^-1 k), pi2_over_alpha2 = pi^2 / alpha^2,
 *     out[b, 0, c] = 1/2 sum_k b_k |band_k|^2
 *     out[b, e, c] = 1/2 sum_k b_k |band_k|^2 (delta_ab - 2 (1 / |kappa|^2 + pi^2 / alpha^2) kappa_a kappa_b).
 * band needs the 8-byte alignment of complex64 only; when it is 16-byte aligned, cells of two or four columns are read
 * with 16-byte loads.  N even, 2 <= N <= 2048; 1 <= batch_size < 2^14 and batch_size * num_columns < 2^21.
 *
 * Both reduce in two levels (one partial per work item or workgroup in the workspace, then one workgroup per point set and
 * column), in float64 and without atomics: two calls give the same bits. */
int64_t nfft_hip_ewald_virial_near_workspace_bytes(const nfft_hip_ewald_box_problem *p);
int nfft_hip_ewald_virial_near(const nfft_hip_ewald_box_problem *p, const float *points, const float *xr,
                               const int32_t *start, double *out, void *workspace, int64_t workspace_bytes, void *stream);
int64_t nfft_hip_ewald_virial_far_workspace_bytes(int64_t N, int64_t batch_size, int64_t num_columns);
int nfft_hip_ewald_virial_far(int64_t N, int64_t batch_size, int64_t num_columns, const void *band, const float *coeffs,
                              const double *box_inverse, double pi2_over_alpha2, double *out, void *workspace,
                              int64_t workspace_bytes, void *stream);

/* ---- virial tensor of the dispersion Ewald sum (no reference counterpart) ----
 * The same two reductions for the periodic 1/r^6 of nfft_hip_ewald_dispersion_near_box: U = 1/2 sum_i c_i psi_i and
 * W_ab = -dU / d eps_ab, seven float64 numbers per point set and column in the order above.  The self term
 * -(alpha^6 / 12) sum_i c_i^2 (in U only) is the caller's; there is no background term.  tr W = 6 U for the converged sum.
 * Arguments, checks, alignment and limits are those of the two entry points above, and so are the workspaces:
 * nfft_hip_ewald_virial_near_workspace_bytes and nfft_hip_ewald_virial_far_workspace_bytes serve both.
 *
 * nfft_hip_ewald_dispersion_virial_near: with a = alpha r, w = exp(-a^2) (1 + a^2 + a^4 / 2) / r^6 and mg = -w'(r) / r,
 *     out[b, 0, c] = 1/2 sum_{i in set b} xr[i, c] sum_{j: 0 < r_ij < r_cut} w(r_ij) xr[j, c]
 *     out[b, e, c] = 1/2 sum_i xr[i, c] sum_j mg(r_ij) d_ij[a] d_ij[b] xr[j, c].
 *
 * nfft_hip_ewald_dispersion_virial_far: coeffs [N, N, N] float32 holds b_k (k = 0 included; cells with b_k = 0 are
 * skipped) and strain_coeffs [N, N, N] float32 holds t_k = (d b_k / d |kappa|) / |kappa| = (2 pi^(7/2) alpha / V)
 * (sqrt(pi) b erfc(b) - exp(-b^2)), b = pi |kappa| / alpha, which the caller evaluates in float64 (the two terms cancel
 * at large b),
 *     out[b, 0, c] = 1/2 sum_k b_k |band_k|^2
 *     out[b, e, c] = 1/2 sum_k |band_k|^2 (b_k delta_ab + t_k kappa_a kappa_b). */
int nfft_hip_ewald_dispersion_virial_near(const nfft_hip_ewald_box_problem *p, const float *points, const float *xr,
                                          const int32_t *start, double *out, void *workspace, int64_t workspace_bytes,
                                          void *stream);
int nfft_hip_ewald_dispersion_virial_far(int64_t N, int64_t batch_size, int64_t num_columns, const void *band,
                                         const float *coeffs, const float *strain_coeffs, const double *box_inverse, double *out,
                                         void *workspace, int64_t workspace_bytes, void *stream);

/* ---- potential, field, energy and virial of the Ewald sum in one pass (no reference counterpart) ----
 * What one constant-pressure step needs from the sum, without doing the walk over the pairs and the pass over the
 * spectrum twice: nfft_hip_ewald_near_box with with_field = 1 and nfft_hip_ewald_virial_near in one pair kernel, and the
 * coefficient product of the field's far part and nfft_hip_ewald_virial_far in one spectral kernel.  The sums, the order
 * energy, xx, yy, zz, yz, xz, xy of the seven numbers, the checks, limits, error codes and workspaces are those of the
 * Coulomb sum's entry points above (section 7i): nfft_hip_ewald_step_near_workspace_bytes returns what
 * nfft_hip_ewald_virial_near_workspace_bytes does and nfft_hip_ewald_step_spectral_workspace_bytes what
 * nfft_hip_ewald_virial_far_workspace_bytes does.  Real data only.
 *
 * nfft_hip_ewald_step_near: points, xr, start and index as for nfft_hip_ewald_near_box (with_field is not used and must be
 * 0 or 1; the unit cube is the box 1, 0, 1, 0, 0, 1),
 *     z[index[i], c]    = sum_{j: 0 < r_ij < r_cut} erfc(alpha r_ij) / r_ij  xr[j, c]              float32 [points, columns]
 *     f[index[i], a, c] = sum_j (-g(r_ij^2)) d_ij[a] xr[j, c]                                       float32 [points, 3, columns]
 *     out7[b, 0, c]     = 1/2 sum_{i in set b} xr[i, c] (the sum of z)                             float64 [batch_size, 7, columns]
 *     out7[b, e, c]     = 1/2 sum_i xr[i, c] sum_j (-g(r_ij^2)) d_ij[a] d_ij[b] xr[j, c],
 * the ten sums of a point and column kept side by side in float32 over one walk.  With no points out7 is set to zero;
 * with no columns nothing is done.
 *
 * nfft_hip_ewald_step_spectral: band, coeffs, box_inverse and pi2_over_alpha2 as for nfft_hip_ewald_virial_far; it
 * writes spectra [batch_size, N, N, N, 4, num_columns] complex64,
 *     spectra[.., 0, c] = b_k band[.., c],   spectra[.., 1 + a, c] = 2 pi i kappa_a b_k band[.., c]
 * (zeros where b_k = 0; 2 pi kappa is formed in float32 from the float64 box_inverse), whose forward transform is the far
 * part of (phi, E) with the signs of the transforms, and out7 as nfft_hip_ewald_virial_far from the same read of band.
 * band and spectra need the 8-byte alignment of complex64 only; when both are 16-byte aligned, cells of one, two or four
 * columns move in 16-byte pieces.
 *
 * Two levels, float64 and no atomics as above: two calls give the same bits. */
int64_t nfft_hip_ewald_step_near_workspace_bytes(const nfft_hip_ewald_box_problem *p);
int nfft_hip_ewald_step_near(const nfft_hip_ewald_box_problem *p, const float *points, const float *xr, const int32_t *start,
                             const int64_t *index, float *z, float *f, double *out7, void *workspace, int64_t workspace_bytes,
                             void *stream);
int64_t nfft_hip_ewald_step_spectral_workspace_bytes(int64_t N, int64_t batch_size, int64_t num_columns);
int nfft_hip_ewald_step_spectral(int64_t N, int64_t batch_size, int64_t num_columns, const void *band, const float *coeffs,
                                 const double *box_inverse, double pi2_over_alpha2, void *spectra, double *out7, void *workspace,
                                 int64_t workspace_bytes, void *stream);

/* ---- forces, energies and virial of a Lennard-Jones + Coulomb model in one pass (no reference counterpart) ----
 * Point j carries a charge q_j, a dispersion coefficient c_j and a repulsion coefficient a_j, packed as xs [points, 3];
 * geometric mixing, C6_ij = c_i c_j and C12_ij = a_i a_j.  The energy is U = U_C + U_LJ with U_C the Coulomb Ewald sum
 * (alpha = p->alpha) and U_LJ = 1/2 sum_ij a_i a_j / r_ij^12 [r_ij < r_cut] minus the dispersion Ewald sum of c
 * (alpha = alpha_dispersion); both sums share r_cut, the box and the cells.  Real data, one column (p->num_columns must be 1).
 *
 * nfft_hip_ewald_lj_step_near: the nfft_hip_ewald_box_problem, the cell-ordered fractional points, start and index of
 * nfft_hip_ewald_step_near (with_field is not used and must be 0 or 1; the unit cube is the box 1, 0, 1, 0, 0, 1).  Over the
 * pairs 0 < r_ij < r_cut, with w_C, mg_C the Coulomb pair weights, w_D, mg_D the dispersion pair weights and
 * s_ij = q_i q_j mg_C - c_i c_j mg_D + 12 a_i a_j / r^14:
 *     f[index[i], a] = sum_j s_ij d_ij[a]                                                      float32 [points, 3]
 *     out8[b, 0]     = 1/2 sum_ij q_i q_j w_C                                                  float64 [batch_size, 8]
 *     out8[b, 1]     = 1/2 sum_ij (a_i a_j / r^12 - c_i c_j w_D)
 *     out8[b, 2 + e] = 1/2 sum_ij s_ij d_ij[a] d_ij[b],   e = 0 .. 5: ab = xx, yy, zz, yz, xz, xy
 * (f is the near part of the force itself: the lane's own coefficients are inside).  With no points out8 is set to zero.
 * Separations below 1.6e-5, or at which 12 a_i a_j / r^14 leaves float32, give values that are not numbers.
 *
 * nfft_hip_ewald_lj_step_spectral: band [batch_size, N, N, N, 2] complex64, the adjoint transform of the columns (q, c);
 * the float32 grids [N, N, N] coeffs_coulomb (b^C_k), coeffs_dispersion (b^D_k) and strain_dispersion (t^D_k, as for
 * nfft_hip_ewald_dispersion_virial_far); box_inverse and pi2_over_alpha2 (of the Coulomb alpha) as for
 * nfft_hip_ewald_virial_far.  It writes spectra [batch_size, N, N, N, 6] complex64,
 *     spectra[.., a] = 2 pi i kappa_a b^C_k band[.., 0],   spectra[.., 3 + a] = 2 pi i kappa_a b^D_k band[.., 1]
 * (zeros where the table is zero; 2 pi kappa in float32), whose forward transform is the far part of (E, G), and
 *     out8[b, 0] = 1/2 sum_k b^C_k |S^q_k|^2,   out8[b, 1] = -1/2 sum_k b^D_k |S^c_k|^2,
 *     out8[b, 2 + e] = the terms of nfft_hip_ewald_virial_far minus those of nfft_hip_ewald_dispersion_virial_far.
 * band and spectra need the 8-byte alignment of complex64 only; when both are 16-byte aligned a cell moves in 16-byte pieces.
 *
 * Checks, limits and error codes are those of the Coulomb step's entry points; the *_workspace_bytes functions return -1 for
 * a problem that would be refused.  Two levels, float64 and no atomics: two calls give the same bits. */
int64_t nfft_hip_ewald_lj_step_near_workspace_bytes(const nfft_hip_ewald_box_problem *p, double alpha_dispersion);
int nfft_hip_ewald_lj_step_near(const nfft_hip_ewald_box_problem *p, double alpha_dispersion, const float *points, const float *xs,
                                const int32_t *start, const int64_t *index, float *f, double *out8, void *workspace,
                                int64_t workspace_bytes, void *stream);
int64_t nfft_hip_ewald_lj_step_spectral_workspace_bytes(int64_t N, int64_t batch_size);
int nfft_hip_ewald_lj_step_spectral(int64_t N, int64_t batch_size, const void *band, const float *coeffs_coulomb,
                                    const float *coeffs_dispersion, const float *strain_dispersion, const double *box_inverse,
                                    double pi2_over_alpha2, void *spectra, double *out8, void *workspace, int64_t workspace_bytes,
                                    void *stream);

/* ---- the same step with bonded-pair exclusions (no reference counterpart) ----
 * The list is the CSR matrix of nfft_hip_ewald_excl over the points in the CALLER's order: row_start int32 [points + 1], col
 * int32 [num_entries] ascending within a row, weight_coulomb and weight_lj float32 [num_entries] holding w = 1 - s for the
 * Coulomb scale s^C and the Lennard-Jones scale s^L (both powers) of the pair.  Each listed pair {i, j} stands in both rows.
 *
 * nfft_hip_ewald_lj_excl_near: nfft_hip_ewald_lj_step_near with the terms of a listed pair SCALED before they are added:
 * q_i q_j by s^C, c_i c_j and a_i a_j by s^L (a pair with both scales zero adds nothing).  index must hold each point's
 * position in the caller's order, below 2^31.  With num_entries = 0, f and out8 have the bits of nfft_hip_ewald_lj_step_near.
 *
 * nfft_hip_ewald_lj_excl_list: points [points, 3] fractional, reduced to [-1/2, 1/2)^3 as the cell order reduces them, and xs
 * [points, 3], both in the CALLER's order; set_start int32 [batch_size + 1], the first point of every point set (may be null
 * for one point set).  With d the image of s_i - s_col[k] as the pair walk forms it, r = |d| and, for r < r_cut (r = 0
 * included), the smooth parts S_C = erf(alpha r) / r, T_C = -S_C' / r at p->alpha and S_D = 1 / r^6 - w_D, T_D = -S_D' / r at
 * alpha_dispersion -- for r >= r_cut the full 1 / r, 1 / r^3, 1 / r^6, 6 / r^8 -- and g = w^L c_i c_j T_D - w^C q_i q_j T_C:
 *     f[i, a]        = sum_{k in row i} g d[a]                                                  float32 [points, 3]
 *     out8[b, 0]     = -sum_{pairs} w^C q_i q_j S_C,   out8[b, 1] = sum_{pairs} w^L c_i c_j S_D     float64 [batch_size, 8]
 *     out8[b, 2 + e] = sum_{pairs} g d[a] d[b],   e = 0 .. 5: ab = xx, yy, zz, yz, xz, xy         (each pair once, col > row)
 * which are to be ADDED to the results of the walk.  Entries whose column lies outside [0, points) are skipped.
 *
 * Both take the checks of nfft_hip_ewald_lj_step_near and in addition refuse null list pointers (row_start always, the others
 * when num_entries > 0), a negative num_entries and one of 2^31 or more.  No atomics: two calls give the same bits. */
int64_t nfft_hip_ewald_lj_excl_near_workspace_bytes(const nfft_hip_ewald_box_problem *p, double alpha_dispersion);
int nfft_hip_ewald_lj_excl_near(const nfft_hip_ewald_box_problem *p, double alpha_dispersion, int64_t num_entries,
                                const float *points, const float *xs, const int32_t *start, const int64_t *index,
                                const int32_t *row_start, const int32_t *col, const float *weight_coulomb, const float *weight_lj,
                                float *f, double *out8, void *workspace, int64_t workspace_bytes, void *stream);
int64_t nfft_hip_ewald_lj_excl_list_workspace_bytes(const nfft_hip_ewald_box_problem *p, double alpha_dispersion);
int nfft_hip_ewald_lj_excl_list(const nfft_hip_ewald_box_problem *p, double alpha_dispersion, int64_t num_entries,
                                const float *points, const float *xs, const int32_t *row_start, const int32_t *col,
                                const float *weight_coulomb, const float *weight_lj, const int32_t *set_start, float *f,
                                double *out8, void *workspace, int64_t workspace_bytes, void *stream);

/* ---- the same walk with per-type-pair Lennard-Jones parameters (no reference counterpart) ----
 * For force fields whose C6_ij and C12_ij are not products of per-point numbers (Lorentz-Berthelot mixing, fitted cross
 * terms).  Point j carries a charge q_j and the coefficient c_j that the GRID sees, packed as xs [points, 2], and a type
 * types[j] in [0, num_types), int32 [points]; xs and types in the cell order of `points`.  table is float32
 * [num_types, num_types, 2] = (C12(t, t'), dC6(t, t')), symmetric in (t, t'), where dC6 is what the pair's C6 has above the
 * product c_i c_j that the far field carries.  A type outside [0, num_types) is clamped into it: nothing is read outside
 * the table.  With w_C, mg_C, w_D, mg_D as for nfft_hip_ewald_lj_step_near, over the pairs 0 < r_ij < r_cut and
 * s_ij = q_i q_j mg_C - c_i c_j mg_D + 12 C12 / r^14 - 6 dC6 / r^8:
 *     f[index[i], a] = sum_j s_ij d_ij[a]                                                      float32 [points, 3]
 *     out8[b, 0]     = 1/2 sum_ij q_i q_j w_C                                                  float64 [batch_size, 8]
 *     out8[b, 1]     = 1/2 sum_ij (C12 / r^12 - dC6 / r^6 - c_i c_j w_D)
 *     out8[b, 2 + e] = 1/2 sum_ij s_ij d_ij[a] d_ij[b],   e = 0 .. 5: ab = xx, yy, zz, yz, xz, xy
 * The list (row_start, col, weight_coulomb, weight_lj, num_entries) is that of nfft_hip_ewald_lj_excl_near: a listed pair's
 * q_i q_j is scaled by s^C and its c_i c_j, C12 and dC6 by s^L before they are added, and nfft_hip_ewald_lj_excl_list on
 * (q, c, 0) removes the far field's share.  All four list pointers null and num_entries = 0: no list, and a kernel that
 * holds no list code; with a list of no entries the bits are the same.  Separations below 1.6e-5, or at which
 * 12 C12 / r^14 or 6 dC6 / r^8 leaves float32, give values that are not numbers.
 *
 * Checks, limits, error codes and the workspace are those of nfft_hip_ewald_lj_excl_near; in addition num_types outside
 * [1, 32], a null table, a table that is not 8-byte aligned (an entry moves as one load) and list pointers without row_start
 * are refused ("Input mismatch").  With no points out8 is set to zero.  No atomics: two calls give the same bits. */
int64_t nfft_hip_ewald_lj_table_near_workspace_bytes(const nfft_hip_ewald_box_problem *p, double alpha_dispersion);
int nfft_hip_ewald_lj_table_near(const nfft_hip_ewald_box_problem *p, double alpha_dispersion, int64_t num_types, int64_t num_entries,
                                 const float *points, const float *xs, const int32_t *types, const float *table,
                                 const int32_t *start, const int64_t *index, const int32_t *row_start, const int32_t *col,
                                 const float *weight_coulomb, const float *weight_lj, float *f, double *out8, void *workspace,
                                 int64_t workspace_bytes, void *stream);

/* ---- the same walk for Buckingham / Born-Mayer-Huggins pair potentials (no reference counterpart) ----
 * For force fields whose repulsion is an exponential (Tosi-Fumi alkali halides, BKS silica, ionic ceramics).  The argument
 * list, xs [points, 2] = (q, c), types, the list and every output are those of nfft_hip_ewald_lj_table_near; table is float32
 * [num_types, num_types, 4] = (A(t, t'), B(t, t'), dC6(t, t'), C8(t, t')), symmetric in (t, t'), for the pair energy
 * A e^(-B r) - C6 / r^6 - C8 / r^8 (B = 1 / rho; attractions enter with positive C6, C8) with dC6 what the pair's C6 has above
 * the product c_i c_j that the far field carries.  Over the pairs 0 < r_ij < r_cut, plainly truncated, and with
 * s_ij = q_i q_j mg_C - c_i c_j mg_D + A B e^(-B r) / r - 6 dC6 / r^8 - 8 C8 / r^10:
 *     f[index[i], a] = sum_j s_ij d_ij[a]                                                      float32 [points, 3]
 *     out8[b, 0]     = 1/2 sum_ij q_i q_j w_C                                                  float64 [batch_size, 8]
 *     out8[b, 1]     = 1/2 sum_ij (A e^(-B r) - dC6 / r^6 - C8 / r^8 - c_i c_j w_D)
 *     out8[b, 2 + e] = 1/2 sum_ij s_ij d_ij[a] d_ij[b],   e = 0 .. 5: ab = xx, yy, zz, yz, xz, xy
 * A listed pair's q_i q_j is scaled by s^C and its c_i c_j, A, dC6 and C8 by s^L before they are added.  With c = 0 (no
 * dispersion on the grid) the terms in c_i c_j are exact zeros and alpha_dispersion only has to be valid.  A type outside
 * [0, num_types) is clamped.  Separations below 1.6e-5, or at which 6 dC6 / r^8 or 8 C8 / r^10 leaves float32, give values that
 * are not numbers; the exponential term is finite everywhere.
 *
 * Checks, limits, error codes and the workspace are those of nfft_hip_ewald_lj_table_near, except that table must be
 * 16-byte aligned (an entry moves as one load).  No atomics: two calls give the same bits. */
int64_t nfft_hip_ewald_bmh_table_near_workspace_bytes(const nfft_hip_ewald_box_problem *p, double alpha_dispersion);
int nfft_hip_ewald_bmh_table_near(const nfft_hip_ewald_box_problem *p, double alpha_dispersion, int64_t num_types, int64_t num_entries,
                                  const float *points, const float *xs, const int32_t *types, const float *table,
                                  const int32_t *start, const int64_t *index, const int32_t *row_start, const int32_t *col,
                                  const float *weight_coulomb, const float *weight_lj, float *f, double *out8, void *workspace,
                                  int64_t workspace_bytes, void *stream);

/* ---- Ewald sum of point charges and point dipoles (no reference counterpart) ----
 * Source j carries a charge q_j and a Cartesian dipole mu_j, packed as xs [points, 4, num_columns] = (q, mu_x, mu_y, mu_z).
 * With d = d_ij, r = |d|, m = mu_j . d and the Smith functions B_0 = erfc(alpha r) / r,
 * B_l = ((2l - 1) B_(l-1) + (2 alpha^2)^l / (alpha sqrt(pi)) exp(-alpha^2 r^2)) / r^2, the two near entry points give, over the
 * pairs 0 < r_ij < r_cut of one point set,
 *     phi[i]     = sum_j q_j B_0 + m B_1
 *     E[i, a]    = sum_j (q_j B_1 + m B_2) d_a - mu_j,a B_1                                        (E = -grad phi)
 *     T[i, a, b] = sum_j q_j (delta_ab B_1 - d_a d_b B_2) + (mu_j,a d_b + mu_j,b d_a + m delta_ab) B_2 - m d_a d_b B_3
 * (T_ab = d E_a / d x_b) as out [points, 4, num_columns] = (phi, E_x, E_y, E_z) for order = 1 and out [points, 10,
 * num_columns] for order = 2, T following in the order xx, yy, zz, yz, xz, xy; rows in the caller's order through index.
 * Problem structs (num_columns counts the columns of four values; with_field must be 0 or 1 and is otherwise not read),
 * the order of the points, validation, error codes, determinism and workspace are those of nfft_hip_ewald_near and
 * nfft_hip_ewald_near_box: nfft_hip_ewald_near_workspace_bytes and nfft_hip_ewald_near_box_workspace_bytes serve these
 * sweeps too.  order must be 1 or 2 ("Input mismatch").
 *
 * nfft_hip_ewald_dipole_spectral: band [batch_size, N, N, N, 4, num_columns] complex64 (the adjoint transform of xs, index
 * k + N/2), coeffs [N, N, N] float32 (b_k), box_inverse[6] = the lower triangle I00, I10, I11, I20, I21, I22 of A^-1
 * (kappa = A^-1 k; the unit cube: 1, 0, 1, 0, 0, 1).  With rho_k = band_q + 2 pi i kappa . band_mu and R = b_k rho_k it writes
 * out [batch_size, N, N, N, 4 or 10, num_columns] complex64,
 *     out[.., 0] = R,   out[.., 1 + a] = 2 pi i kappa_a R,   out[.., 4 + e] = 4 pi^2 kappa_a kappa_b R   (order = 2),
 * whose forward transform is the far part of (phi, E, T): the signs are those of the transforms (the adjoint sums
 * exp(+2 pi i k.s), the forward exp(-2 pi i k.s)).  2 pi kappa is formed in float32 from the float64 box_inverse.  One
 * pass, no workspace.  N even, 2 <= N <= 2048, 1 <= batch_size < 2^14, 0 <= num_columns < 2^21, N^3 num_columns < 2^31. */
int nfft_hip_ewald_dipole_near(const nfft_hip_ewald_problem *p, const float *points, const float *xs, const int32_t *start,
                               const int64_t *index, int32_t order, float *out, void *workspace, int64_t workspace_bytes,
                               void *stream);
int nfft_hip_ewald_dipole_near_box(const nfft_hip_ewald_box_problem *p, const float *points, const float *xs,
                                   const int32_t *start, const int64_t *index, int32_t order, float *out, void *workspace,
                                   int64_t workspace_bytes, void *stream);
int nfft_hip_ewald_dipole_spectral(int64_t N, int64_t batch_size, int64_t num_columns, int32_t order, const void *band,
                                   const float *coeffs, const double *box_inverse, void *out, void *stream);

/* ---- Periodic Stokeslet sum, Hasimoto's Ewald sum (no reference counterpart) ----
 * Source j carries a Cartesian force f_j, xs [points, 3, num_columns].  With d = d_ij, r = |d|, m = d . f_j, the Smith functions
 * B_0, B_1, B_2 of the dipole sum above and g = (2 alpha / sqrt(pi)) exp(-alpha^2 r^2), the two near entry points give, over the
 * pairs 0 < r_ij < r_cut of one point set,
 *     u[i, a]    = sum_j (B_0 - g) f_j,a + B_1 m d_a
 *     G[i, a, b] = sum_j (2 alpha^2 g - B_1) f_j,a d_b + B_1 (d_a f_j,b + m delta_ab) - B_2 m d_a d_b        (G_ab = d u_a / d x_b)
 * as out [points, 3, num_columns] for order = 1 and out [points, 12, num_columns] for order = 2, G following row-major in ab
 * (it is not symmetric; its trace is zero); rows in the caller's order through index.  Problem structs (num_columns counts
 * the columns of three values; with_field must be 0 or 1 and is otherwise not read), the order of the points, validation,
 * error codes, determinism and workspace are those of nfft_hip_ewald_near and nfft_hip_ewald_near_box:
 * nfft_hip_ewald_near_workspace_bytes and nfft_hip_ewald_near_box_workspace_bytes serve these sweeps too.  order must be 1 or
 * 2 ("Input mismatch").
 *
 * nfft_hip_ewald_stokeslet_spectral: band [batch_size, N, N, N, 3, num_columns] complex64 (the adjoint transform of xs, index
 * k + N/2), coeffs [N, N, N] float32 (c_k = 2 b_k (1 + pi^2 |kappa|^2 / alpha^2)), box_inverse[6] = the lower triangle of A^-1 as
 * for nfft_hip_ewald_dipole_spectral.  With tau = 2 pi kappa and rho the three rows of band it writes
 * out [batch_size, N, N, N, 3 or 12, num_columns] complex64,
 *     U = c_k (rho - tau (tau . rho) / |tau|^2),   out[.., a] = U_a,   out[.., 3 + 3 a + b] = -i tau_b U_a   (order = 2),
 * the quotient taken as 0 where |tau|^2 = 0, whose forward transform is the far part of (u, G): the signs are those of the
 * transforms (the adjoint sums exp(+2 pi i k.s), the forward exp(-2 pi i k.s), whose derivative along x_b is -i tau_b).
 * tau is formed in float32 from the float64 box_inverse.  One pass, no workspace.  Limits as for the dipole sum's. */
int nfft_hip_ewald_stokeslet_near(const nfft_hip_ewald_problem *p, const float *points, const float *xs, const int32_t *start,
                                  const int64_t *index, int32_t order, float *out, void *workspace, int64_t workspace_bytes,
                                  void *stream);
int nfft_hip_ewald_stokeslet_near_box(const nfft_hip_ewald_box_problem *p, const float *points, const float *xs,
                                      const int32_t *start, const int64_t *index, int32_t order, float *out, void *workspace,
                                      int64_t workspace_bytes, void *stream);
int nfft_hip_ewald_stokeslet_spectral(int64_t N, int64_t batch_size, int64_t num_columns, int32_t order, const void *band,
                                      const float *coeffs, const double *box_inverse, void *out, void *stream);

/* ---- Periodic Rotne-Prager-Yamakawa sum, Beenakker's Ewald sum (no reference counterpart) ----
 * Source j is a sphere of the radius `radius` (one per call) with a Cartesian force f_j, xs [points, 3, num_columns].  The
 * tensor is (1 + (a^2 / 3) lap) S(d) of the Stokeslet S above for r >= 2 a and (4 / (3 a)) ((1 - 9 r / (32 a)) I + 3 d d^T / (32 a r))
 * for overlapping spheres.  With q = a^2 / 3 and B_l, g as above the two entry points give, over the pairs 0 < r_ij < r_cut of
 * one point set,
 *     u[i, a]    = sum_j W1 f_j,a + W2 m d_a
 *     G[i, a, b] = sum_j D1 f_j,a d_b + D2 m d_a d_b + W2 (m delta_ab + d_a f_j,b)                          (G_ab = d u_a / d x_b)
 *     W1 = (B_0 - g) + q (2 B_1 + (8 alpha^2 - 4 alpha^4 r^2) g)                    W2 = B_1 + q (4 alpha^4 g - 2 B_2)
 *     D1 = (2 alpha^2 g - B_1) + q (-2 B_2 + (8 alpha^6 r^2 - 24 alpha^4) g)            D2 = -B_2 + q (2 B_3 - 8 alpha^6 g)
 * and for r < 2 a these plus the difference of the overlap form and the unscreened tensor.  Coincident points (r = 0) do
 * not see each other; the sphere's own mobility 4 / (3 a) is the caller's self term.  Output, problem structs, the order of
 * the points, validation, error codes, determinism and workspace are those of nfft_hip_ewald_stokeslet_near and
 * nfft_hip_ewald_stokeslet_near_box; in addition radius must be finite and positive with 2 radius <= r_cut ("Input mismatch").
 * The far part is nfft_hip_ewald_stokeslet_spectral with the coefficients c_k (1 - (a^2 / 3) |tau|^2). */
int nfft_hip_ewald_rpy_near(const nfft_hip_ewald_problem *p, const float *points, const float *xs, const int32_t *start,
                            const int64_t *index, int32_t order, double radius, float *out, void *workspace,
                            int64_t workspace_bytes, void *stream);
int nfft_hip_ewald_rpy_near_box(const nfft_hip_ewald_box_problem *p, const float *points, const float *xs, const int32_t *start,
                                const int64_t *index, int32_t order, double radius, float *out, void *workspace,
                                int64_t workspace_bytes, void *stream);

/* ---- Bonded-pair exclusions of the Coulomb and dispersion Ewald sums (no reference counterpart) ----
 * What a list of unordered pairs {i, j} of one point set takes back out of nfft_hip_ewald_near (kind 0) or
 * nfft_hip_ewald_dispersion_near (kind 1) plus their far fields.  The list is symmetric and sorted, in CSR form over the
 * points IN THE CALLER'S ORDER (no cell order, no index array):
 *   points    [n, 3] float32, reduced to [-1/2, 1/2)^3 exactly as for the sweeps (fractional for the box entry point)
 *   xr        [n, Cr] float32 real columns
 *   row_start int32 [n + 1], col int32 [num_entries], weight float32 [num_entries] = 1 - scale of the pair
 *     z[i, c]        = sum_{k in row i} weight[k] K0(r) xr[col[k], c]           K0 = 1 / r (kind 0), 1 / r^6 (kind 1)
 *     field[i, a, c] = sum_{k in row i} weight[k] K1(r) d[a] xr[col[k], c]      K1 = 1 / r^3,        6 / r^8
 * with d the minimum image of points_i - points_col[k], formed by the very routine of the sweeps (the same bits), r = |d|.
 * An entry at r = 0 gives K0 = 2 alpha / sqrt(pi) (kind 0) or alpha^6 / 6 (kind 1), the limit of the smooth part, and no
 * field.  The caller SUBTRACTS z and field from the sums.  field [n, 3, Cr] is written with with_field = 1 only.  Entries
 * whose column lies outside [0, n) are skipped.  No atomics, a row is added in its order: two calls give the same bits.
 * No workspace.  Validation ("Input mismatch...") before any device access: null pointers, negative counts,
 * num_points and num_entries < 2^31, kind 0 or 1, with_field 0 or 1, alpha finite and positive, batch_size >= 1, and for the
 * box entry points a finite box with a positive diagonal (nfft_hip_ewald_excl does not read box).
 *
 * nfft_hip_ewald_excl_virial: the listed pairs' share of the energy and the virial of nfft_hip_ewald_virial_near /
 * nfft_hip_ewald_dispersion_virial_near, each pair once, in their order (energy, xx, yy, zz, yz, xz, xy), float64
 * [batch_size, 7, Cr]:
 *     out[b, 0, c] = sum_{pairs of set b} weight K0(r) xr[i, c] xr[j, c]
 *     out[b, e, c] = sum_{pairs of set b} weight K1(r) d[a] d[b] xr[i, c] xr[j, c]          (r = 0: the energy only)
 * in the box `box` (the unit cube is 1, 0, 1, 0, 0, 1).  set_start int32 [batch_size + 1]: the first point of every point
 * set (the points are sorted by point set); null with batch_size = 1.  Two levels in float64 without atomics, as
 * nfft_hip_ewald_virial_near; num_columns < 2^21 and batch_size * num_columns < 2^21 are required.  With no points or no
 * entries the output is set to zero; with no columns nothing is done. */
#define NFFT_HIP_EXCL_COULOMB 0
#define NFFT_HIP_EXCL_DISPERSION 1
typedef struct nfft_hip_ewald_excl_problem {
    int32_t kind;        /* NFFT_HIP_EXCL_* */
    int32_t with_field;  /* 0: z only; 1: z and field (not used by the virial) */
    int64_t num_points;
    int64_t num_columns; /* real columns Cr */
    int64_t num_entries; /* entries of col and weight: twice the number of pairs */
    int64_t batch_size;  /* point sets (the virial's output rows) */
    double alpha;        /* splitting parameter, > 0 */
    double box[6];       /* A00, A10, A11, A20, A21, A22 */
} nfft_hip_ewald_excl_problem;
int nfft_hip_ewald_excl(const nfft_hip_ewald_excl_problem *p, const float *points, const float *xr, const int32_t *row_start,
                        const int32_t *col, const float *weight, float *z, float *field, void *stream);
int nfft_hip_ewald_excl_box(const nfft_hip_ewald_excl_problem *p, const float *points, const float *xr,
                            const int32_t *row_start, const int32_t *col, const float *weight, float *z, float *field,
                            void *stream);
int64_t nfft_hip_ewald_excl_virial_workspace_bytes(const nfft_hip_ewald_excl_problem *p);
int nfft_hip_ewald_excl_virial(const nfft_hip_ewald_excl_problem *p, const float *points, const float *xr,
                               const int32_t *row_start, const int32_t *col, const float *weight, const int32_t *set_start,
                               double *out, void *workspace, int64_t workspace_bytes, void *stream);

/* ---- Ewald sum of the screened Coulomb (Yukawa) potential exp(-lambda r) / r (no reference counterpart) ----
 * The sum of q_j exp(-lambda r) / r over all images is split with beta = lambda / (2 alpha): the smooth part is summed on the
 * whole torus with nfft_hip_fastsum (coefficients 4 pi exp(-K / (4 alpha^2)) / (V K), K = 4 pi^2 |kappa|^2 + lambda^2, k = 0
 * included unless the caller wants the one-component-plasma background; set up by the host side), and the first two entry
 * points add the short-ranged rest:
 *     z[i, c]        = sum_{j in the point set of i, 0 < r_ij < r_cut} w(r_ij) xr[j, c]
 *     field[i, a, c] = sum_j mg(r_ij) d_ij[a] xr[j, c]                    (with_field = 1; minus the gradient)
 *     w  = (P + M) / (2 r),   P = exp(lambda r) erfc(alpha r + beta),   M = exp(-lambda r) erfc(alpha r - beta)
 *     mg = -w'(r) / r = (w + lambda (M - P) / 2 + (2 alpha / sqrt(pi)) exp(-alpha^2 r^2 - beta^2)) / r^2
 * on the unit torus and in a box.  The third is the pair part of the virial of U = 1/2 sum_i q_i phi_i at fixed lambda,
 *     out[b, 0, c] = 1/2 sum_{i in set b} xr[i, c] sum_{j: 0 < r_ij < r_cut} w(r_ij) xr[j, c]
 *     out[b, e, c] = 1/2 sum_i xr[i, c] sum_j mg(r_ij) d_ij[a] d_ij[b] xr[j, c]        (xx, yy, zz, yz, xz, xy)
 * in float64 [batch_size, 7, columns]; the spectral part is nfft_hip_ewald_dispersion_virial_far with the grids b_k and
 * t_k = -8 pi^2 b_k (1 / (4 alpha^2) + 1 / K), and the self and background terms are the caller's.
 * Problem structs, arguments, the order of the points, validation, error codes, determinism and workspaces are EXACTLY those
 * of nfft_hip_ewald_near, nfft_hip_ewald_near_box and nfft_hip_ewald_virial_near, whose cell and workspace functions serve
 * these too.  In addition screening = lambda must be finite, >= 0 and at most 50 / r_cut ("Input mismatch: ... screening ...",
 * checked before anything else, also for an empty problem): past it exp(-lambda r_cut) / r_cut is below exp(-50) / r_cut and
 * float32 exponentials of lambda r run out of range at 88.  screening = 0 gives the Coulomb weights erfc(alpha r) / r. */
int nfft_hip_ewald_yukawa_near(const nfft_hip_ewald_problem *p, const float *points, const float *xr, const int32_t *start,
                               const int64_t *index, double screening, float *z, float *field, void *workspace,
                               int64_t workspace_bytes, void *stream);
int nfft_hip_ewald_yukawa_near_box(const nfft_hip_ewald_box_problem *p, const float *points, const float *xr,
                                   const int32_t *start, const int64_t *index, double screening, float *z, float *field,
                                   void *workspace, int64_t workspace_bytes, void *stream);
int nfft_hip_ewald_yukawa_virial_near(const nfft_hip_ewald_box_problem *p, const float *points, const float *xr,
                                      const int32_t *start, double screening, double *out, void *workspace,
                                      int64_t workspace_bytes, void *stream);

/* Coefficient set-up (csrc/cuda/kernel_coeffs.cu, drivers core_cuda.cu:855-1064).  Outputs are [N]^dim
 * arrays, index l + N/2 on every axis.
 *   gaussian_analytic_coeffs      float32:  prod_d sqrt(pi) sigma exp(-sigma^2 pi^2 l_d^2)      (kernel_coeffs.cu:6-30)
 *   interpolation_grid            float32 [N^dim, dim] (radial = 0) or [N^dim] norms (radial = 1)  (:76-123)
 *   gaussian_interpolated_coeffs  complex64: fftshift(FFT(ifftshift(K(k/N - 1/2)))) / N^dim, K Gaussian (p < 0) or
 *                                 Gaussian clipped outside radius 1/2 (p == 0); only p <= 0, eps == 0  (:33-73, :179-202)
 *   interpolated_kernel_coeffs    complex64: the same recipe on user samples (float32 or complex64)  (:126-202) */
int nfft_hip_gaussian_analytic_coeffs(double sigma, int64_t N, int32_t dim, float *coeffs, void *stream);
int nfft_hip_interpolation_grid(int64_t N, int32_t dim, int radial, float *grid, void *stream);
int64_t nfft_hip_coeffs_workspace_bytes(int64_t N, int32_t dim);
int nfft_hip_gaussian_interpolated_coeffs(double sigma, int64_t N, int32_t dim, int64_t p, double eps, void *coeffs,
                                          void *workspace, int64_t workspace_bytes, void *stream);
int nfft_hip_interpolated_kernel_coeffs(const void *grid_values, int values_are_complex, int64_t N, int32_t dim,
                                        void *coeffs, void *workspace, int64_t workspace_bytes, void *stream);

/* ---- measurement hooks (bench.py) ----
 * When enabled, nfft_hip_adjoint / nfft_hip_forward bracket each stage with HIP events recorded on the
 * caller's stream.  nfft_hip_profile_collect waits for the recorded events and returns, per stage, the
 * summed GPU time in milliseconds and the number of launches since the last collect.  Stage order:
 * 0 point plan (binning), 1 coefficient gather, 2 grid zero-fill, 3 spreading, 4 FFT, 5 roll-off, 6 interpolation,
 * 7 product with the kernel grid (nfft_hip_toeplitz_apply only).
 * The reference has no counterpart (it has no timers at all).
 * Two event records per stage cost 3-6 us of stream time each: ~70 us per adjoint + forward pair, which is 1-2 % of a
 * 10^7-point step but more than half of a 10^3-point one.  nfft_hip_profile_stages restricts the timers to the stages
 * whose bit is set (bit s = stage s; default: all), e.g. 1u << 3 times the spreading kernel alone. */
#define NFFT_HIP_NUM_STAGES 8
void nfft_hip_profile_enable(int enable);
void nfft_hip_profile_stages(unsigned stage_mask);
int nfft_hip_profile_collect(double *ms_per_stage, int64_t *launches_per_stage, int num_stages);

#ifdef __cplusplus
}
#endif
#endif /* NFFT_HIP_H */
