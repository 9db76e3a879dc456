// Internal launch interface between the C-ABI layer (api.hip) and the kernel files.
#pragma once
#include "../../include/nfft_hip.h"
#include "common.h"

namespace nfft {

// binning.hip
int launch_plan_points(const Geom &g, const PlanLayout &L, const float *pos, const int64_t *batch, int64_t n, int64_t B,
                       void *plan, hipStream_t stream);
// What launch_plan_points decides on the host for a plan of layout L: `one_level` (1-D / 2-D: the first level is the whole
// sort), `local_scan` (its scatter pass scans the table of counts itself), `fuse` (the second level may take the one-pass
// kernel; the device decides, sort2_route_kernel), the item count of the scan between the passes and which scan runs
// (0 none, 1 small_scan_kernel<4>, 2 small_scan_kernel<16>, 3 hipcub).
struct PlanDecisions {
    bool one_level, local_scan, fuse;
    int64_t scan_items;
    int scan_kind;
};
PlanDecisions plan_decisions(const Geom &g, const PlanLayout &L);
// Seal of a point plan: a 64-bit checksum of the points (and the batch vector) it was built from, left in the plan's seal
// block (common.h: PlanLayout::off_seal) by the pass that counts the points -- no pass of its own.  verify: recompute the
// checksum from the arrays as they are now into accumulator `slot` and raise kFaultStalePlan in the device's status
// block when it differs.
int launch_points_verify(const float *pos, const int64_t *batch, int64_t n, int dim, void *seal, int slot, hipStream_t stream);
// xs[c * n + slot] = xr[perm[slot] * cols + c]
int launch_gather_rows(const Geom &g, const PlanLayout &L, const void *plan, int64_t n, const float *xr, int64_t cols,
                       float *xs, hipStream_t stream);

// spread.hip: grid[p, :] += ... for local planes p in [0, nplanes); global plane plane0 + p = b * Cr + cr
int launch_spread(const Geom &g, const PlanLayout &L, const void *plan, const float *xr, const float *xs, int64_t n, int64_t Cr,
                  int64_t plane0, int64_t nplanes, float *grid, hipStream_t stream);

// spread_reg.hip: register-tile spreading for 3-D grids (no atomics; writes every cell of the planes, so the
// grid needs no zero-fill).  Same arguments as launch_spread.
bool spread_reg_supported(const Geom &g);
int launch_spread_reg(const Geom &g, const PlanLayout &L, const void *plan, const float *xs, int64_t n, int64_t Cr,
                      int64_t plane0, int64_t nplanes, float *grid, hipStream_t stream);

// spread_mfma.hip: matrix-core spreading for the wide 3-D tiling (g.wide)
bool spread_mfma_supported(const Geom &g);
// largest |x| per (point set, real column) plane -> xmax[B * Cr] (bit patterns): the kernel's operand scales.  Reads the
// caller's row-major [point][Cr] array; set boundaries come from the halo plan (the batch vector is sorted)
int launch_plane_absmax(const Geom &g_halo, const PlanLayout &L_halo, const void *plan_halo, const float *xr, int64_t n,
                        int64_t B, int64_t Cr, unsigned *xmax, hipStream_t stream);
// coefficients: xr (row-major [point][Cr], read through the index in the plan records) or, when xr == nullptr, xs (copy in
// plan order, planar, stride L.cap: gather_rows).  tickets: kTicketPlanes ints of the caller's workspace, the counters of
// the persistent launch over the plan's work list (range_items.h: next_work_item); nullptr: round robin.  The same for the
// matrix-core gathers below.
int launch_spread_mfma(const Geom &g, const PlanLayout &L, const void *plan, const float *xr, const float *xs,
                       const unsigned *xmax, int64_t n, int64_t Cr, int64_t plane0, int64_t nplanes, float *grid,
                       int *tickets, hipStream_t stream);

// interp.hip: yr[perm[slot] * Cr + cr] = sum over taps of grid[p, ...]
int launch_interp(const Geom &g, const PlanLayout &L, const void *plan, const float *grid, int64_t n, int64_t Cr,
                  int64_t plane0, int64_t nplanes, float *yr, hipStream_t stream);
// interp_grad.hip: gradient gather of the forward transform with respect to the points, on the halo plan of any tiling.
// part[(cr * n + i) * dim + u] = w[i * Cr + cr] * d/dpos[i, u] (interpolation of plane b * Cr + cr at point i); every
// (cr, i) of the planes [plane0, plane0 + nplanes) is written once.  grad_reduce: dpos[e] = sum_cr part[cr * len + e] in
// plane order (len = n * dim).
int launch_interp_grad(const Geom &g, const PlanLayout &L, const void *plan, const float *grid, int64_t n, int64_t Cr,
                       int64_t plane0, int64_t nplanes, const float *w, float *part, hipStream_t stream);
// The same gather that also writes the interpolated value yr[i * Cr + cr] of every (plane, point), as launch_interp does.
int launch_interp_value_grad(const Geom &g, const PlanLayout &L, const void *plan, const float *grid, int64_t n, int64_t Cr,
                             int64_t plane0, int64_t nplanes, const float *w, float *part, float *yr, hipStream_t stream);
int launch_grad_reduce(const float *part, int64_t len, int64_t Cr, float *dpos, hipStream_t stream);
// The backward of that gather for an upstream v [n, dim]: dw[i * Cr + cr] = sum_u v[i, u] d Fr / d pos[i, u]
// and part[(cr * n + i) * dim + b] = w[i * Cr + cr] sum_u v[i, u] d^2 Fr / d pos[i, u] d pos[i, b] (grad_reduce sums it);
// either output may be null (w is read only for part).
int launch_interp_hvp(const Geom &g, const PlanLayout &L, const void *plan, const float *grid, int64_t n, int64_t Cr,
                      int64_t plane0, int64_t nplanes, const float *w, const float *v, float *dw, float *part,
                      hipStream_t stream);
// spread.hip, the derivative spreading (the transpose of launch_interp_hvp's dw): grid planes
// [plane0, plane0 + nplanes) += xr[i * Cr + cr] prod psi (-2 c M) sum_u v[i, u] t_u; the halo plan of a narrow tiling only
bool spread_deriv_supported(const Geom &g);
int launch_spread_deriv(const Geom &g, const PlanLayout &L, const void *plan, const float *xr, const float *v, int64_t n,
                        int64_t Cr, int64_t plane0, int64_t nplanes, float *grid, hipStream_t stream);
// hvp_spectral.hip: u[i * Cr + j] = w[i * Cr + j] v[i * dim + a] (the adjoint's input of axis a), and
// dxhat (+)= 2 pi i k_a y (y: that adjoint's complex [B, N^dim, C]; the real part when dxhat is real)
int launch_hvp_stage(const float *w, const float *v, int64_t n, int64_t Cr, int dim, int a, float *u, hipStream_t stream);
int launch_hvp_combine(const void *y, int64_t B, int64_t N, int dim, int64_t C, int a, int accumulate, int out_complex,
                       void *dxhat, hipStream_t stream);
// matrix-core gather for the wide 3-D tiling (interp_mfma.hip)
bool interp_mfma_supported(const Geom &g);
int launch_interp_mfma(const Geom &g, const PlanLayout &L, const void *plan, const float *grid, int64_t n, int64_t Cr,
                       int64_t plane0, int64_t nplanes, float *yr, int *tickets, hipStream_t stream);

// streamed variant (interp_stream.hip): producer waves feed the plane ring, consumer waves pull blocks from a queue
bool interp_stream_supported(const Geom &g);
bool interp_stream_pays(const Geom &g, const PlanLayout &L, int64_t n);  // big work items only
int launch_interp_stream(const Geom &g, const PlanLayout &L, const void *plan, const float *grid, int64_t n, int64_t Cr,
                         int64_t plane0, int64_t nplanes, float *yr, int *tickets, hipStream_t stream);
// several coefficient columns per workgroup, one wave per column (interp_cols.hip): the point-side operands are built
// once for 8 columns, each wave streams its own column's planes from global memory
bool interp_cols_supported(const Geom &g);
int launch_interp_cols(const Geom &g, const PlanLayout &L, const void *plan, const float *grid, int64_t n, int64_t Cr,
                       int64_t plane0, int64_t nplanes, float *yr, int *tickets, hipStream_t stream);

// spectral.hip
// adjoint roll-off: spec = R2C(grid) per real plane [nplanes, M^(d-1) * (M/2+1)] complex -> y [B, N^d, C]
// mult / mult_kind: optional per-frequency factor [N^d] multiplied in on the way out (fastsum; 0 none, 1 float, 2 float2)
int launch_deconv_adjoint(const Geom &g, const float2 *spec, int64_t C, int x_is_complex, int real_output,
                          int64_t plane0, int64_t nplanes, void *y, const void *mult, int mult_kind, hipStream_t stream);
// forward roll-off: xhat [B, N^d, C] -> Hermitian half-spectra of the real planes of g
int launch_deconv_forward(const Geom &g, const void *xhat, int64_t C, int x_is_complex, int real_output,
                          int64_t plane0, int64_t nplanes, float2 *spec, hipStream_t stream);

// fft.cpp (rocFFT, plans cached per (kind, dim, M, batch) and device)
// kR2C / kC2R: full dim-dimensional real transforms of every plane; k*Rows: 1-D transforms of every grid row
// (last axis only), used together with the pruned column passes of colfft.hip
// kC2CForward: in-place complex forward transform of an N^dim array (coefficient set-up, coeffs.hip)
enum FftKind { kR2C = 0, kC2R = 1, kR2CRows = 2, kC2RRows = 3, kC2CForward = 4 };
int64_t fft_work_bytes(FftKind kind, int dim, int M, int64_t nplanes);
int fft_execute(FftKind kind, int dim, int M, int64_t nplanes, void *in, void *out, void *work, int64_t work_bytes,
                hipStream_t stream);

// colfft.hip: pruned strided passes over axes 1 and 0 fused with the roll-off (3-D, power-of-two M)
bool colfft_supported(const Geom &g);
int64_t colfft_scratch_bytes(const Geom &g, int64_t nplanes);
// `compact`: the axis-2 half spectrum holds only the N/2+1 kept columns per row (own row passes below) instead of
// rocFFT's M/2+1
int launch_colfft_adjoint(const Geom &g, const float2 *spec, bool compact, void *scratch, int64_t scratch_planes,
                          int64_t C, int x_is_complex, int real_output, int64_t plane0, int64_t nplanes, void *y,
                          const void *mult, int mult_kind, hipStream_t stream);
int launch_colfft_forward(const Geom &g, const void *xhat, void *scratch, int64_t scratch_planes, int64_t C,
                          int x_is_complex, int real_output, int64_t plane0, int64_t nplanes, float2 *spec, bool compact,
                          hipStream_t stream);
// Column-innermost pipeline for several coefficient columns (3-D, M = 128 .. 1024): the planes of a chunk travel in groups
// of 16 with the plane index innermost in both intermediate arrays, so the last adjoint pass writes (the first forward pass
// reads) the reference's [B, N^3, C] layout in place -- no planar copy, no transposes.  The buffers hold
// colfft_ci_planes(nplanes) planes (whole groups).  Row passes included.
bool colfft_ci_supported(const Geom &g);
int64_t colfft_ci_planes(int64_t nplanes);
int launch_row_r2c_ci(const Geom &g, const float *grid, int64_t nplanes, float2 *spec, hipStream_t stream);
int launch_row_c2r_ci(const Geom &g, const float2 *spec, int64_t nplanes, float *grid, hipStream_t stream);
int launch_colfft_adjoint_ci(const Geom &g, const float2 *spec, void *scratch, int64_t C, int x_is_complex,
                             int real_output, int64_t plane0, int64_t nplanes, void *y, const void *mult, int mult_kind,
                             hipStream_t stream);
int launch_colfft_forward_ci(const Geom &g, const void *xhat, float2 *spec, void *scratch, int64_t C, int x_is_complex,
                             int real_output, int64_t plane0, int64_t nplanes, hipStream_t stream);
// test support (api.hip nfft_dbg_fft_route): out[6] = {NC, 1 if a compile-time instantiation runs} of the adjoint's axis-1
// pass, of its axis-0 pass and of the forward passes for a chunk of nplanes planes (`ci`: the column-innermost launches)
void colfft_tile_widths(const Geom &g, bool compact, bool ci, int x_is_complex, int64_t nplanes, int32_t *out);
// planar [ncols][N^d] <-> column-interleaved [B, N^d, C] copies (tiled transposes) for the column passes with C > 1
int launch_column_layout(bool to_interleaved, const void *src, void *dst, int64_t K, int64_t C, int64_t col0,
                         int64_t ncols, int elem_bytes, hipStream_t stream);
// pruned real <-> half-complex row passes (axis 2), one wave per row; M in {128 .. 1024}
bool rowfft_supported(const Geom &g);
int launch_row_r2c(const Geom &g, const float *grid, void *scratch, int64_t scratch_planes, int64_t nplanes,
                   float2 *spec, hipStream_t stream);
int launch_row_c2r(const Geom &g, const float2 *spec, void *scratch, int64_t scratch_planes, int64_t nplanes,
                   float *grid, hipStream_t stream);

// toeplitz.hip (the normal operator A^H W A)
// set-up: t [B, M^dim] complex, lag n at index n + N (the bandwidth-2N adjoint of the weights) -> the Hermitian half
// spectrum [B, M^(dim-1) * (M/2+1)] whose kC2R transform is the real kernel grid K; lags with a component -N zeroed,
// M^-dim folded in.  g: the geometry of the bandwidth-N problem (g.M = 2N)
int launch_toeplitz_spectrum(const Geom &g, const float2 *t, int64_t B, float2 *spec, hipStream_t stream);
// grid planes [plane0, plane0 + nplanes) of a chunk (local index 0 .. nplanes) *= K[plane / Cr]; K [B, M^dim] float32,
// 16-byte aligned.  One load of K per point set and cell for all of the set's planes in the chunk; no atomics.
int launch_toeplitz_multiply(const Geom &g, float *grid, const float *K, int64_t Cr, int64_t plane0, int64_t nplanes,
                             hipStream_t stream);

// colfft.hip: the row passes of both FFT stages fused with that product (rowfft_supported grids, planar route): the compact
// half spectrum of the planes 2 * pair, 2 * pair + 1 (pair < npairs) of a chunk is transformed to real rows in LDS,
// multiplied by K[(pair0 + pair) / pairs_per_set] and transformed back, in place -- the grid never reaches memory
int launch_row_toeplitz(const Geom &g, float2 *spec, const float *K, int64_t pairs_per_set, int64_t pair0, int64_t npairs,
                        hipStream_t stream);

// nearfield.hip (the near-field pair sum of the fast summation for singular kernels): arguments as
// nfft_hip_nearfield; `items`: nearfield_item_slots(p) int2 of workspace for the work items
int64_t nearfield_item_slots(const nfft_hip_nearfield_problem *p);
int launch_nearfield(const nfft_hip_nearfield_problem *p, const float *src, const float *xr, const int *sstart,
                     const float *tgt, const int64_t *tindex, const int *tstart, float *z, void *items, hipStream_t stream);
// nearfield_grad.hip (the near field's gradient at the targets and its transpose): arguments as
// nfft_hip_nearfield_gradient -- `spos` / `in` / `sstart` the streamed side, `opos` / `oindex` / `ostart` the output side;
// `items` as above
int launch_nearfield_gradient(const nfft_hip_nearfield_problem *p, int transpose, const double *gradient_poly,
                              const float *spos, const float *in, const int *sstart, const float *opos, const int64_t *oindex,
                              const int *ostart, float *out, void *items, hipStream_t stream);
// nearfield_pgrad.hip (the near field's gradient with respect to the points): arguments as
// nfft_hip_nearfield_point_gradient -- `spos` / `sval` / `sstart` the streamed side, `opos` / `oval` / `oindex` / `ostart`
// the output side; `items` as above
int launch_nearfield_point_gradient(const nfft_hip_nearfield_problem *p, int symmetric, const double *gradient_poly,
                                    const float *spos, const float *sval, const int *sstart, const float *opos,
                                    const float *oval, const int64_t *oindex, const int *ostart, float *out, void *items,
                                    hipStream_t stream);
// ewald_near.hip (the wrapped pair sum erfc(alpha r) / r of the Ewald sum and its field): arguments
// as nfft_hip_ewald_near; `items`: ewald_near_item_slots(p) int2 of workspace for the work items
int64_t ewald_near_item_slots(const nfft_hip_ewald_problem *p);
int launch_ewald_near(const nfft_hip_ewald_problem *p, const float *pos, const float *xr, const int *start,
                      const int64_t *index, float *z, float *f, void *items, hipStream_t stream);
// ewald_near.hip again (the same pair sum in an orthorhombic or triclinic box, on fractional positions, DESIGN.md section
// 7h): arguments as nfft_hip_ewald_near_box; `items`: ewald_near_box_item_slots(p) int2 of workspace
int64_t ewald_near_box_item_slots(const nfft_hip_ewald_box_problem *p);
int launch_ewald_near_box(const nfft_hip_ewald_box_problem *p, const float *pos, const float *xr, const int *start,
                          const int64_t *index, float *z, float *f, void *items, hipStream_t stream);
// ewald_disp.hip (the wrapped pair sum of the dispersion Ewald sum, 1/r^6, and its field): arguments
// and `items` as launch_ewald_near / launch_ewald_near_box (the same item slots)
int launch_ewald_dispersion_near(const nfft_hip_ewald_problem *p, const float *pos, const float *xr, const int *start,
                                 const int64_t *index, float *z, float *f, void *items, hipStream_t stream);
int launch_ewald_dispersion_near_box(const nfft_hip_ewald_box_problem *p, const float *pos, const float *xr, const int *start,
                                     const int64_t *index, float *z, float *f, void *items, hipStream_t stream);
// ewald_dipole.hip (the Ewald sum of charges and point dipoles): the wrapped pair sum of (phi, E) and,
// at order 2, T, arguments as nfft_hip_ewald_dipole_near / _near_box, `items` as launch_ewald_near / launch_ewald_near_box
// (the same item slots); and the spectral step, arguments as nfft_hip_ewald_dipole_spectral
int launch_ewald_dipole_near(const nfft_hip_ewald_problem *p, int order, const float *pos, const float *xs, const int *start,
                             const int64_t *index, float *out, void *items, hipStream_t stream);
int launch_ewald_dipole_near_box(const nfft_hip_ewald_box_problem *p, int order, const float *pos, const float *xs,
                                 const int *start, const int64_t *index, float *out, void *items, hipStream_t stream);
int launch_ewald_dipole_spectral(int64_t N, int64_t batch_size, int64_t num_columns, int order, const void *band,
                                 const float *coeffs, const double *box_inverse, void *out, hipStream_t stream);
// ewald_stokeslet.hip (the periodic Stokeslet sum): the wrapped pair sum of u and, at order 2, of
// G = grad u, arguments as nfft_hip_ewald_stokeslet_near / _near_box, `items` as launch_ewald_near / launch_ewald_near_box
// (the same item slots); and the spectral step, arguments as nfft_hip_ewald_stokeslet_spectral
int launch_ewald_stokeslet_near(const nfft_hip_ewald_problem *p, int order, const float *pos, const float *xs, const int *start,
                                const int64_t *index, float *out, void *items, hipStream_t stream);
int launch_ewald_stokeslet_near_box(const nfft_hip_ewald_box_problem *p, int order, const float *pos, const float *xs,
                                    const int *start, const int64_t *index, float *out, void *items, hipStream_t stream);
int launch_ewald_stokeslet_spectral(int64_t N, int64_t batch_size, int64_t num_columns, int order, const void *band,
                                    const float *coeffs, const double *box_inverse, void *out, hipStream_t stream);
// ewald_rpy.hip (the periodic Rotne-Prager-Yamakawa sum): the wrapped pair sum of u and, at order 2, of
// G = grad u for spheres of one radius, arguments as nfft_hip_ewald_rpy_near / _near_box, `items` as launch_ewald_stokeslet_near
int launch_ewald_rpy_near(const nfft_hip_ewald_problem *p, int order, double radius, const float *pos, const float *xs,
                          const int *start, const int64_t *index, float *out, void *items, hipStream_t stream);
int launch_ewald_rpy_near_box(const nfft_hip_ewald_box_problem *p, int order, double radius, const float *pos, const float *xs,
                              const int *start, const int64_t *index, float *out, void *items, hipStream_t stream);
// ewald_virial.hip (the virial tensor of the Ewald sum): the pair reduction, arguments as
// nfft_hip_ewald_virial_near, `workspace`: ewald_virial_near_workspace(p) bytes, 256-byte aligned (the work items, then one
// partial per item slot); and the spectral reduction, arguments as nfft_hip_ewald_virial_far, `workspace`:
// ewald_virial_far_workspace(...) bytes, 8-byte aligned
int64_t ewald_virial_near_workspace(const nfft_hip_ewald_box_problem *p);
int launch_ewald_virial_near(const nfft_hip_ewald_box_problem *p, const float *pos, const float *xr, const int *start,
                             double *out, void *workspace, hipStream_t stream);
int64_t ewald_virial_far_workspace(int64_t N, int64_t batch_size, int64_t num_columns);
int launch_ewald_virial_far(int64_t N, int64_t batch_size, int64_t num_columns, const void *band, const float *coeffs,
                            const double *box_inverse, double pi2_over_alpha2, double *out, void *workspace,
                            hipStream_t stream);
// ... and what the dispersion sum's virial shares with it: the item slots and the partials of the near workspace, the
// workgroups per point set of the far reduction, and the second level (out [batch_size, 7, C] from `partial`: with `items`
// the item slots of each set's cells, without them rows_per_set rows per set)
int64_t ewald_virial_near_item_slots(const nfft_hip_ewald_box_problem *p);
double *ewald_virial_near_partials(const nfft_hip_ewald_box_problem *p, void *workspace);
int ewald_virial_far_blocks(int64_t N);
int launch_virial_sum(const double *partial, int64_t batch_size, int64_t C, int rows_per_set, const void *items, const int *start,
                      int cells_per_set, double *out, hipStream_t stream);
// (the same level over `partial` [rows, terms, C] for any number of terms: out [batch_size, terms, C])
int launch_virial_sum_terms(const double *partial, int terms, int64_t batch_size, int64_t C, int rows_per_set, const void *items,
                            const int *start, int cells_per_set, double *out, hipStream_t stream);
// The step walks (step_frame.h): one pair walk per pair law, all with one argument list -- that of
// nfft_hip_ewald_lj_table_near, row_start == nullptr for the unmasked walk; the product law reads no types and no table --
// and one workspace: ewald_step8_near_workspace(p) bytes, 256-byte aligned (the work items, then one partial [8] per item
// slot).  ewald_lj_step.hip: the product law a_i a_j / r^12 (sections 7r, 7s); ewald_lj_table.hip: the (C12, dC6) table
// (section 7t); ewald_bmh_table.hip: the (A, B, dC6, C8) table of Buckingham / Born-Mayer-Huggins (section 7u)
typedef int step_near_launch(const nfft_hip_ewald_box_problem *p, double alpha_dispersion, int64_t num_types, int64_t num_entries,
                             const float *pos, const float *xs, const int *types, const float *table, const int *start,
                             const int64_t *index, const int *row_start, const int *col, const float *weight_coulomb,
                             const float *weight_lj, float *f, double *out, void *workspace, hipStream_t stream);
int64_t ewald_step8_near_workspace(const nfft_hip_ewald_box_problem *p);
step_near_launch launch_ewald_lj_step_near, launch_ewald_lj_table_near, launch_ewald_bmh_table_near;
// ewald_lj_step.hip also has the spectral pass of these steps, arguments as nfft_hip_ewald_lj_step_spectral; `workspace`:
// ewald_lj_step_spectral_workspace(N, B) bytes, 8-byte aligned
int64_t ewald_lj_step_spectral_workspace(int64_t N, int64_t batch_size);
int launch_ewald_lj_step_spectral(int64_t N, int64_t batch_size, const void *band, const float *coeffs_coulomb,
                                  const float *coeffs_dispersion, const float *strain_dispersion, const double *box_inverse,
                                  double pi2_over_alpha2, void *spectra, double *out, void *workspace, hipStream_t stream);
// ewald_lj_excl.hip (bonded-pair exclusions of these steps): the list kernel, arguments as
// nfft_hip_ewald_lj_excl_list; `workspace`: ewald_lj_excl_list_workspace(p) bytes, 8-byte aligned
int64_t ewald_lj_excl_list_workspace(const nfft_hip_ewald_box_problem *p);
int launch_ewald_lj_excl_list(const nfft_hip_ewald_box_problem *p, double alpha_dispersion, int64_t num_entries, const float *pos,
                              const float *xs, const int *row_start, const int *col, const float *weight_coulomb,
                              const float *weight_lj, const int *set_start, float *f, double *out, void *workspace,
                              hipStream_t stream);
// ewald_step.hip (potential, field, energy and virial of the Ewald sum in one pair walk and one spectral pass, DESIGN.md
// section 7q): arguments as nfft_hip_ewald_step_near / _spectral, the workspaces those of ewald_virial.hip
// (ewald_virial_near_workspace, ewald_virial_far_workspace), the second level its launch_virial_sum
int launch_ewald_step_near(const nfft_hip_ewald_box_problem *p, const float *pos, const float *xr, const int *start,
                           const int64_t *index, float *z, float *f, double *out, void *workspace, hipStream_t stream);
int launch_ewald_step_spectral(int64_t N, int64_t batch_size, int64_t num_columns, const void *band, const float *coeffs,
                               const double *box_inverse, double pi2_over_alpha2, void *spectra, double *out, void *workspace,
                               hipStream_t stream);
// ewald_disp_virial.hip (the virial tensor of the dispersion Ewald sum): arguments as
// nfft_hip_ewald_dispersion_virial_near / _far, the workspaces those of ewald_virial.hip
int launch_ewald_dispersion_virial_near(const nfft_hip_ewald_box_problem *p, const float *pos, const float *xr, const int *start,
                                        double *out, void *workspace, hipStream_t stream);
int launch_ewald_dispersion_virial_far(int64_t N, int64_t batch_size, int64_t num_columns, const void *band, const float *coeffs,
                                       const float *strain_coeffs, const double *box_inverse, double *out, void *workspace,
                                       hipStream_t stream);
// ewald_yukawa.hip (the Ewald sum of the screened Coulomb potential e^(-lambda r) / r): the wrapped pair
// sum and its field, arguments and `items` as launch_ewald_near / launch_ewald_near_box (the same item slots), and the pair
// part of its virial, arguments and `workspace` as launch_ewald_virial_near; `screening` is lambda
int launch_ewald_yukawa_near(const nfft_hip_ewald_problem *p, double screening, const float *pos, const float *xr, const int *start,
                             const int64_t *index, float *z, float *f, void *items, hipStream_t stream);
int launch_ewald_yukawa_near_box(const nfft_hip_ewald_box_problem *p, double screening, const float *pos, const float *xr,
                                 const int *start, const int64_t *index, float *z, float *f, void *items, hipStream_t stream);
int launch_ewald_yukawa_virial_near(const nfft_hip_ewald_box_problem *p, double screening, const float *pos, const float *xr,
                                    const int *start, double *out, void *workspace, hipStream_t stream);
// ewald_excl.hip (bonded-pair exclusions of the Coulomb and dispersion Ewald sums): the list kernel on
// the unit torus and in a box, arguments as nfft_hip_ewald_excl / _box; and the listed pairs' share of the virial, arguments
// as nfft_hip_ewald_excl_virial, `workspace`: ewald_excl_virial_workspace(p) bytes, 8-byte aligned (one partial per workgroup;
// the second level is launch_virial_sum)
int launch_ewald_excl(const nfft_hip_ewald_excl_problem *p, const float *pos, const float *xr, const int *row_start,
                      const int *col, const float *weight, float *z, float *f, hipStream_t stream);
int launch_ewald_excl_box(const nfft_hip_ewald_excl_problem *p, const float *pos, const float *xr, const int *row_start,
                          const int *col, const float *weight, float *z, float *f, hipStream_t stream);
int64_t ewald_excl_virial_workspace(const nfft_hip_ewald_excl_problem *p);
int launch_ewald_excl_virial(const nfft_hip_ewald_excl_problem *p, const float *pos, const float *xr, const int *row_start,
                             const int *col, const float *weight, const int *set_start, double *out, void *workspace,
                             hipStream_t stream);

// smallgrid.hip: transforms whose oversampled grid (<= 4096 cells) fits one workgroup's LDS -- one kernel per direction,
// no point plan
bool small_grid_supported(const nfft_hip_problem *p);
int launch_small_grid_adjoint(const nfft_hip_problem *p, const float *pos, const int64_t *batch, const void *x, int x_is_complex,
                           int real_output, void *y, const void *mult, int mult_kind, hipStream_t stream);
int launch_small_grid_forward(const nfft_hip_problem *p, const float *pos, const int64_t *batch, const void *xhat, int x_is_complex,
                           int real_output, void *y, hipStream_t stream);

// api.hip: optional per-stage GPU timing with HIP events on the caller's stream (nfft_hip_profile_*)
enum Stage { kStagePlan = 0, kStageGather, kStageZero, kStageSpread, kStageFft, kStageDeconv, kStageInterp, kStageMultiply, kNumStages };
struct StageTimer {
    StageTimer(Stage stage, hipStream_t stream);
    ~StageTimer();
    int slot;
    hipStream_t stream;
};

} // namespace nfft
