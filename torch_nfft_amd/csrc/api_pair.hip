// C-ABI entry points of the pair kernels (include/nfft_hip.h): the near field of the fast summation for singular kernels,
// the near parts of the Ewald sums (1/r, 1/r^6, dipoles and Stokeslets) on the torus and in a box, the virial reductions, the bonded-pair
// exclusions.  They share only the error plumbing and
// the workspace conventions (host_util.h) with the transforms of api.hip.
#include "../../include/nfft_hip.h"

#include <cmath>

#include "common.h"
#include "host_util.h"
#include "kernels.h"

using namespace nfft;

// ---- near field of the fast summation for singular kernels ------------------------------------
namespace {
constexpr int64_t kNearMaxCells = int64_t(1) << 20;

int validate_nearfield(const nfft_hip_nearfield_problem *p)
{
    if (!p) { set_error("Input mismatch: null problem"); return NFFT_HIP_EINVAL; }
    if (p->dim < 1 || p->dim > 3) { set_error("Input mismatch: dim must be 1, 2 or 3"); return NFFT_HIP_EINVAL; }
    if (p->kernel < 0 || p->kernel > NFFT_HIP_KERNEL_LAPLACIAN_RBF) { set_error("Input mismatch: unknown kernel"); return NFFT_HIP_EINVAL; }
    if (p->poly_terms < 1 || p->poly_terms > 8) { set_error("Input mismatch: poly_terms must be in 1..8"); return NFFT_HIP_EINVAL; }
    if (p->num_sources < 0 || p->num_targets < 0 || p->num_columns < 0 || p->batch_size < 1) {
        set_error("Input mismatch: negative size");
        return NFFT_HIP_EINVAL;
    }
    if (p->num_sources >= (int64_t(1) << 31) || p->num_targets >= (int64_t(1) << 31)) {
        set_error("Input mismatch: too many points");
        return NFFT_HIP_EINVAL;
    }
    if (!(p->eps_I > 0.0) || !(p->eps_I < 0.5)) { set_error("Input mismatch: eps_I must lie in (0, 1/2)"); return NFFT_HIP_EINVAL; }
    if (p->cells_per_axis < 1 || 0.5 / p->cells_per_axis < p->eps_I * (1.0 - 1e-12)) {
        set_error("Input mismatch: cells must have an edge 1 / (2 cells_per_axis) >= eps_I");
        return NFFT_HIP_EINVAL;
    }
    int64_t cells = p->batch_size;
    for (int a = 0; a < p->dim && cells <= kNearMaxCells; ++a) cells *= p->cells_per_axis;
    if (cells > kNearMaxCells && p->cells_per_axis > 1) { set_error("Input mismatch: too many cells"); return NFFT_HIP_EINVAL; }
    if (cells >= (int64_t(1) << 30)) { set_error("Input mismatch: too many point sets"); return NFFT_HIP_EINVAL; }
    const bool needs_c = p->kernel >= NFFT_HIP_KERNEL_INVERSE_MULTIQUADRIC;
    if (!(p->c >= 0.0) || (needs_c && !(p->c > 0.0))) { set_error("Input mismatch: the shape parameter c must be positive"); return NFFT_HIP_EINVAL; }
    if (!all_finite(p->poly, p->poly_terms, 3e38)) { set_error("Input mismatch: poly is not finite"); return NFFT_HIP_EINVAL; }
    return 0;
}

int64_t nearfield_need(const nfft_hip_nearfield_problem *p) { return nearfield_item_slots(p) * (int64_t)sizeof(int2) + 256; }

int check_gradient_poly(const nfft_hip_nearfield_problem *p, const double *gradient_poly)
{
    if (!gradient_poly) { set_error("Input mismatch: gradient_poly is null"); return NFFT_HIP_EINVAL; }
    if (!all_finite(gradient_poly, p->poly_terms - 1, 3e38)) {
        set_error("Input mismatch: gradient_poly is not finite");
        return NFFT_HIP_EINVAL;
    }
    return 0;
}

// what the torus problem and the box problem have in common: with_field, the sizes, the point count and alpha
template <class Problem>
int validate_ewald_head(const Problem *p)
{
    if (!p) { set_error("Input mismatch: null problem"); return NFFT_HIP_EINVAL; }
    if (p->with_field != 0 && p->with_field != 1) { set_error("Input mismatch: with_field must be 0 or 1"); return NFFT_HIP_EINVAL; }
    if (p->num_points < 0 || p->num_columns < 0 || p->batch_size < 1) {
        set_error("Input mismatch: negative size");
        return NFFT_HIP_EINVAL;
    }
    if (p->num_points >= (int64_t(1) << 31)) { set_error("Input mismatch: too many points"); return NFFT_HIP_EINVAL; }
    if (!(p->alpha > 0.0) || !(p->alpha < 1e18)) { set_error("Input mismatch: alpha must be positive and finite"); return NFFT_HIP_EINVAL; }
    return 0;
}

} // namespace

extern "C" {

int64_t nfft_hip_nearfield_cells(int32_t dim, double eps_I, int64_t batch_size)
{
    if (dim < 1 || dim > 3 || !(eps_I > 0.0) || !(eps_I < 0.5) || batch_size < 1) {
        set_error("Input mismatch: nearfield cells need dim in 1..3, eps_I in (0, 1/2) and batch_size >= 1");
        return -1;
    }
    int64_t G = (int64_t)std::min(0.5 / eps_I, 1048576.0);
    while (G > 1 && 0.5 / (double)G < eps_I) --G;  // (the quotient may have been rounded up)
    auto cells = [&](int64_t g) { int64_t c = batch_size; for (int a = 0; a < dim; ++a) c *= g; return c; };
    while (G > 1 && cells(G) > kNearMaxCells) G = G > 64 ? G / 2 : G - 1;
    return G < 1 ? 1 : G;
}

int64_t nfft_hip_nearfield_workspace_bytes(const nfft_hip_nearfield_problem *p)
{
    if (validate_nearfield(p)) return -1;
    return nearfield_need(p);
}

int nfft_hip_nearfield(const nfft_hip_nearfield_problem *p, const float *sources, const float *xr,
                       const int32_t *source_start, const float *targets, const int64_t *target_index,
                       const int32_t *target_start, float *z, void *workspace, int64_t workspace_bytes, void *stream)
{
    if (int rc = take_pending_fault()) return rc;  // a kernel of an earlier call gave up: say so
    if (int rc = validate_nearfield(p)) return rc;
    if (p->num_targets == 0 || p->num_columns == 0) return 0;
    if (!z) { set_error("Input mismatch: z is null"); return NFFT_HIP_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    if (p->num_sources == 0) {
        NFFT_HIP_CHECK(hipMemsetAsync(z, 0, (size_t)(p->num_targets * p->num_columns) * sizeof(float), s));
        return 0;
    }
    if (!sources || !xr || !source_start || !targets || !target_index || !target_start) {
        set_error("Input mismatch: null input");
        return NFFT_HIP_EINVAL;
    }
    char *ws = workspace_base(workspace, workspace_bytes, nearfield_need(p));
    if (!ws) return NFFT_HIP_EWORKSPACE;
    return launch_nearfield(p, sources, xr, source_start, targets, target_index, target_start, z, ws, s);
}

// ---- its gradient at the targets and the transpose ---------------------------------------------
static int validate_nearfield_gradient(const nfft_hip_nearfield_problem *p)
{
    if (int rc = validate_nearfield(p)) return rc;
    if (p->poly_terms < 2) {
        set_error("Input mismatch: the near field's gradient needs poly_terms >= 2 (K_R must be differentiable at eps_I)");
        return NFFT_HIP_EINVAL;
    }
    return 0;
}

int64_t nfft_hip_nearfield_gradient_workspace_bytes(const nfft_hip_nearfield_problem *p)
{
    if (validate_nearfield_gradient(p)) return -1;
    return nearfield_need(p);
}

int nfft_hip_nearfield_gradient(const nfft_hip_nearfield_problem *p, int32_t transpose, const double *gradient_poly,
                                const float *sources, const float *xr, const int32_t *source_start, const float *targets,
                                const int64_t *target_index, const int32_t *target_start, float *out, void *workspace,
                                int64_t workspace_bytes, void *stream)
{
    if (int rc = take_pending_fault()) return rc;  // a kernel of an earlier call gave up: say so
    if (int rc = validate_nearfield_gradient(p)) return rc;
    if (transpose != 0 && transpose != 1) { set_error("Input mismatch: transpose must be 0 or 1"); return NFFT_HIP_EINVAL; }
    if (int rc = check_gradient_poly(p, gradient_poly)) return rc;
    if (p->num_targets == 0 || p->num_columns == 0) return 0;
    if (!out) { set_error("Input mismatch: out is null"); return NFFT_HIP_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    if (p->num_sources == 0) {
        const int64_t row = transpose ? p->num_columns : p->dim * p->num_columns;
        NFFT_HIP_CHECK(hipMemsetAsync(out, 0, (size_t)(p->num_targets * row) * sizeof(float), s));
        return 0;
    }
    if (!sources || !xr || !source_start || !targets || !target_index || !target_start) {
        set_error("Input mismatch: null input");
        return NFFT_HIP_EINVAL;
    }
    char *ws = workspace_base(workspace, workspace_bytes, nearfield_need(p));
    if (!ws) return NFFT_HIP_EWORKSPACE;
    return launch_nearfield_gradient(p, transpose, gradient_poly, sources, xr, source_start, targets, target_index,
                                     target_start, out, ws, s);
}

// ---- its gradient with respect to the points ----------------------------------------------------
int64_t nfft_hip_nearfield_point_gradient_workspace_bytes(const nfft_hip_nearfield_problem *p)
{
    if (validate_nearfield_gradient(p)) return -1;
    return nearfield_need(p);
}

int nfft_hip_nearfield_point_gradient(const nfft_hip_nearfield_problem *p, int32_t symmetric, const double *gradient_poly,
                                      const float *streamed, const float *streamed_values, const int32_t *streamed_start,
                                      const float *output, const float *output_values, const int64_t *output_index,
                                      const int32_t *output_start, float *out, void *workspace, int64_t workspace_bytes,
                                      void *stream)
{
    if (int rc = take_pending_fault()) return rc;  // a kernel of an earlier call gave up: say so
    if (int rc = validate_nearfield_gradient(p)) return rc;
    if (symmetric != 0 && symmetric != 1) { set_error("Input mismatch: symmetric must be 0 or 1"); return NFFT_HIP_EINVAL; }
    if (symmetric && p->num_sources != p->num_targets) {
        set_error("Input mismatch: a symmetric sweep needs one point set on both sides");
        return NFFT_HIP_EINVAL;
    }
    if (int rc = check_gradient_poly(p, gradient_poly)) return rc;
    if (p->num_targets == 0 || p->num_columns == 0) return 0;
    if (!out) { set_error("Input mismatch: out is null"); return NFFT_HIP_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    if (p->num_sources == 0) {
        NFFT_HIP_CHECK(hipMemsetAsync(out, 0, (size_t)(p->num_targets * p->dim) * sizeof(float), s));
        return 0;
    }
    if (!streamed || !streamed_values || !streamed_start || !output || !output_values || !output_index || !output_start) {
        set_error("Input mismatch: null input");
        return NFFT_HIP_EINVAL;
    }
    char *ws = workspace_base(workspace, workspace_bytes, nearfield_need(p));
    if (!ws) return NFFT_HIP_EWORKSPACE;
    return launch_nearfield_point_gradient(p, symmetric, gradient_poly, streamed, streamed_values, streamed_start, output,
                                           output_values, output_index, output_start, out, ws, s);
}

// ---- near part of the Ewald sum for the periodic 1/r ------------------------------------------
static int validate_ewald(const nfft_hip_ewald_problem *p)
{
    if (int rc = validate_ewald_head(p)) return rc;
    if (!(p->r_cut > 0.0) || !(p->r_cut <= 1.0 / 3.0)) { set_error("Input mismatch: r_cut must lie in (0, 1/3]"); return NFFT_HIP_EINVAL; }
    if (p->cells_per_axis < 3 || 1.0 / p->cells_per_axis < p->r_cut * (1.0 - 1e-12)) {
        set_error("Input mismatch: cells must be at least 3 per axis with an edge 1 / cells_per_axis >= r_cut");
        return NFFT_HIP_EINVAL;
    }
    if (p->batch_size > kNearMaxCells ||
        p->batch_size * p->cells_per_axis * p->cells_per_axis * p->cells_per_axis > kNearMaxCells) {
        set_error("Input mismatch: too many cells");
        return NFFT_HIP_EINVAL;
    }
    return 0;
}

static int64_t ewald_near_need(const nfft_hip_ewald_problem *p) { return ewald_near_item_slots(p) * (int64_t)sizeof(int2) + 256; }

int64_t nfft_hip_ewald_near_cells(double r_cut, int64_t batch_size)
{
    if (!(r_cut > 0.0) || !(r_cut <= 1.0 / 3.0) || batch_size < 1) {
        set_error("Input mismatch: ewald cells need r_cut in (0, 1/3] and batch_size >= 1");
        return -1;
    }
    int64_t G = (int64_t)std::min(1.0 / r_cut, 1024.0);
    while (G > 3 && 1.0 / (double)G < r_cut) --G;  // (the quotient may have been rounded up)
    if (G < 3) G = 3;                              // (... or down, at r_cut = 1/3)
    while (G > 3 && batch_size * G * G * G > kNearMaxCells) --G;
    if (batch_size > kNearMaxCells || batch_size * G * G * G > kNearMaxCells) {
        set_error("Input mismatch: too many point sets for a grid of 3 cells per axis");
        return -1;
    }
    return G;
}

int64_t nfft_hip_ewald_near_workspace_bytes(const nfft_hip_ewald_problem *p)
{
    if (validate_ewald(p)) return -1;
    return ewald_near_need(p);
}

// the checks of a wrapped pair sweep on the torus, in their order; *ws: the aligned workspace, or null where there is nothing to launch
static int ewald_near_checks(const nfft_hip_ewald_problem *p, const float *points, const float *xr, const int32_t *start,
                             const int64_t *index, float *z, float *field, void *workspace, int64_t workspace_bytes, char **ws)
{
    *ws = nullptr;
    if (int rc = take_pending_fault()) return rc;  // a kernel of an earlier call gave up: say so
    if (int rc = validate_ewald(p)) return rc;
    if (p->num_points == 0 || p->num_columns == 0) return 0;
    if (!z) { set_error("Input mismatch: z is null"); return NFFT_HIP_EINVAL; }
    if (p->with_field && !field) { set_error("Input mismatch: field is null"); return NFFT_HIP_EINVAL; }
    if (!points || !xr || !start || !index) { set_error("Input mismatch: null input"); return NFFT_HIP_EINVAL; }
    *ws = workspace_base(workspace, workspace_bytes, ewald_near_need(p));
    return *ws ? 0 : NFFT_HIP_EWORKSPACE;
}

// the checks of a wrapped pair sweep on the torus, then `launch` (the Coulomb sweep, the dispersion sweep of section 7j or
// the dipole sweep of section 7l or the Stokeslet sweep of section 7m)
typedef int (*ewald_launch)(const nfft_hip_ewald_problem *, const float *, const float *, const int *, const int64_t *, float *,
                            float *, void *, hipStream_t);
static int ewald_near_call(ewald_launch launch, const nfft_hip_ewald_problem *p, const float *points, const float *xr,
                           const int32_t *start, const int64_t *index, float *z, float *field, void *workspace,
                           int64_t workspace_bytes, void *stream)
{
    char *ws;
    if (int rc = ewald_near_checks(p, points, xr, start, index, z, field, workspace, workspace_bytes, &ws)) return rc;
    if (!ws) return 0;
    return launch(p, points, xr, start, index, z, field, ws, (hipStream_t)stream);
}

int nfft_hip_ewald_near(const nfft_hip_ewald_problem *p, const float *points, const float *xr, const int32_t *start,
                        const int64_t *index, float *z, float *field, void *workspace, int64_t workspace_bytes,
                        void *stream)
{
    return ewald_near_call(launch_ewald_near, p, points, xr, start, index, z, field, workspace, workspace_bytes, stream);
}

// ---- near part of the dispersion Ewald sum, 1/r^6: the same problem, checks and workspace -------
int nfft_hip_ewald_dispersion_near(const nfft_hip_ewald_problem *p, const float *points, const float *xr,
                                   const int32_t *start, const int64_t *index, float *z, float *field, void *workspace,
                                   int64_t workspace_bytes, void *stream)
{
    return ewald_near_call(launch_ewald_dispersion_near, p, points, xr, start, index, z, field, workspace, workspace_bytes,
                           stream);
}

// ---- the same pair sum in an orthorhombic or triclinic box ------------------------------------
// perpendicular widths w_a = 1 / |column a of A^-1| of the box A00, A10, A11, A20, A21, A22; false unless every entry is
// finite and the diagonal positive
static bool ewald_box_widths(const double *box, double *w)
{
    if (!all_finite(box, 6, 1e300)) return false;
    const double a00 = box[0], a10 = box[1], a11 = box[2], a20 = box[3], a21 = box[4], a22 = box[5];
    if (!(a00 > 0.0) || !(a11 > 0.0) || !(a22 > 0.0)) return false;
    // A^-1 is lower triangular too
    const double i00 = 1.0 / a00, i11 = 1.0 / a11, i22 = 1.0 / a22;
    const double i10 = -a10 * i00 * i11, i21 = -a21 * i11 * i22;
    const double i20 = (a10 * a21 - a11 * a20) * i00 * i11 * i22;
    w[0] = 1.0 / std::sqrt(i00 * i00 + i10 * i10 + i20 * i20);
    w[1] = 1.0 / std::sqrt(i11 * i11 + i21 * i21);
    w[2] = a22;
    for (int a = 0; a < 3; ++a)
        if (!(w[a] > 0.0) || !(w[a] < 1e300)) return false;
    return true;
}

// r_cut in (0, min_a w_a / 3] (the quotient's last bit is not held against the caller)
static bool ewald_box_r_cut_ok(const double *w, double r_cut)
{
    const double wmin = std::min(w[0], std::min(w[1], w[2]));
    return r_cut > 0.0 && r_cut * (1.0 - 1e-12) <= wmin / 3.0;
}

static int validate_ewald_box(const nfft_hip_ewald_box_problem *p)
{
    if (int rc = validate_ewald_head(p)) return rc;
    double w[3];
    if (!ewald_box_widths(p->box, w)) {
        set_error("Input mismatch: the box must be finite with a positive diagonal");
        return NFFT_HIP_EINVAL;
    }
    if (!ewald_box_r_cut_ok(w, p->r_cut)) {
        set_error("Input mismatch: r_cut must lie in (0, min w_a / 3] for the box's perpendicular widths w_a");
        return NFFT_HIP_EINVAL;
    }
    int64_t cells = p->batch_size;
    for (int a = 0; a < 3; ++a) {
        if (p->cells[a] < 3 || p->cells[a] > 1024 || w[a] / p->cells[a] < p->r_cut * (1.0 - 1e-12)) {
            set_error("Input mismatch: cells must be at least 3 per axis with a width w_a / cells[a] >= r_cut");
            return NFFT_HIP_EINVAL;
        }
        cells = cells > kNearMaxCells ? cells : cells * p->cells[a];
    }
    if (cells > kNearMaxCells) { set_error("Input mismatch: too many cells"); return NFFT_HIP_EINVAL; }
    return 0;
}

static int64_t ewald_box_need(const nfft_hip_ewald_box_problem *p) { return ewald_near_box_item_slots(p) * (int64_t)sizeof(int2) + 256; }

int64_t nfft_hip_ewald_box_cells(const double *box, double r_cut, int64_t batch_size, int32_t *cells_out)
{
    double w[3];
    if (!box || !cells_out) { set_error("Input mismatch: null input"); return -1; }
    if (!ewald_box_widths(box, w)) {
        set_error("Input mismatch: the box must be finite with a positive diagonal");
        return -1;
    }
    if (!ewald_box_r_cut_ok(w, r_cut) || batch_size < 1) {
        set_error("Input mismatch: ewald cells need r_cut in (0, min w_a / 3] and batch_size >= 1");
        return -1;
    }
    int64_t G[3];
    for (int a = 0; a < 3; ++a) {
        G[a] = (int64_t)std::min(w[a] / r_cut, 1024.0);
        while (G[a] > 3 && w[a] / (double)G[a] < r_cut) --G[a];  // (the quotient may have been rounded up)
        if (G[a] < 3) G[a] = 3;                                  // (... or down, at r_cut = w_a / 3)
    }
    while (batch_size <= kNearMaxCells && batch_size * G[0] * G[1] * G[2] > kNearMaxCells) {
        int a = 0;  // the largest count first
        if (G[1] > G[a]) a = 1;
        if (G[2] > G[a]) a = 2;
        if (G[a] <= 3) break;
        --G[a];
    }
    if (batch_size > kNearMaxCells || batch_size * G[0] * G[1] * G[2] > kNearMaxCells) {
        set_error("Input mismatch: too many point sets for a grid of 3 cells per axis");
        return -1;
    }
    for (int a = 0; a < 3; ++a) cells_out[a] = (int32_t)G[a];
    return 0;
}

int64_t nfft_hip_ewald_near_box_workspace_bytes(const nfft_hip_ewald_box_problem *p)
{
    if (validate_ewald_box(p)) return -1;
    return ewald_box_need(p);
}

// (as ewald_near_checks)
static int ewald_near_box_checks(const nfft_hip_ewald_box_problem *p, const float *points, const float *xr, const int32_t *start,
                                 const int64_t *index, float *z, float *field, void *workspace, int64_t workspace_bytes,
                                 char **ws)
{
    *ws = nullptr;
    if (int rc = take_pending_fault()) return rc;  // a kernel of an earlier call gave up: say so
    if (int rc = validate_ewald_box(p)) return rc;
    if (p->num_points == 0 || p->num_columns == 0) return 0;
    if (!z) { set_error("Input mismatch: z is null"); return NFFT_HIP_EINVAL; }
    if (p->with_field && !field) { set_error("Input mismatch: field is null"); return NFFT_HIP_EINVAL; }
    if (!points || !xr || !start || !index) { set_error("Input mismatch: null input"); return NFFT_HIP_EINVAL; }
    *ws = workspace_base(workspace, workspace_bytes, ewald_box_need(p));
    return *ws ? 0 : NFFT_HIP_EWORKSPACE;
}

typedef int (*ewald_box_launch)(const nfft_hip_ewald_box_problem *, const float *, const float *, const int *, const int64_t *,
                                float *, float *, void *, hipStream_t);
static int ewald_near_box_call(ewald_box_launch launch, const nfft_hip_ewald_box_problem *p, const float *points,
                               const float *xr, const int32_t *start, const int64_t *index, float *z, float *field,
                               void *workspace, int64_t workspace_bytes, void *stream)
{
    char *ws;
    if (int rc = ewald_near_box_checks(p, points, xr, start, index, z, field, workspace, workspace_bytes, &ws)) return rc;
    if (!ws) return 0;
    return launch(p, points, xr, start, index, z, field, ws, (hipStream_t)stream);
}

int nfft_hip_ewald_near_box(const nfft_hip_ewald_box_problem *p, const float *points, const float *xr,
                            const int32_t *start, const int64_t *index, float *z, float *field, void *workspace,
                            int64_t workspace_bytes, void *stream)
{
    return ewald_near_box_call(launch_ewald_near_box, p, points, xr, start, index, z, field, workspace, workspace_bytes, stream);
}

int nfft_hip_ewald_dispersion_near_box(const nfft_hip_ewald_box_problem *p, const float *points, const float *xr,
                                       const int32_t *start, const int64_t *index, float *z, float *field, void *workspace,
                                       int64_t workspace_bytes, void *stream)
{
    return ewald_near_box_call(launch_ewald_dispersion_near_box, p, points, xr, start, index, z, field, workspace,
                               workspace_bytes, stream);
}

// ---- Ewald sum of charges and point dipoles: the same problems, checks and workspaces ------------
static int check_dipole_order(int32_t order)
{
    if (order != 1 && order != 2) { set_error("Input mismatch: order must be 1 or 2"); return NFFT_HIP_EINVAL; }
    return 0;
}

// the dipole sweeps of order 1 and 2 as the shared calls launch them (one output: the field pointer is not used)
static int dipole_near_1(const nfft_hip_ewald_problem *p, const float *pos, const float *xs, const int *start, const int64_t *index,
                         float *out, float *, void *items, hipStream_t s)
{
    return launch_ewald_dipole_near(p, 1, pos, xs, start, index, out, items, s);
}

static int dipole_near_2(const nfft_hip_ewald_problem *p, const float *pos, const float *xs, const int *start, const int64_t *index,
                         float *out, float *, void *items, hipStream_t s)
{
    return launch_ewald_dipole_near(p, 2, pos, xs, start, index, out, items, s);
}

static int dipole_near_box_1(const nfft_hip_ewald_box_problem *p, const float *pos, const float *xs, const int *start,
                             const int64_t *index, float *out, float *, void *items, hipStream_t s)
{
    return launch_ewald_dipole_near_box(p, 1, pos, xs, start, index, out, items, s);
}

static int dipole_near_box_2(const nfft_hip_ewald_box_problem *p, const float *pos, const float *xs, const int *start,
                             const int64_t *index, float *out, float *, void *items, hipStream_t s)
{
    return launch_ewald_dipole_near_box(p, 2, pos, xs, start, index, out, items, s);
}

// (out stands for z and for field in the shared checks)
int nfft_hip_ewald_dipole_near(const nfft_hip_ewald_problem *p, const float *points, const float *xs, const int32_t *start,
                               const int64_t *index, int32_t order, float *out, void *workspace, int64_t workspace_bytes,
                               void *stream)
{
    if (int rc = check_dipole_order(order)) return rc;
    return ewald_near_call(order == 2 ? dipole_near_2 : dipole_near_1, p, points, xs, start, index, out, out, workspace,
                           workspace_bytes, stream);
}

int nfft_hip_ewald_dipole_near_box(const nfft_hip_ewald_box_problem *p, const float *points, const float *xs,
                                   const int32_t *start, const int64_t *index, int32_t order, float *out, void *workspace,
                                   int64_t workspace_bytes, void *stream)
{
    if (int rc = check_dipole_order(order)) return rc;
    return ewald_near_box_call(order == 2 ? dipole_near_box_2 : dipole_near_box_1, p, points, xs, start, index, out, out,
                               workspace, workspace_bytes, stream);
}

// ---- periodic Stokeslet sum: the same problems, checks and workspaces ---------------------------
// the Stokeslet sweeps of order 1 and 2 as the shared calls launch them (one output: the field pointer is not used)
static int stokeslet_near_1(const nfft_hip_ewald_problem *p, const float *pos, const float *xs, const int *start,
                            const int64_t *index, float *out, float *, void *items, hipStream_t s)
{
    return launch_ewald_stokeslet_near(p, 1, pos, xs, start, index, out, items, s);
}

static int stokeslet_near_2(const nfft_hip_ewald_problem *p, const float *pos, const float *xs, const int *start,
                            const int64_t *index, float *out, float *, void *items, hipStream_t s)
{
    return launch_ewald_stokeslet_near(p, 2, pos, xs, start, index, out, items, s);
}

static int stokeslet_near_box_1(const nfft_hip_ewald_box_problem *p, const float *pos, const float *xs, const int *start,
                                const int64_t *index, float *out, float *, void *items, hipStream_t s)
{
    return launch_ewald_stokeslet_near_box(p, 1, pos, xs, start, index, out, items, s);
}

static int stokeslet_near_box_2(const nfft_hip_ewald_box_problem *p, const float *pos, const float *xs, const int *start,
                                const int64_t *index, float *out, float *, void *items, hipStream_t s)
{
    return launch_ewald_stokeslet_near_box(p, 2, pos, xs, start, index, out, items, s);
}

// (out stands for z and for field in the shared checks; the order is checked as for the dipole sweep)
int nfft_hip_ewald_stokeslet_near(const nfft_hip_ewald_problem *p, const float *points, const float *xs, const int32_t *start,
                                  const int64_t *index, int32_t order, float *out, void *workspace, int64_t workspace_bytes,
                                  void *stream)
{
    if (int rc = check_dipole_order(order)) return rc;
    return ewald_near_call(order == 2 ? stokeslet_near_2 : stokeslet_near_1, p, points, xs, start, index, out, out, workspace,
                           workspace_bytes, stream);
}

int nfft_hip_ewald_stokeslet_near_box(const nfft_hip_ewald_box_problem *p, const float *points, const float *xs,
                                      const int32_t *start, const int64_t *index, int32_t order, float *out, void *workspace,
                                      int64_t workspace_bytes, void *stream)
{
    if (int rc = check_dipole_order(order)) return rc;
    return ewald_near_box_call(order == 2 ? stokeslet_near_box_2 : stokeslet_near_box_1, p, points, xs, start, index, out, out,
                               workspace, workspace_bytes, stream);
}

// ---- periodic Rotne-Prager-Yamakawa sum: the same problems, checks and workspaces ---------------
// the sphere radius: finite, positive, and two spheres in contact inside the pair sum's reach (the overlap branch r < 2 a
// belongs to the pair sum alone)
static int check_rpy_radius(double radius, const double *r_cut)
{
    if (!(radius > 0.0) || !(radius < 1e300)) { set_error("Input mismatch: radius must be positive and finite"); return NFFT_HIP_EINVAL; }
    if (r_cut && 2.0 * radius > *r_cut) { set_error("Input mismatch: 2 radius <= r_cut is required"); return NFFT_HIP_EINVAL; }
    return 0;
}

// (out stands for z and for field in the shared checks; the order is checked as for the dipole sweep)
int nfft_hip_ewald_rpy_near(const nfft_hip_ewald_problem *p, const float *points, const float *xs, const int32_t *start,
                            const int64_t *index, int32_t order, double radius, float *out, void *workspace,
                            int64_t workspace_bytes, void *stream)
{
    if (int rc = check_dipole_order(order)) return rc;
    if (int rc = check_rpy_radius(radius, p ? &p->r_cut : nullptr)) return rc;
    char *ws;
    if (int rc = ewald_near_checks(p, points, xs, start, index, out, out, workspace, workspace_bytes, &ws)) return rc;
    if (!ws) return 0;
    return launch_ewald_rpy_near(p, order, radius, points, xs, start, index, out, ws, (hipStream_t)stream);
}

int nfft_hip_ewald_rpy_near_box(const nfft_hip_ewald_box_problem *p, const float *points, const float *xs, const int32_t *start,
                                const int64_t *index, int32_t order, double radius, float *out, void *workspace,
                                int64_t workspace_bytes, void *stream)
{
    if (int rc = check_dipole_order(order)) return rc;
    if (int rc = check_rpy_radius(radius, p ? &p->r_cut : nullptr)) return rc;
    char *ws;
    if (int rc = ewald_near_box_checks(p, points, xs, start, index, out, out, workspace, workspace_bytes, &ws)) return rc;
    if (!ws) return 0;
    return launch_ewald_rpy_near_box(p, order, radius, points, xs, start, index, out, ws, (hipStream_t)stream);
}

// ---- virial tensor of the Ewald sum -----------------------------------------------------------
static int validate_virial_far(int64_t N, int64_t batch_size, int64_t num_columns)
{
    if (N < 2 || N > 2048 || N % 2) { set_error("Input mismatch: N must be even with 2 <= N <= 2048"); return NFFT_HIP_EINVAL; }
    // (the launches: 1024 workgroups per point set at most, one workgroup per point set and column)
    if (batch_size < 1 || batch_size >= (int64_t(1) << 14) || num_columns < 0 || num_columns >= (int64_t(1) << 21) ||
        batch_size * num_columns >= (int64_t(1) << 21)) {
        set_error("Input mismatch: 1 <= batch_size < 2^14, num_columns >= 0 and batch_size * num_columns < 2^21 are required");
        return NFFT_HIP_EINVAL;
    }
    return 0;
}

// the lower triangle of A^-1 as the far reductions take it
static int validate_box_inverse(const double *box_inverse)
{
    if (!box_inverse) { set_error("Input mismatch: box_inverse is null"); return NFFT_HIP_EINVAL; }
    if (!all_finite(box_inverse, 6, 1e300)) {
        set_error("Input mismatch: the entries of box_inverse must be finite");
        return NFFT_HIP_EINVAL;
    }
    if (!(box_inverse[0] > 0.0) || !(box_inverse[2] > 0.0) || !(box_inverse[5] > 0.0)) {
        set_error("Input mismatch: the diagonal of box_inverse must be positive");
        return NFFT_HIP_EINVAL;
    }
    return 0;
}

// the box problem's own checks, and the second level's launch: one workgroup per point set and column
static int validate_virial_near(const nfft_hip_ewald_box_problem *p)
{
    if (int rc = validate_ewald_box(p)) return rc;
    if (p->num_columns >= (int64_t(1) << 21) || p->batch_size * p->num_columns >= (int64_t(1) << 31)) {
        set_error("Input mismatch: num_columns < 2^21 and batch_size * num_columns < 2^31 are required");
        return NFFT_HIP_EINVAL;
    }
    return 0;
}

static int64_t virial_near_need(const nfft_hip_ewald_box_problem *p) { return ewald_virial_near_workspace(p) + 256; }
static int64_t virial_far_need(int64_t N, int64_t B, int64_t C) { return ewald_virial_far_workspace(N, B, C) + 256; }

int64_t nfft_hip_ewald_virial_near_workspace_bytes(const nfft_hip_ewald_box_problem *p)
{
    if (validate_virial_near(p)) return -1;
    return virial_near_need(p);
}

// (`launch`: the pair reduction of the Coulomb sum, or that of the dispersion sum on the same problem, section 7k)
typedef int (*virial_near_launch)(const nfft_hip_ewald_box_problem *, const float *, const float *, const int *, double *, void *,
                                  hipStream_t);
// the checks of a pair reduction, in their order; *ws: the aligned workspace, or null where there is nothing to launch
static int virial_near_checks(const nfft_hip_ewald_box_problem *p, const float *points, const float *xr, const int32_t *start,
                              double *out, void *workspace, int64_t workspace_bytes, void *stream, char **ws)
{
    *ws = nullptr;
    if (int rc = take_pending_fault()) return rc;  // a kernel of an earlier call gave up: say so
    if (int rc = validate_virial_near(p)) return rc;
    if (p->num_columns == 0) return 0;
    if (!out) { set_error("Input mismatch: out is null"); return NFFT_HIP_EINVAL; }
    if (p->num_points == 0) {
        NFFT_HIP_CHECK(hipMemsetAsync(out, 0, (size_t)(p->batch_size * 7 * p->num_columns) * sizeof(double), (hipStream_t)stream));
        return 0;
    }
    if (!points || !xr || !start) { set_error("Input mismatch: null input"); return NFFT_HIP_EINVAL; }
    *ws = workspace_base(workspace, workspace_bytes, virial_near_need(p));
    return *ws ? 0 : NFFT_HIP_EWORKSPACE;
}

static int virial_near_call(virial_near_launch launch, const nfft_hip_ewald_box_problem *p, const float *points, const float *xr,
                            const int32_t *start, double *out, void *workspace, int64_t workspace_bytes, void *stream)
{
    char *ws;
    if (int rc = virial_near_checks(p, points, xr, start, out, workspace, workspace_bytes, stream, &ws)) return rc;
    if (!ws) return 0;
    return launch(p, points, xr, start, out, ws, (hipStream_t)stream);
}

int nfft_hip_ewald_virial_near(const nfft_hip_ewald_box_problem *p, const float *points, const float *xr,
                               const int32_t *start, double *out, void *workspace, int64_t workspace_bytes, void *stream)
{
    return virial_near_call(launch_ewald_virial_near, p, points, xr, start, out, workspace, workspace_bytes, stream);
}

// pi^2 / alpha^2 of the Coulomb sum's spectral reductions
static int check_pi2_over_alpha2(double pi2_over_alpha2)
{
    if (!(pi2_over_alpha2 > 0.0) || !(pi2_over_alpha2 < 1e300)) {
        set_error("Input mismatch: pi2_over_alpha2 must be positive and finite");
        return NFFT_HIP_EINVAL;
    }
    return 0;
}

// the kernels with one thread per (frequency, column) count them in 32 bits
static int check_spectral_elements(int64_t N, int64_t num_columns)
{
    if (N * N * N * num_columns >= (int64_t(1) << 31)) {
        set_error("Input mismatch: N^3 num_columns < 2^31 is required");
        return NFFT_HIP_EINVAL;
    }
    return 0;
}

int64_t nfft_hip_ewald_virial_far_workspace_bytes(int64_t N, int64_t batch_size, int64_t num_columns)
{
    if (validate_virial_far(N, batch_size, num_columns)) return -1;
    return virial_far_need(N, batch_size, num_columns);
}

int nfft_hip_ewald_virial_far(int64_t N, int64_t batch_size, int64_t num_columns, const void *band, const float *coeffs,
                              const double *box_inverse, double pi2_over_alpha2, double *out, void *workspace,
                              int64_t workspace_bytes, void *stream)
{
    if (int rc = take_pending_fault()) return rc;  // a kernel of an earlier call gave up: say so
    if (int rc = validate_virial_far(N, batch_size, num_columns)) return rc;
    if (int rc = validate_box_inverse(box_inverse)) return rc;
    if (int rc = check_pi2_over_alpha2(pi2_over_alpha2)) return rc;
    if (num_columns == 0) return 0;
    if (!band || !coeffs || !out) { set_error("Input mismatch: null input"); return NFFT_HIP_EINVAL; }
    char *ws = workspace_base(workspace, workspace_bytes, virial_far_need(N, batch_size, num_columns));
    if (!ws) return NFFT_HIP_EWORKSPACE;
    return launch_ewald_virial_far(N, batch_size, num_columns, band, coeffs, box_inverse, pi2_over_alpha2, out, ws,
                                   (hipStream_t)stream);
}

// ---- potential, field, energy and virial in one pass: the checks and workspaces of section 7i ----
int64_t nfft_hip_ewald_step_near_workspace_bytes(const nfft_hip_ewald_box_problem *p)
{
    return nfft_hip_ewald_virial_near_workspace_bytes(p);
}

int nfft_hip_ewald_step_near(const nfft_hip_ewald_box_problem *p, const float *points, const float *xr, const int32_t *start,
                             const int64_t *index, float *z, float *f, double *out7, void *workspace, int64_t workspace_bytes,
                             void *stream)
{
    char *ws;
    if (int rc = virial_near_checks(p, points, xr, start, out7, workspace, workspace_bytes, stream, &ws)) return rc;
    if (!ws) return 0;  // (no columns, or no points: out7 has been zeroed and there is no row of z or f)
    if (!index || !z || !f) { set_error("Input mismatch: null input"); return NFFT_HIP_EINVAL; }
    return launch_ewald_step_near(p, points, xr, start, index, z, f, out7, ws, (hipStream_t)stream);
}

int64_t nfft_hip_ewald_step_spectral_workspace_bytes(int64_t N, int64_t batch_size, int64_t num_columns)
{
    return nfft_hip_ewald_virial_far_workspace_bytes(N, batch_size, num_columns);
}

int nfft_hip_ewald_step_spectral(int64_t N, int64_t batch_size, int64_t num_columns, const void *band, const float *coeffs,
                                 const double *box_inverse, double pi2_over_alpha2, void *spectra, double *out7, void *workspace,
                                 int64_t workspace_bytes, void *stream)
{
    if (int rc = take_pending_fault()) return rc;  // a kernel of an earlier call gave up: say so
    if (int rc = validate_virial_far(N, batch_size, num_columns)) return rc;
    if (int rc = validate_box_inverse(box_inverse)) return rc;
    if (int rc = check_pi2_over_alpha2(pi2_over_alpha2)) return rc;
    if (num_columns == 0) return 0;
    if (!band || !coeffs || !spectra || !out7) { set_error("Input mismatch: null input"); return NFFT_HIP_EINVAL; }
    char *ws = workspace_base(workspace, workspace_bytes, virial_far_need(N, batch_size, num_columns));
    if (!ws) return NFFT_HIP_EWORKSPACE;
    return launch_ewald_step_spectral(N, batch_size, num_columns, band, coeffs, box_inverse, pi2_over_alpha2, spectra, out7, ws,
                                      (hipStream_t)stream);
}

// ---- Lennard-Jones + Coulomb step: the box problem's checks, eight sums per point set ----------
// the problem of the pair walk: the box problem with one column (the three values of a point are not columns) and the
// second splitting parameter
static int validate_lj_step_near(const nfft_hip_ewald_box_problem *p, double alpha_dispersion)
{
    if (int rc = validate_ewald_box(p)) return rc;
    if (p->num_columns != 1) { set_error("Input mismatch: num_columns must be 1"); return NFFT_HIP_EINVAL; }
    if (!(alpha_dispersion > 0.0) || !(alpha_dispersion < 1e18)) {
        set_error("Input mismatch: alpha_dispersion must be positive and finite");
        return NFFT_HIP_EINVAL;
    }
    return 0;
}

static int validate_lj_step_spectral(int64_t N, int64_t batch_size) { return validate_virial_far(N, batch_size, 1); }

// the four walks of these steps (step_frame.h) have one workspace ...
int64_t nfft_hip_ewald_lj_step_near_workspace_bytes(const nfft_hip_ewald_box_problem *p, double alpha_dispersion)
{
    if (validate_lj_step_near(p, alpha_dispersion)) return -1;
    return ewald_step8_near_workspace(p) + 256;
}

// ... and, after the pending fault and their own checks (`rc`: the first of them that failed), one call: out8, the empty
// problem, the null checks (a walk with a table reads types), the workspace and the launch
static int step_near_call(step_near_launch *launch, int rc, const nfft_hip_ewald_box_problem *p, double alpha_dispersion,
                          int64_t num_types, int64_t num_entries, const float *points, const float *xs, const int32_t *types,
                          const float *table, const int32_t *start, const int64_t *index, const int32_t *row_start,
                          const int32_t *col, const float *weight_coulomb, const float *weight_lj, float *f, double *out8,
                          void *workspace, int64_t workspace_bytes, void *stream)
{
    if (rc) return rc;
    if (!out8) { set_error("Input mismatch: out is null"); return NFFT_HIP_EINVAL; }
    if (p->num_points == 0) {  // (no row of f)
        NFFT_HIP_CHECK(hipMemsetAsync(out8, 0, (size_t)(p->batch_size * 8) * sizeof(double), (hipStream_t)stream));
        return 0;
    }
    if (!points || !xs || (table && !types) || !start || !index || !f) { set_error("Input mismatch: null input"); return NFFT_HIP_EINVAL; }
    char *ws = workspace_base(workspace, workspace_bytes, ewald_step8_near_workspace(p) + 256);
    if (!ws) return NFFT_HIP_EWORKSPACE;
    return launch(p, alpha_dispersion, num_types, num_entries, points, xs, types, table, start, index, row_start, col, weight_coulomb,
                  weight_lj, f, out8, ws, (hipStream_t)stream);
}

int nfft_hip_ewald_lj_step_near(const nfft_hip_ewald_box_problem *p, double alpha_dispersion, const float *points, const float *xs,
                                const int32_t *start, const int64_t *index, float *f, double *out8, void *workspace,
                                int64_t workspace_bytes, void *stream)
{
    const int fault = take_pending_fault();  // a kernel of an earlier call gave up: say so
    return step_near_call(launch_ewald_lj_step_near, fault ? fault : validate_lj_step_near(p, alpha_dispersion), p, alpha_dispersion,
                          0, 0, points, xs, nullptr, nullptr, start, index, nullptr, nullptr, nullptr, nullptr, f, out8, workspace,
                          workspace_bytes, stream);
}

int64_t nfft_hip_ewald_lj_step_spectral_workspace_bytes(int64_t N, int64_t batch_size)
{
    if (validate_lj_step_spectral(N, batch_size)) return -1;
    return ewald_lj_step_spectral_workspace(N, batch_size) + 256;
}

int nfft_hip_ewald_lj_step_spectral(int64_t N, int64_t batch_size, const void *band, const float *coeffs_coulomb,
                                    const float *coeffs_dispersion, const float *strain_dispersion, const double *box_inverse,
                                    double pi2_over_alpha2, void *spectra, double *out8, void *workspace, int64_t workspace_bytes,
                                    void *stream)
{
    if (int rc = take_pending_fault()) return rc;  // a kernel of an earlier call gave up: say so
    if (int rc = validate_lj_step_spectral(N, batch_size)) return rc;
    if (int rc = validate_box_inverse(box_inverse)) return rc;
    if (int rc = check_pi2_over_alpha2(pi2_over_alpha2)) return rc;
    if (!band || !coeffs_coulomb || !coeffs_dispersion || !strain_dispersion || !spectra || !out8) {
        set_error("Input mismatch: null input");
        return NFFT_HIP_EINVAL;
    }
    char *ws = workspace_base(workspace, workspace_bytes, ewald_lj_step_spectral_workspace(N, batch_size) + 256);
    if (!ws) return NFFT_HIP_EWORKSPACE;
    return launch_ewald_lj_step_spectral(N, batch_size, band, coeffs_coulomb, coeffs_dispersion, strain_dispersion, box_inverse,
                                         pi2_over_alpha2, spectra, out8, ws, (hipStream_t)stream);
}

// ---- the same step with bonded-pair exclusions: the checks above, and the list's -------------
static int validate_lj_excl(const nfft_hip_ewald_box_problem *p, double alpha_dispersion, int64_t num_entries, const void *row_start,
                            const void *col, const void *weight_coulomb, const void *weight_lj)
{
    if (int rc = validate_lj_step_near(p, alpha_dispersion)) return rc;
    if (num_entries < 0) { set_error("Input mismatch: negative num_entries"); return NFFT_HIP_EINVAL; }
    if (p->num_points >= (int64_t(1) << 31) || num_entries >= (int64_t(1) << 31)) {
        set_error("Input mismatch: too many points or entries");
        return NFFT_HIP_EINVAL;
    }
    if (p->num_points > 0 && (!row_start || (num_entries > 0 && (!col || !weight_coulomb || !weight_lj)))) {
        set_error("Input mismatch: null list");
        return NFFT_HIP_EINVAL;
    }
    return 0;
}

int64_t nfft_hip_ewald_lj_excl_near_workspace_bytes(const nfft_hip_ewald_box_problem *p, double alpha_dispersion)
{
    return nfft_hip_ewald_lj_step_near_workspace_bytes(p, alpha_dispersion);
}

int nfft_hip_ewald_lj_excl_near(const nfft_hip_ewald_box_problem *p, double alpha_dispersion, int64_t num_entries,
                                const float *points, const float *xs, const int32_t *start, const int64_t *index,
                                const int32_t *row_start, const int32_t *col, const float *weight_coulomb, const float *weight_lj,
                                float *f, double *out8, void *workspace, int64_t workspace_bytes, void *stream)
{
    const int fault = take_pending_fault();  // a kernel of an earlier call gave up: say so
    return step_near_call(
        launch_ewald_lj_step_near,
        fault ? fault : validate_lj_excl(p, alpha_dispersion, num_entries, row_start, col, weight_coulomb, weight_lj), p,
        alpha_dispersion, 0, num_entries, points, xs, nullptr, nullptr, start, index, row_start, col, weight_coulomb, weight_lj, f,
        out8, workspace, workspace_bytes, stream);
}

int64_t nfft_hip_ewald_lj_excl_list_workspace_bytes(const nfft_hip_ewald_box_problem *p, double alpha_dispersion)
{
    if (validate_lj_step_near(p, alpha_dispersion)) return -1;
    return ewald_lj_excl_list_workspace(p) + 256;
}

int nfft_hip_ewald_lj_excl_list(const nfft_hip_ewald_box_problem *p, double alpha_dispersion, int64_t num_entries,
                                const float *points, const float *xs, const int32_t *row_start, const int32_t *col,
                                const float *weight_coulomb, const float *weight_lj, const int32_t *set_start, float *f,
                                double *out8, void *workspace, int64_t workspace_bytes, void *stream)
{
    if (int rc = take_pending_fault()) return rc;  // a kernel of an earlier call gave up: say so
    if (int rc = validate_lj_excl(p, alpha_dispersion, num_entries, row_start, col, weight_coulomb, weight_lj)) return rc;
    if (!out8) { set_error("Input mismatch: out is null"); return NFFT_HIP_EINVAL; }
    if (p->num_points == 0) {  // (no row of f)
        NFFT_HIP_CHECK(hipMemsetAsync(out8, 0, (size_t)(p->batch_size * 8) * sizeof(double), (hipStream_t)stream));
        return 0;
    }
    if (!points || !xs || !f || (p->batch_size > 1 && !set_start)) { set_error("Input mismatch: null input"); return NFFT_HIP_EINVAL; }
    char *ws = workspace_base(workspace, workspace_bytes, ewald_lj_excl_list_workspace(p) + 256);
    if (!ws) return NFFT_HIP_EWORKSPACE;
    return launch_ewald_lj_excl_list(p, alpha_dispersion, num_entries, points, xs, row_start, col, weight_coulomb, weight_lj,
                                     set_start, f, out8, ws, (hipStream_t)stream);
}

// ---- the same walk with a type-pair table (DESIGN.md sections 7t and 7u): the checks above, the table's, and the list's if
// any.  An entry of entry_bytes bytes (8: (C12, dC6); 16: (A, B, dC6, C8)) moves as one load ---
static int validate_step_table(const nfft_hip_ewald_box_problem *p, double alpha_dispersion, int64_t num_types, const void *table,
                               int entry_bytes, int64_t num_entries, const void *row_start, const void *col,
                               const void *weight_coulomb, const void *weight_lj)
{
    if (int rc = validate_lj_step_near(p, alpha_dispersion)) return rc;
    if (num_types < 1 || num_types > 32) { set_error("Input mismatch: num_types must lie in [1, 32]"); return NFFT_HIP_EINVAL; }
    if (!table) { set_error("Input mismatch: table is null"); return NFFT_HIP_EINVAL; }
    if ((uintptr_t)table & (uintptr_t)(entry_bytes - 1)) {
        set_error(entry_bytes == 8 ? "Input mismatch: table must be 8-byte aligned" : "Input mismatch: table must be 16-byte aligned");
        return NFFT_HIP_EINVAL;
    }
    if (p->num_points >= (int64_t(1) << 31)) { set_error("Input mismatch: too many points or entries"); return NFFT_HIP_EINVAL; }
    if (!row_start) {  // no list: the unmasked walk
        if (col || weight_coulomb || weight_lj || num_entries != 0) {
            set_error("Input mismatch: a list without row_start");
            return NFFT_HIP_EINVAL;
        }
        return 0;
    }
    return validate_lj_excl(p, alpha_dispersion, num_entries, row_start, col, weight_coulomb, weight_lj);
}

int64_t nfft_hip_ewald_lj_table_near_workspace_bytes(const nfft_hip_ewald_box_problem *p, double alpha_dispersion)
{
    return nfft_hip_ewald_lj_step_near_workspace_bytes(p, alpha_dispersion);
}

int nfft_hip_ewald_lj_table_near(const nfft_hip_ewald_box_problem *p, double alpha_dispersion, int64_t num_types, int64_t num_entries,
                                 const float *points, const float *xs, const int32_t *types, const float *table,
                                 const int32_t *start, const int64_t *index, const int32_t *row_start, const int32_t *col,
                                 const float *weight_coulomb, const float *weight_lj, float *f, double *out8, void *workspace,
                                 int64_t workspace_bytes, void *stream)
{
    const int fault = take_pending_fault();  // a kernel of an earlier call gave up: say so
    return step_near_call(
        launch_ewald_lj_table_near,
        fault ? fault : validate_step_table(p, alpha_dispersion, num_types, table, 8, num_entries, row_start, col, weight_coulomb, weight_lj),
        p, alpha_dispersion, num_types, num_entries, points, xs, types, table, start, index, row_start, col, weight_coulomb, weight_lj,
        f, out8, workspace, workspace_bytes, stream);
}

// ---- the walk of the Buckingham / Born-Mayer-Huggins step ---
int64_t nfft_hip_ewald_bmh_table_near_workspace_bytes(const nfft_hip_ewald_box_problem *p, double alpha_dispersion)
{
    return nfft_hip_ewald_lj_step_near_workspace_bytes(p, alpha_dispersion);
}

int nfft_hip_ewald_bmh_table_near(const nfft_hip_ewald_box_problem *p, double alpha_dispersion, int64_t num_types, int64_t num_entries,
                                  const float *points, const float *xs, const int32_t *types, const float *table,
                                  const int32_t *start, const int64_t *index, const int32_t *row_start, const int32_t *col,
                                  const float *weight_coulomb, const float *weight_lj, float *f, double *out8, void *workspace,
                                  int64_t workspace_bytes, void *stream)
{
    const int fault = take_pending_fault();  // a kernel of an earlier call gave up: say so
    return step_near_call(
        launch_ewald_bmh_table_near,
        fault ? fault : validate_step_table(p, alpha_dispersion, num_types, table, 16, num_entries, row_start, col, weight_coulomb, weight_lj),
        p, alpha_dispersion, num_types, num_entries, points, xs, types, table, start, index, row_start, col, weight_coulomb, weight_lj,
        f, out8, workspace, workspace_bytes, stream);
}

// ---- the spectral step of the dipole sum -------------------------------------------------------
int nfft_hip_ewald_dipole_spectral(int64_t N, int64_t batch_size, int64_t num_columns, int32_t order, const void *band,
                                   const float *coeffs, const double *box_inverse, void *out, void *stream)
{
    if (int rc = take_pending_fault()) return rc;  // a kernel of an earlier call gave up: say so
    if (int rc = check_dipole_order(order)) return rc;
    if (int rc = validate_virial_far(N, batch_size, num_columns)) return rc;
    if (int rc = check_spectral_elements(N, num_columns)) return rc;
    if (int rc = validate_box_inverse(box_inverse)) return rc;
    if (num_columns == 0) return 0;
    if (!band || !coeffs || !out) { set_error("Input mismatch: null input"); return NFFT_HIP_EINVAL; }
    return launch_ewald_dipole_spectral(N, batch_size, num_columns, order, band, coeffs, box_inverse, out, (hipStream_t)stream);
}

// ---- the spectral step of the Stokeslet sum: the checks of the dipole sum's ---------------------
int nfft_hip_ewald_stokeslet_spectral(int64_t N, int64_t batch_size, int64_t num_columns, int32_t order, const void *band,
                                      const float *coeffs, const double *box_inverse, void *out, void *stream)
{
    if (int rc = take_pending_fault()) return rc;  // a kernel of an earlier call gave up: say so
    if (int rc = check_dipole_order(order)) return rc;
    if (int rc = validate_virial_far(N, batch_size, num_columns)) return rc;
    if (int rc = check_spectral_elements(N, num_columns)) return rc;
    if (int rc = validate_box_inverse(box_inverse)) return rc;
    if (num_columns == 0) return 0;
    if (!band || !coeffs || !out) { set_error("Input mismatch: null input"); return NFFT_HIP_EINVAL; }
    return launch_ewald_stokeslet_spectral(N, batch_size, num_columns, order, band, coeffs, box_inverse, out, (hipStream_t)stream);
}

// ---- virial tensor of the dispersion Ewald sum: the checks and workspaces of section 7i -------
int nfft_hip_ewald_dispersion_virial_near(const nfft_hip_ewald_box_problem *p, const float *points, const float *xr,
                                          const int32_t *start, double *out, void *workspace, int64_t workspace_bytes,
                                          void *stream)
{
    return virial_near_call(launch_ewald_dispersion_virial_near, p, points, xr, start, out, workspace, workspace_bytes, stream);
}

int nfft_hip_ewald_dispersion_virial_far(int64_t N, int64_t batch_size, int64_t num_columns, const void *band,
                                         const float *coeffs, const float *strain_coeffs, const double *box_inverse, double *out,
                                         void *workspace, int64_t workspace_bytes, void *stream)
{
    if (int rc = take_pending_fault()) return rc;  // a kernel of an earlier call gave up: say so
    if (int rc = validate_virial_far(N, batch_size, num_columns)) return rc;
    if (int rc = validate_box_inverse(box_inverse)) return rc;
    if (num_columns == 0) return 0;
    if (!band || !coeffs || !strain_coeffs || !out) { set_error("Input mismatch: null input"); return NFFT_HIP_EINVAL; }
    char *ws = workspace_base(workspace, workspace_bytes, virial_far_need(N, batch_size, num_columns));
    if (!ws) return NFFT_HIP_EWORKSPACE;
    return launch_ewald_dispersion_virial_far(N, batch_size, num_columns, band, coeffs, strain_coeffs, box_inverse, out, ws,
                                              (hipStream_t)stream);
}

// ---- Ewald sum of the screened Coulomb potential: the same problems, checks and workspaces --------
// the screening parameter: finite, not negative, and lambda r_cut <= 50 (float32 exponentials of lambda r leave their range at 88,
// and at 50 the pair weight at the cut is below e^-50 / r_cut); the product is checked once the problem's own r_cut has been (r_cut == nullptr: not yet)
static int check_screening(double screening, const double *r_cut)
{
    if (!(screening >= 0.0) || !(screening < 1e300)) {
        set_error("Input mismatch: screening must be finite and >= 0");
        return NFFT_HIP_EINVAL;
    }
    if (r_cut && !(screening * *r_cut <= 50.0)) {
        set_error("Input mismatch: screening * r_cut <= 50 is required");
        return NFFT_HIP_EINVAL;
    }
    return 0;
}

// (In the three entry points below take_pending_fault and the problem's validation run here, so that the screening is judged
// before the shared checks return early on an empty problem, and once more inside those checks.  The repetition is
// deliberate: the first non-zero return leaves, a taken fault is not reported twice, and the validation only reads.)
int nfft_hip_ewald_yukawa_near(const nfft_hip_ewald_problem *p, const float *points, const float *xr, const int32_t *start,
                               const int64_t *index, double screening, float *z, float *field, void *workspace,
                               int64_t workspace_bytes, void *stream)
{
    if (int rc = take_pending_fault()) return rc;  // a kernel of an earlier call gave up: say so
    if (int rc = check_screening(screening, nullptr)) return rc;
    if (int rc = validate_ewald(p)) return rc;
    if (int rc = check_screening(screening, &p->r_cut)) return rc;
    char *ws;
    if (int rc = ewald_near_checks(p, points, xr, start, index, z, field, workspace, workspace_bytes, &ws)) return rc;
    if (!ws) return 0;
    return launch_ewald_yukawa_near(p, screening, points, xr, start, index, z, field, ws, (hipStream_t)stream);
}

int nfft_hip_ewald_yukawa_near_box(const nfft_hip_ewald_box_problem *p, const float *points, const float *xr,
                                   const int32_t *start, const int64_t *index, double screening, float *z, float *field,
                                   void *workspace, int64_t workspace_bytes, void *stream)
{
    if (int rc = take_pending_fault()) return rc;  // a kernel of an earlier call gave up: say so
    if (int rc = check_screening(screening, nullptr)) return rc;
    if (int rc = validate_ewald_box(p)) return rc;
    if (int rc = check_screening(screening, &p->r_cut)) return rc;
    char *ws;
    if (int rc = ewald_near_box_checks(p, points, xr, start, index, z, field, workspace, workspace_bytes, &ws)) return rc;
    if (!ws) return 0;
    return launch_ewald_yukawa_near_box(p, screening, points, xr, start, index, z, field, ws, (hipStream_t)stream);
}

int nfft_hip_ewald_yukawa_virial_near(const nfft_hip_ewald_box_problem *p, const float *points, const float *xr,
                                      const int32_t *start, double screening, double *out, void *workspace,
                                      int64_t workspace_bytes, void *stream)
{
    if (int rc = take_pending_fault()) return rc;  // a kernel of an earlier call gave up: say so
    if (int rc = check_screening(screening, nullptr)) return rc;
    if (int rc = validate_virial_near(p)) return rc;
    if (int rc = check_screening(screening, &p->r_cut)) return rc;
    char *ws;
    if (int rc = virial_near_checks(p, points, xr, start, out, workspace, workspace_bytes, stream, &ws)) return rc;
    if (!ws) return 0;
    return launch_ewald_yukawa_virial_near(p, screening, points, xr, start, out, ws, (hipStream_t)stream);
}

// ---- bonded-pair exclusions of the Coulomb and dispersion Ewald sums ----------------------------
static int validate_excl(const nfft_hip_ewald_excl_problem *p, bool with_box)
{
    if (!p) { set_error("Input mismatch: null problem"); return NFFT_HIP_EINVAL; }
    if (p->kind != NFFT_HIP_EXCL_COULOMB && p->kind != NFFT_HIP_EXCL_DISPERSION) {
        set_error("Input mismatch: kind must be 0 (Coulomb) or 1 (dispersion)");
        return NFFT_HIP_EINVAL;
    }
    if (p->with_field != 0 && p->with_field != 1) { set_error("Input mismatch: with_field must be 0 or 1"); return NFFT_HIP_EINVAL; }
    if (p->num_points < 0 || p->num_columns < 0 || p->num_entries < 0 || p->batch_size < 1) {
        set_error("Input mismatch: negative size");
        return NFFT_HIP_EINVAL;
    }
    if (p->num_points >= (int64_t(1) << 31) || p->num_entries >= (int64_t(1) << 31)) {
        set_error("Input mismatch: too many points or entries");
        return NFFT_HIP_EINVAL;
    }
    if (!(p->alpha > 0.0) || !(p->alpha < 1e18)) { set_error("Input mismatch: alpha must be positive and finite"); return NFFT_HIP_EINVAL; }
    double w[3];
    if (with_box && !ewald_box_widths(p->box, w)) {
        set_error("Input mismatch: the box must be finite with a positive diagonal");
        return NFFT_HIP_EINVAL;
    }
    return 0;
}

typedef int (*excl_launch)(const nfft_hip_ewald_excl_problem *, const float *, const float *, const int *, const int *,
                           const float *, float *, float *, hipStream_t);
static int excl_call(excl_launch launch, bool with_box, const nfft_hip_ewald_excl_problem *p, const float *points, const float *xr,
                     const int32_t *row_start, const int32_t *col, const float *weight, float *z, float *field, void *stream)
{
    if (int rc = take_pending_fault()) return rc;  // a kernel of an earlier call gave up: say so
    if (int rc = validate_excl(p, with_box)) return rc;
    if (p->num_points == 0 || p->num_columns == 0) return 0;
    if (!z) { set_error("Input mismatch: z is null"); return NFFT_HIP_EINVAL; }
    if (p->with_field && !field) { set_error("Input mismatch: field is null"); return NFFT_HIP_EINVAL; }
    if (!points || !xr || !row_start || (p->num_entries > 0 && (!col || !weight))) {
        set_error("Input mismatch: null input");
        return NFFT_HIP_EINVAL;
    }
    return launch(p, points, xr, row_start, col, weight, z, field, (hipStream_t)stream);
}

int nfft_hip_ewald_excl(const nfft_hip_ewald_excl_problem *p, const float *points, const float *xr, const int32_t *row_start,
                        const int32_t *col, const float *weight, float *z, float *field, void *stream)
{
    return excl_call(launch_ewald_excl, false, p, points, xr, row_start, col, weight, z, field, stream);
}

int nfft_hip_ewald_excl_box(const nfft_hip_ewald_excl_problem *p, const float *points, const float *xr,
                            const int32_t *row_start, const int32_t *col, const float *weight, float *z, float *field,
                            void *stream)
{
    return excl_call(launch_ewald_excl_box, true, p, points, xr, row_start, col, weight, z, field, stream);
}

// the list's own checks, and the second level's launch: one workgroup per point set and column
static int validate_excl_virial(const nfft_hip_ewald_excl_problem *p)
{
    if (int rc = validate_excl(p, true)) return rc;
    if (p->num_columns >= (int64_t(1) << 21) || p->batch_size >= (int64_t(1) << 21) ||
        p->batch_size * p->num_columns >= (int64_t(1) << 21)) {
        set_error("Input mismatch: num_columns < 2^21 and batch_size * num_columns < 2^21 are required");
        return NFFT_HIP_EINVAL;
    }
    return 0;
}

static int64_t excl_virial_need(const nfft_hip_ewald_excl_problem *p) { return ewald_excl_virial_workspace(p) + 256; }

int64_t nfft_hip_ewald_excl_virial_workspace_bytes(const nfft_hip_ewald_excl_problem *p)
{
    if (validate_excl_virial(p)) return -1;
    return excl_virial_need(p);
}

int nfft_hip_ewald_excl_virial(const nfft_hip_ewald_excl_problem *p, const float *points, const float *xr,
                               const int32_t *row_start, const int32_t *col, const float *weight, const int32_t *set_start,
                               double *out, void *workspace, int64_t workspace_bytes, void *stream)
{
    if (int rc = take_pending_fault()) return rc;  // a kernel of an earlier call gave up: say so
    if (int rc = validate_excl_virial(p)) return rc;
    if (p->num_columns == 0) return 0;
    if (!out) { set_error("Input mismatch: out is null"); return NFFT_HIP_EINVAL; }
    if (p->num_points == 0 || p->num_entries == 0) {
        NFFT_HIP_CHECK(hipMemsetAsync(out, 0, (size_t)(p->batch_size * 7 * p->num_columns) * sizeof(double), (hipStream_t)stream));
        return 0;
    }
    if (!points || !xr || !row_start || !col || !weight || (p->batch_size > 1 && !set_start)) {
        set_error("Input mismatch: null input");
        return NFFT_HIP_EINVAL;
    }
    char *ws = workspace_base(workspace, workspace_bytes, excl_virial_need(p));
    if (!ws) return NFFT_HIP_EWORKSPACE;
    return launch_ewald_excl_virial(p, points, xr, row_start, col, weight, set_start, out, ws, (hipStream_t)stream);
}

}  // extern "C"
