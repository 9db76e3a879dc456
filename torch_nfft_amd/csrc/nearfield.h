// What the near-field pair kernels share besides their frame (nearfield.hip: the value, DESIGN.md section 7d;
// nearfield_grad.hip: the gradient at the targets and its transpose, section 7e; nearfield_pgrad.hip: the gradient with
// respect to the points, section 7f): the sizes of a work item and of an LDS tile, the parameter block, K'(r) / r and the
// work-item list.  The wrapped pair kernels of the Ewald sum (ewald_near.hip, ewald_virial.hip, sections 7g-7i) take the
// sizes and the work-item list from here too.  The frame itself -- lane decode, walks, tile sweep -- is pair_frame.h.
#pragma once
#include "common.h"
#include "kernels.h"

namespace nfft {

constexpr int kNearBlock = 128;  // output points of a work item = lanes of its workgroup (two waves)
constexpr int kNearTile = 256;   // streamed points per LDS tile: 4 KiB of positions + 4 bytes per staged value each

struct NearParams {
    int dim, G, terms;
    int64_t Cr;
    float c2, inv_c, inv_c2;  // shape parameter: c^2, 1/c, 1/c^2
    float eps2, inv_eps2;     // eps_I^2 and its inverse
    float poly[8];            // the Horner coefficients in u = r^2 / eps_I^2, zero past `terms`
};

// the block of a problem with `terms` coefficients `poly` (float64 on the host, rounded once)
inline NearParams near_params(const nfft_hip_nearfield_problem *p, const double *poly, int terms)
{
    NearParams q;
    q.dim = p->dim;
    q.G = p->cells_per_axis;
    q.terms = terms;
    q.Cr = p->num_columns;
    q.c2 = (float)(p->c * p->c);
    q.inv_c = p->c > 0.0 ? (float)(1.0 / p->c) : 0.f;
    q.inv_c2 = p->c > 0.0 ? (float)(1.0 / (p->c * p->c)) : 0.f;
    q.eps2 = (float)(p->eps_I * p->eps_I);
    q.inv_eps2 = (float)(1.0 / (p->eps_I * p->eps_I));
    for (int e = 0; e < 8; ++e) q.poly[e] = e < terms ? (float)poly[e] : 0.f;
    return q;
}

// K'(r) / r from r^2 > 0: one rsqrt, rcp, log or exp (the Laplacian RBF needs r itself as well: two)
template <int KERNEL>
__device__ __forceinline__ float kernel_slope(float r2, const NearParams &q)
{
    if (KERNEL == NFFT_HIP_KERNEL_ONE_OVER_MODULUS) {  // -r^-3
        const float i = rsqrtf(r2);
        return -(i * i) * i;
    }
    if (KERNEL == NFFT_HIP_KERNEL_ONE_OVER_SQUARE) {  // -2 r^-4
        const float i = __builtin_amdgcn_rcpf(r2);
        return -2.0f * (i * i);
    }
    if (KERNEL == NFFT_HIP_KERNEL_LOGARITHM) return __builtin_amdgcn_rcpf(r2);       // r^-2
    if (KERNEL == NFFT_HIP_KERNEL_THINPLATE_SPLINE) return logf(r2) + 1.0f;           // 2 log r + 1
    if (KERNEL == NFFT_HIP_KERNEL_MULTIQUADRIC) return rsqrtf(r2 + q.c2);             // (r^2 + c^2)^(-1/2)
    if (KERNEL == NFFT_HIP_KERNEL_INVERSE_MULTIQUADRIC) {                             // -(r^2 + c^2)^(-3/2)
        const float i = rsqrtf(r2 + q.c2);
        return -(i * i) * i;
    }
    if (KERNEL == NFFT_HIP_KERNEL_GAUSSIAN) return -2.0f * q.inv_c2 * expf(-r2 * q.inv_c2);  // -(2 / c^2) e^(-r^2 / c^2)
    const float i = rsqrtf(r2);  // NFFT_HIP_KERNEL_LAPLACIAN_RBF: -e^(-r / c) / (c r)
    return -(q.inv_c * i) * expf(-(r2 * i) * q.inv_c);
}

// nearfield.hip: fills items[0 .. nearfield_item_slots(p)) with (cell, first output point) of every piece of kNearBlock
// output points of one cell, -1 in the slots that stay empty; tstart is the output side's start table
int launch_nearfield_items(const nfft_hip_nearfield_problem *p, const int *tstart, int2 *items, hipStream_t stream);
// the same for a table of `cells` cells (all point sets) over `num_targets` output points: nearfield_item_slots(cells,
// num_targets) slots (ewald_near.hip cuts its full-box grid with it)
int64_t nearfield_item_slots(int64_t cells, int64_t num_targets);
int launch_nearfield_items(int64_t cells, int64_t num_targets, const int *tstart, int2 *items, hipStream_t stream);

}  // namespace nfft
