// Virial tensor of the Ewald sum for the periodic 1/r: the two reductions that the potential and
// field kernels do not do.  For the homogeneous strain A -> A (1 + eps) at fixed fractional coordinates,
// W_ab = -dU / d eps_ab is the sum of a pair part, a spectral part and the background term (added by the host side):
//
//     near[b, 0, c]  = 1/2 sum_{i in set b} x_ic sum_{j: 0 < r_ij < r_c} erfc(alpha r_ij) / r_ij  x_jc          (energy)
//     near[b, e, c]  = 1/2 sum_i x_ic sum_j (-g(r_ij^2)) d_ij,a d_ij,b x_jc,   e = 1 .. 6: ab = xx, yy, zz, yz, xz, xy
//     far[b, 0, c]   = 1/2 sum_k b_k |band_k|^2                                                                  (energy)
//     far[b, e, c]   = 1/2 sum_k b_k |band_k|^2 (delta_ab - 2 (1 / |kappa|^2 + pi^2 / alpha^2) kappa_a kappa_b)
//
// with g = K'(r) / r for K = erfc(alpha r) / r, d_ij = (ds - rint(ds)) A and kappa = A^-1 k, as in ewald_near.hip.
//
// Both reductions are the frames' (DESIGN.md section 7w), which say what they do:
// virial_near_kernel<CC, CoulombVirialWeight>  of virial_frame.h with the pair weights of ewald_near_kernel
//                                              (until 7w: ewald_virial_near_kernel<CC>).
// virial_far_kernel<CC, CoulombStrain>         of spectral_frame.h with the closed form of t_k; the cells that it skips are
//                                              k = 0 and the zeroed planes k_a = -N/2 (until 7w: ewald_virial_far_kernel<CC>).
// virial_sum_kernel                            here: the second level of both, one workgroup per (point set, column) adds
//                                              that set's partials, each thread a fixed stride of them in order, then the
//                                              workgroup sum.
//
// The second level, the workspaces and their layout serve every reduction on the two frames through launch_virial_sum_terms,
// ewald_virial_near_item_slots / _partials and ewald_virial_far_blocks.
//
// No atomics anywhere and every order of addition is fixed by the launch geometry: two calls give the same bits.
#include "spectral_frame.h"

namespace nfft {

namespace {

constexpr int kVirialFarBlocks = 1024;  // workgroups per point set of a spectral reduction, at most

// the pair weight of the Coulomb sum (virial_frame.h has what a weight is): EwaldPairWeight, no block of its own
struct CoulombVirialWeight {
    struct Params {};
    static __device__ __forceinline__ void weights(float rr, const EwaldPairParams &q, const Params &, float &w, float &mg)
    {
        const EwaldPairWeight e(rr, q);
        w = e.w;
        mg = e.mg(q);
    }
};

// out[b, e, c] = sum of partial[row, e, c] over the rows of point set b, column c (one workgroup each,
// blockIdx.x = b C + c), e < terms: seven here and in the sums that share this level, eight in ewald_lj_step.hip (section 7r).
// items == nullptr: the rows are b * rows_per_set ... (b + 1) * rows_per_set.  Otherwise the rows are the item slots of the
// set's cells: slot = first point / kNearBlock + cell + piece grows with the cell, so they are the slots from that of the
// set's first cell up to that of the next set's first cell.  The last slot of a cell lies before the first slot of the next
// cell, so that range holds items of set b (item.x / cells_per_set == b) and empty slots (item.x < 0, skipped), no others.
__global__ void __launch_bounds__(kVirialBlock) virial_sum_kernel(const double *__restrict__ partial, int terms, int64_t C,
                                                                  int rows_per_set, const int2 *__restrict__ items,
                                                                  const int *__restrict__ start, int cells_per_set,
                                                                  double *__restrict__ out)
{
    __shared__ double s_red[kVirialBlock / 64][1];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x / C, c = blockIdx.x % C;
    int64_t lo, hi;
    if (items) {
        const int64_t k0 = b * cells_per_set, k1 = (b + 1) * cells_per_set;
        lo = start[k0] / kNearBlock + k0;
        hi = start[k1] / kNearBlock + k1;
    } else {
        lo = b * rows_per_set;
        hi = lo + rows_per_set;
    }
    for (int e = 0; e < terms; ++e) {
        double v = 0.0;
        for (int64_t row = lo + tid; row < hi; row += kVirialBlock) {
            if (items) {
                const int cell = items[row].x;
                if (cell < 0) continue;
            }
            v += partial[(row * terms + e) * C + c];
        }
        const double sum[1] = {v};
        const double r = block_sum_f64(sum, s_red);
        if (tid == 0) out[(b * terms + e) * C + c] = r;
    }
}

int64_t virial_cells(const nfft_hip_ewald_box_problem *p)
{
    return p->batch_size * p->cells[0] * p->cells[1] * p->cells[2];
}

int virial_far_blocks(int64_t N)
{
    const int64_t cells = N * N * N;
    return (int)std::min<int64_t>((cells + kVirialBlock - 1) / kVirialBlock, kVirialFarBlocks);
}

}  // namespace

int ewald_virial_far_blocks(int64_t N) { return virial_far_blocks(N); }

// the second level on `partial` [rows, terms, C]: out [batch_size, terms, C]; the rows of a point set as virial_sum_kernel
// takes them
int launch_virial_sum_terms(const double *partial, int terms, int64_t batch_size, int64_t C, int rows_per_set, const void *items,
                            const int *start, int cells_per_set, double *out, hipStream_t stream)
{
    hipLaunchKernelGGL(virial_sum_kernel, dim3((unsigned)(batch_size * C)), dim3(kVirialBlock), 0, stream, partial, terms, C,
                       rows_per_set, (const int2 *)items, start, cells_per_set, out);
    NFFT_HIP_CHECK(hipGetLastError());
    return 0;
}

// ... with the seven terms of a virial
int launch_virial_sum(const double *partial, int64_t batch_size, int64_t C, int rows_per_set, const void *items, const int *start,
                      int cells_per_set, double *out, hipStream_t stream)
{
    return launch_virial_sum_terms(partial, kVirialTerms, batch_size, C, rows_per_set, items, start, cells_per_set, out, stream);
}

int64_t ewald_virial_near_item_slots(const nfft_hip_ewald_box_problem *p)
{
    return nearfield_item_slots(virial_cells(p), p->num_points);
}

int64_t ewald_virial_near_workspace(const nfft_hip_ewald_box_problem *p)
{
    const int64_t slots = ewald_virial_near_item_slots(p);
    return round256(slots * (int64_t)sizeof(int2)) + slots * kVirialTerms * p->num_columns * (int64_t)sizeof(double);
}

// the near workspace: the work items, then (256-byte aligned) one partial per item slot
double *ewald_virial_near_partials(const nfft_hip_ewald_box_problem *p, void *workspace)
{
    return (double *)((char *)workspace + round256(ewald_virial_near_item_slots(p) * (int64_t)sizeof(int2)));
}

int launch_ewald_virial_near(const nfft_hip_ewald_box_problem *p, const float *pos, const float *xr, const int *start,
                             double *out, void *workspace, hipStream_t stream)
{
    return launch_virial_near<CoulombVirialWeight>(p, {}, pos, xr, start, out, workspace, stream);
}

int64_t ewald_virial_far_workspace(int64_t N, int64_t batch_size, int64_t num_columns)
{
    return batch_size * virial_far_blocks(N) * kVirialTerms * num_columns * (int64_t)sizeof(double);
}

int launch_ewald_virial_far(int64_t N, int64_t batch_size, int64_t num_columns, const void *band, const float *coeffs,
                            const double *box_inverse, double pi2_over_alpha2, double *out, void *workspace,
                            hipStream_t stream)
{
    return launch_virial_far(N, batch_size, num_columns, band, coeffs, box_inverse, CoulombStrain{pi2_over_alpha2}, out, workspace,
                             stream);
}

}  // namespace nfft
