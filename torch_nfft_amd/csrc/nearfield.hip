// Near field of the fast summation for singular kernels: the pair sum
//
//     z_i = sum_{j in the point set of i, |t_i - s_j| < eps_I} (K(r_ij) - T_I(r_ij)) x_j,      r_ij = |t_i - s_j|,
//
// that turns the NFFT sum of the regularised kernel K_R (T_I inside eps_I) back into the sum of K itself (Potts, Steidl,
// Nieslony 2004).  No reference counterpart: the reference sums smooth kernels only.
//
// The caller hands in both point sets ordered by (point set, cell) of a grid of G^dim cubes of edge 1/(2G) >= eps_I over
// [-1/4, 1/4]^dim, cell index c_0 + G c_1 + G^2 c_2, with the first point of every cell (start tables).  A target meets
// sources of its own and the 3^dim - 1 neighbouring cells only; along axis 0 the three neighbours are consecutive cells, so
// the walk is over 3^(dim-1) contiguous source ranges ("rows").
//
// nearfield_items_kernel   one thread per cell: cuts the cell's targets into work items of kNearBlock
// nearfield_kernel         the tiled N-body loop on the frame of pair_frame.h.  A workgroup owns one item, a lane one
//                          target; the sources of a row stream through LDS in tiles of kNearTile (position as one float4,
//                          CC columns of x); every lane reads the same source (an LDS broadcast) and keeps its CC sums in
//                          registers: its own are the pair weight K - T_I and one sum per column.  The loop is bound by
//                          the VALU: about 20 instructions and one transcendental per pair against one or two 16-byte LDS
//                          broadcasts.  No atomics: a target's pairs are added in the order of the sorted sources.
#include "pair_frame.h"

namespace nfft {

namespace {

// K(r) from r^2.  The kernels that are singular at 0 return 0 there: the self term is left out of the sum.
template <int KERNEL>
__device__ __forceinline__ float kernel_value(float r2, const NearParams &q)
{
    if (KERNEL == NFFT_HIP_KERNEL_ONE_OVER_MODULUS) return r2 > 0.f ? rsqrtf(r2) : 0.f;
    if (KERNEL == NFFT_HIP_KERNEL_ONE_OVER_SQUARE) return r2 > 0.f ? 1.0f / r2 : 0.f;
    if (KERNEL == NFFT_HIP_KERNEL_LOGARITHM) return r2 > 0.f ? 0.5f * logf(r2) : 0.f;
    if (KERNEL == NFFT_HIP_KERNEL_THINPLATE_SPLINE) return r2 > 0.f ? 0.5f * r2 * logf(r2) : 0.f;
    if (KERNEL == NFFT_HIP_KERNEL_MULTIQUADRIC) return sqrtf(r2 + q.c2);
    if (KERNEL == NFFT_HIP_KERNEL_INVERSE_MULTIQUADRIC) return rsqrtf(r2 + q.c2);
    if (KERNEL == NFFT_HIP_KERNEL_GAUSSIAN) return expf(-r2 * q.inv_c2);
    return expf(-sqrtf(r2) * q.inv_c);  // NFFT_HIP_KERNEL_LAPLACIAN_RBF
}

// items[slot] = (cell, first target) for slot = first / kNearBlock + cell + piece: distinct for all pieces of all cells
// (the pieces of a cell end at or before slot (end of the cell) / kNearBlock + cell, the next cell starts one later).
// The slots nobody writes keep the -1 they were filled with.
__global__ void __launch_bounds__(256) nearfield_items_kernel(const int *__restrict__ tstart, int ncells, int2 *__restrict__ items)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= ncells) return;
    const int ts = tstart[k], te = tstart[k + 1];
    int64_t slot = (int64_t)(ts / kNearBlock) + k;
    for (int t = ts; t < te; t += kNearBlock, ++slot) items[slot] = make_int2(k, t);
}

// PT: Horner terms, 4 or 8; the coefficients past `terms` are zero, which leaves the sum of the others bit for bit
template <int KERNEL, int CC, int PT>
__global__ void __launch_bounds__(kNearBlock) nearfield_kernel(NearParams q, const int2 *__restrict__ items,
                                                               const float *__restrict__ src, const float *__restrict__ xr,
                                                               const int *__restrict__ sstart, const float *__restrict__ tgt,
                                                               const int64_t *__restrict__ tindex,
                                                               const int *__restrict__ tstart, float *__restrict__ z)
{
    __shared__ float4 s_pos[kNearTile];
    __shared__ __attribute__((aligned(16))) float s_x[kNearTile * CC];
    const int2 item = items[blockIdx.x];
    if (item.x < 0) return;  // (uniform: an empty slot)
    const PairLane lane = pair_lane(item, tstart);
    const OpenWalk walk(lane.cell, q.dim, q.G);
    // a lane without a target sits far away: every pair fails the distance test
    const float4 t = lane_position(lane, tgt, q.dim, 1e9f);
    float a[PT];
#pragma unroll
    for (int e = 0; e < PT; ++e) a[e] = q.poly[e];
    for (int64_t col0 = 0; col0 < q.Cr; col0 += CC) {
        float acc[CC];
#pragma unroll
        for (int c = 0; c < CC; ++c) acc[c] = 0.f;
        const StageColumns<CC> stage = {s_x, xr, q.Cr, col0};
        walk(sstart, [&](int first, int last) {
            sweep_range<4>(first, last, lane, s_pos, src, q.dim, stage, [&](int j) {
                const PairSep d = open_sep(t, s_pos[j]);
                const float ti = horner(a, d.rr * q.inv_eps2);
                const float w = d.rr < q.eps2 ? kernel_value<KERNEL>(d.rr, q) - ti : 0.f;
#pragma unroll
                for (int c = 0; c < CC; ++c) acc[c] += w * s_x[j * CC + c];
            });
        });
        if (lane.active) {
            float *zp = z + tindex[lane.ti] * q.Cr + col0;
#pragma unroll
            for (int c = 0; c < CC; ++c)
                if (col0 + c < q.Cr) zp[c] = acc[c];
        }
    }
}

}  // namespace

namespace {
int64_t nearfield_cells(const nfft_hip_nearfield_problem *p)
{
    int64_t cells = p->batch_size;
    for (int a = 0; a < p->dim; ++a) cells *= p->cells_per_axis;
    return cells;
}
}  // namespace

int64_t nearfield_item_slots(int64_t cells, int64_t num_targets) { return num_targets / kNearBlock + cells + 1; }

int64_t nearfield_item_slots(const nfft_hip_nearfield_problem *p)
{
    return nearfield_item_slots(nearfield_cells(p), p->num_targets);
}

int launch_nearfield_items(int64_t cells, int64_t num_targets, const int *tstart, int2 *items, hipStream_t stream)
{
    NFFT_HIP_CHECK(hipMemsetAsync(items, 0xFF, (size_t)nearfield_item_slots(cells, num_targets) * sizeof(int2), stream));
    hipLaunchKernelGGL(nearfield_items_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, stream, tstart, (int)cells,
                       items);
    NFFT_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_nearfield_items(const nfft_hip_nearfield_problem *p, const int *tstart, int2 *items, hipStream_t stream)
{
    return launch_nearfield_items(nearfield_cells(p), p->num_targets, tstart, items, stream);
}

int launch_nearfield(const nfft_hip_nearfield_problem *p, const float *src, const float *xr, const int *sstart,
                     const float *tgt, const int64_t *tindex, const int *tstart, float *z, void *items, hipStream_t stream)
{
    const NearParams q = near_params(p, p->poly, p->poly_terms);
    const int64_t slots = nearfield_item_slots(p);
    if (int rc = launch_nearfield_items(p, tstart, (int2 *)items, stream)) return rc;
    const dim3 grid((unsigned)slots), block(kNearBlock);
    dispatch_kernel(p->kernel, [&](auto K) {
        dispatch_columns(q.Cr, [&](auto CC) {
            dispatch_terms(q.terms, [&](auto PT) {
                hipLaunchKernelGGL((nearfield_kernel<K(), CC(), PT()>), grid, block, 0, stream, q, (const int2 *)items, src, xr,
                                   sstart, tgt, tindex, tstart, z);
            });
        });
    });
    NFFT_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace nfft
