// The frame of the pair reductions on top of pair_frame.h: ewald_virial.hip, ewald_disp_virial.hip and
// ewald_yukawa.hip each give a PAIR WEIGHT, and virial_near_kernel<CC, Weight> is the reduction around it, once:
//
//     ewald_near_kernel<CC, true, true>'s items, lanes, LDS tiles, 27-cell walk, image and test 0 < rr < rc2, with seven
//     float32 sums per column -- w v and mg d_a d_b v (xx, yy, zz, yz, xz, xy) -- and no store per point.  At the end of a
//     column pass a lane multiplies its sums by x_i / 2 of its own target (exactly zero for a lane without one), in float64
//     from there on, and the workgroup adds its lanes: a butterfly inside each wave, then the waves in order.  One partial
//     [7, Cr] float64 per item slot; the second level is launch_virial_sum_terms of ewald_virial.hip.  No atomics anywhere
//     and every order of addition is fixed by the launch geometry: two calls give the same bits.
//
// A weight has
//     Params                      its block beside EwaldPairParams, a kernel argument by value (empty where q says it all)
//     weights(rr, q, params, w, mg)   the pair's w and mg = -w'(r) / r from rr = r^2
// -ffp-contract=on fuses within one expression only: a weight's expressions live whole inside the pair weight that it wraps.
//
// Three pieces serve other kernels too.  The epilogue pair_sums_to_partial: ewald_step_near_kernel (ewald_step.hip), which
// hands it seven of its ten sums.  The launch sequence launch_pair_reduction: that kernel and step_near_kernel (step_frame.h).
// The partial store block_sums_to_partial: step_near_kernel and the spectral reductions (spectral_frame.h).
#pragma once
#include "host_util.h"
#include "pair_frame.h"

namespace nfft {

constexpr int kVirialTerms = 7;    // energy, xx, yy, zz, yz, xz, xy
constexpr int kVirialBlock = 256;  // lanes of the spectral reductions and of the second level (virial_sum_kernel)

// The workgroup's sums of v [TERMS, CC] (block_sum_f64), times `scale`, into partial [slot = blockIdx.x, TERMS, C] at the
// columns col0 .. col0 + CC - 1 that exist.  Every thread must be here.
template <int TERMS, int CC, int WAVES>
__device__ __forceinline__ void block_sums_to_partial(const double (&v)[TERMS * CC], double (&s_red)[WAVES][TERMS * CC],
                                                      double scale, int64_t C, int64_t col0, double *__restrict__ partial)
{
    const double r = block_sum_f64(v, s_red);
    const int tid = threadIdx.x;
    if (tid < TERMS * CC) {
        const int e = tid / CC, c = tid % CC;
        if (col0 + c < C) partial[((int64_t)blockIdx.x * TERMS + e) * C + col0 + c] = scale * r;
    }
}

// The epilogue of a column pass of a pair reduction: sum(e, c) is the lane's float32 sum of term e < 7 and column col0 + c.
// x_i / 2 of the lane's own target, float64 from here on; a lane without a target, or a column past Cr, adds exactly zero
template <int CC, typename Sum>
__device__ __forceinline__ void pair_sums_to_partial(const PairLane &lane, const float *__restrict__ xr, int64_t Cr, int64_t col0,
                                                     Sum &&sum, double (&s_red)[kNearBlock / 64][kVirialTerms * CC],
                                                     double *__restrict__ partial)
{
    double red[kVirialTerms * CC];
#pragma unroll
    for (int c = 0; c < CC; ++c) {
        const bool live = lane.active && col0 + c < Cr;
        const double h = live ? 0.5 * (double)xr[(int64_t)lane.ti * Cr + col0 + c] : 0.0;
#pragma unroll
        for (int e = 0; e < kVirialTerms; ++e) red[e * CC + c] = live ? h * (double)sum(e, c) : 0.0;
    }
    block_sums_to_partial<kVirialTerms, CC>(red, s_red, 1.0, Cr, col0, partial);
}

template <int CC, class Weight>
__global__ void __launch_bounds__(kNearBlock) virial_near_kernel(EwaldPairParams q, typename Weight::Params wp,
                                                                 const int2 *__restrict__ items, const float *__restrict__ pos,
                                                                 const float *__restrict__ xr, const int *__restrict__ start,
                                                                 double *__restrict__ partial)
{
    __shared__ float4 s_pos[kNearTile];
    __shared__ __attribute__((aligned(16))) float s_x[kNearTile * CC];
    __shared__ double s_red[kNearBlock / 64][kVirialTerms * CC];
    const int2 item = items[blockIdx.x];
    if (item.x < 0) return;  // (uniform: an empty slot; the second level skips it)
    const PairLane lane = pair_lane(item, start);
    const WrappedWalk walk(lane.cell, q.G0, q.G1, q.G2);
    // (a lane without a target sums pairs of the origin; its sums are replaced by zero before the reduction)
    const float4 t = lane_position(lane, pos, 3, 0.f);
    for (int64_t col0 = 0; col0 < q.Cr; col0 += CC) {
        float acc[kVirialTerms][CC];
#pragma unroll
        for (int e = 0; e < kVirialTerms; ++e)
#pragma unroll
            for (int c = 0; c < CC; ++c) acc[e][c] = 0.f;
        const StageColumns<CC> stage = {s_x, xr, q.Cr, col0};
        walk(start, [&](int first, int last) {
            sweep_range<2>(first, last, lane, s_pos, pos, 3, stage, [&](int j) {
                const PairSep d = ewald_image<true>(t, s_pos[j], q);
                // the lanes that fail the test sit the expansion out
                if (!(d.rr > 0.f && d.rr < q.rc2)) return;
                float w, mg;
                Weight::weights(d.rr, q, wp, w, mg);
                const float gx = mg * d.dx, gy = mg * d.dy, gz = mg * d.dz;
                const float pxx = gx * d.dx, pyy = gy * d.dy, pzz = gz * d.dz;
                const float pyz = gy * d.dz, pxz = gx * d.dz, pxy = gx * d.dy;
#pragma unroll
                for (int c = 0; c < CC; ++c) {
                    const float v = s_x[j * CC + c];
                    acc[0][c] += w * v;
                    acc[1][c] += pxx * v;
                    acc[2][c] += pyy * v;
                    acc[3][c] += pzz * v;
                    acc[4][c] += pyz * v;
                    acc[5][c] += pxz * v;
                    acc[6][c] += pxy * v;
                }
            });
        });
        pair_sums_to_partial<CC>(lane, xr, q.Cr, col0, [&](int e, int c) { return acc[e][c]; }, s_red, partial);
    }
}

// The launch sequence of a pair reduction or step walk on the box problem p.  `workspace`: the work items, then (256-byte
// aligned, ewald_virial_near_partials) one partial [terms, C] per item slot.  The items, then launch(grid, items, partial)
// -- the caller's kernel, one workgroup per item slot -- then the second level over the item slots: out [batch_size, terms, C]
template <typename Launch>
int launch_pair_reduction(const nfft_hip_ewald_box_problem *p, int terms, int64_t C, const int *start, double *out, void *workspace,
                          hipStream_t stream, Launch &&launch)
{
    const int64_t cells_per_set = (int64_t)p->cells[0] * p->cells[1] * p->cells[2];
    int2 *items = (int2 *)workspace;
    double *partial = ewald_virial_near_partials(p, workspace);
    if (int rc = launch_nearfield_items(p->batch_size * cells_per_set, p->num_points, start, items, stream)) return rc;
    launch(dim3((unsigned)ewald_virial_near_item_slots(p)), (const int2 *)items, partial);
    NFFT_HIP_CHECK(hipGetLastError());
    return launch_virial_sum_terms(partial, terms, p->batch_size, C, 0, items, start, (int)cells_per_set, out, stream);
}

// ... of virial_near_kernel with the weight's block `wp`: arguments as launch_ewald_virial_near
template <class Weight>
int launch_virial_near(const nfft_hip_ewald_box_problem *p, const typename Weight::Params &wp, const float *pos, const float *xr,
                       const int *start, double *out, void *workspace, hipStream_t stream)
{
    const EwaldPairParams q = ewald_pair_params(p->cells[0], p->cells[1], p->cells[2], p->num_columns, p->alpha, p->r_cut, p->box);
    return launch_pair_reduction(p, kVirialTerms, q.Cr, start, out, workspace, stream,
                                 [&](dim3 grid, const int2 *items, double *partial) {
                                     dispatch_columns(q.Cr, [&](auto CC) {
                                         hipLaunchKernelGGL((virial_near_kernel<CC(), Weight>), grid, dim3(kNearBlock), 0, stream, q, wp,
                                                            items, pos, xr, start, partial);
                                     });
                                 });
}

}  // namespace nfft
