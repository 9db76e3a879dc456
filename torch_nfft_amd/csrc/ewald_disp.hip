// Near part of the Ewald sum for the periodic 1/r^6, the dispersion sum: for one point set on both
// sides, with a = alpha r,
//
//     z[i, c]    =  sum_{j: 0 < r_ij < r_c} w(r_ij) xr[j, c],             w(r)  = e^(-a^2) (1 + a^2 + a^4 / 2) / r^6
//     f[i, a, c] =  sum_{j: 0 < r_ij < r_c} mg(r_ij) d_ij[a] xr[j, c],    mg(r) = -w'(r) / r = e^(-a^2) (6 + 6 a^2 + 3 a^4 + a^6) / r^8,
//
// d_ij the minimum image of x_i - x_j and r_ij its length.  The twin of ewald_near_kernel (ewald_near.hip, sections 7g and
// 7h), which says what BOX = false (the unit torus) and BOX = true (fractional positions in a lower-triangular box) mean:
// the same frame of pair_frame.h, the same wrapped walk, image, distance branch, staging and epilogue.  Its own is the
// pair weight (DispersionPairWeight): one reciprocal of r^2, one __expf and two Horner forms in a^2, no erfc expansion.
#include "pair_frame.h"

namespace nfft {

namespace {

template <int CC, bool FIELD, bool BOX>
__global__ void __launch_bounds__(kNearBlock) ewald_disp_near_kernel(EwaldPairParams q, const int2 *__restrict__ items,
                                                                     const float *__restrict__ pos, const float *__restrict__ xr,
                                                                     const int *__restrict__ start,
                                                                     const int64_t *__restrict__ index, float *__restrict__ z,
                                                                     float *__restrict__ f)
{
    __shared__ float4 s_pos[kNearTile];
    __shared__ __attribute__((aligned(16))) float s_x[kNearTile * CC];
    const int2 item = items[blockIdx.x];
    if (item.x < 0) return;  // (uniform: an empty slot)
    const PairLane lane = pair_lane(item, start);
    const WrappedWalk walk(lane.cell, q.G0, BOX ? q.G1 : q.G0, BOX ? q.G2 : q.G0);  // (cubic: one count, one division)
    // (a lane without a target sums pairs of the origin and stores nothing)
    const float4 t = lane_position(lane, pos, 3, 0.f);
    for (int64_t col0 = 0; col0 < q.Cr; col0 += CC) {
        float acc[CC];
        float fx[FIELD ? CC : 1], fy[FIELD ? CC : 1], fz[FIELD ? CC : 1];
#pragma unroll
        for (int c = 0; c < CC; ++c) acc[c] = 0.f;
#pragma unroll
        for (int c = 0; c < (FIELD ? CC : 1); ++c) fx[c] = fy[c] = fz[c] = 0.f;
        const StageColumns<CC> stage = {s_x, xr, q.Cr, col0};
        walk(start, [&](int first, int last) {
            sweep_range<2>(first, last, lane, s_pos, pos, 3, stage, [&](int j) {
                const PairSep d = ewald_image<BOX>(t, s_pos[j], q);
                if (!(d.rr > 0.f && d.rr < q.rc2)) return;
                const DispersionPairWeight e(d.rr, q);
#pragma unroll
                for (int c = 0; c < CC; ++c) acc[c] += e.w * s_x[j * CC + c];
                if (FIELD) {
                    const float mg = e.mg();
                    const float gx = mg * d.dx, gy = mg * d.dy, gz = mg * d.dz;
#pragma unroll
                    for (int c = 0; c < (FIELD ? CC : 1); ++c) {
                        const float v = s_x[j * CC + c];
                        fx[c] += gx * v;
                        fy[c] += gy * v;
                        fz[c] += gz * v;
                    }
                }
            });
        });
        if (lane.active) {
            const int64_t row = index[lane.ti];
            float *zp = z + row * q.Cr + col0;
#pragma unroll
            for (int c = 0; c < CC; ++c)
                if (col0 + c < q.Cr) zp[c] = acc[c];
            if (FIELD) {
                float *fp = f + row * 3 * q.Cr + col0;
#pragma unroll
                for (int c = 0; c < (FIELD ? CC : 1); ++c)
                    if (col0 + c < q.Cr) {
                        fp[c] = fx[c];
                        fp[q.Cr + c] = fy[c];
                        fp[2 * q.Cr + c] = fz[c];
                    }
            }
        }
    }
}

// the items of `cells` cells over `num_points` points into `slots` slots, then the pair kernel
template <bool BOX>
int launch_pairs(const EwaldPairParams &q, int64_t cells, int64_t slots, int64_t num_points, bool with_field, const float *pos,
                 const float *xr, const int *start, const int64_t *index, float *z, float *f, void *items, hipStream_t stream)
{
    if (int rc = launch_nearfield_items(cells, num_points, start, (int2 *)items, stream)) return rc;
    const dim3 grid((unsigned)slots), block(kNearBlock);
    dispatch_flag(with_field, [&](auto FIELD) {
        dispatch_columns(q.Cr, [&](auto CC) {
            hipLaunchKernelGGL((ewald_disp_near_kernel<CC(), FIELD() != 0, BOX>), grid, block, 0, stream, q, (const int2 *)items,
                               pos, xr, start, index, z, f);
        });
    });
    NFFT_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace

// (the cell counts and the item slots are those of ewald_near.hip: one workspace serves both sweeps)
int launch_ewald_dispersion_near(const nfft_hip_ewald_problem *p, const float *pos, const float *xr, const int *start,
                                 const int64_t *index, float *z, float *f, void *items, hipStream_t stream)
{
    const int G = p->cells_per_axis;
    const EwaldPairParams q = ewald_pair_params(G, G, G, p->num_columns, p->alpha, p->r_cut, nullptr);
    return launch_pairs<false>(q, p->batch_size * G * G * G, ewald_near_item_slots(p), p->num_points, p->with_field != 0, pos, xr,
                               start, index, z, f, items, stream);
}

int launch_ewald_dispersion_near_box(const nfft_hip_ewald_box_problem *p, const float *pos, const float *xr, const int *start,
                                     const int64_t *index, float *z, float *f, void *items, hipStream_t stream)
{
    const EwaldPairParams q = ewald_pair_params(p->cells[0], p->cells[1], p->cells[2], p->num_columns, p->alpha, p->r_cut, p->box);
    return launch_pairs<true>(q, p->batch_size * p->cells[0] * p->cells[1] * p->cells[2], ewald_near_box_item_slots(p),
                              p->num_points, p->with_field != 0, pos, xr, start, index, z, f, items, stream);
}

}  // namespace nfft
