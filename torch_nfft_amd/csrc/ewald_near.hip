// Near part of the Ewald sum for the periodic 1/r (DESIGN.md sections 7g and 7h): for one point set on both sides
//
//     z[i, c]    =  sum_{j: 0 < r_ij < r_c} erfc(alpha r_ij) / r_ij  xr[j, c]
//     f[i, a, c] = -sum_{j: 0 < r_ij < r_c} g(r_ij^2) d_ij[a] xr[j, c],     g = K'(r) / r for K = erfc(alpha r) / r,
//
// d_ij the minimum image of x_i - x_j and r_ij its length.  One kernel template for the two geometries:
//
// BOX = false  the unit torus, x in [-1/2, 1/2)^3: G^3 cells of edge 1/G >= r_c, d = dx - rint(dx);
// BOX = true   an orthorhombic or triclinic box with the lower-triangular matrix A (rows = lattice vectors).  The kernel
//              holds FRACTIONAL positions s in [-1/2, 1/2)^3, x = s A: G0 x G1 x G2 cells of fractional edge 1 / G_a,
//              G_a <= w_a / r_c for the perpendicular width w_a of the box along axis a, cell index c0 + G0 (c1 + G1 c2);
//              ds is wrapped componentwise, then d = ds A (three products and three FMAs for the lower triangle).  alpha,
//              r_c, z and f are in the box's own Cartesian units.  Under r_c <= w_a / 3 an image with |d| < r_c has
//              |ds_a| <= |d| / w_a < 1/3 on every axis, so the componentwise wrap IS that image, it is the only one, and it
//              lies in one of the 27 cells: no lattice search at any tilt.
//
// The kernel stands on the frame of pair_frame.h -- work items of kNearBlock targets of one cell,
// one lane per target, the sources streamed through LDS in tiles of kNearTile as one float4 broadcast per pair, CC columns
// of sums in registers, no atomics -- with the wrapped walk: the cells cover the WHOLE torus, the rows wrap with G1 and G2,
// and within a row the cells c0 - 1 .. c0 + 1 are one contiguous range of sources for 0 < c0 < G0 - 1 and two at either end
// of the row.  Every G_a >= 3 makes the 27 cells distinct, so no pair is met twice.  Its own: the image and the distance
// test as a branch, the pair weights, and one or four sums per column.
//
// The loop is bound by the VALU: the expansion of erfcf (see DESIGN.md 7g for the measurement).
#include "pair_frame.h"

namespace nfft {

namespace {

template <int CC, bool FIELD, bool BOX>
__global__ void __launch_bounds__(kNearBlock) ewald_near_kernel(EwaldPairParams q, const int2 *__restrict__ items,
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
                // about one pair in six of the 27 cells passes: the lanes that fail sit the expansion out
                if (!(d.rr > 0.f && d.rr < q.rc2)) return;
                const EwaldPairWeight e(d.rr, q);
#pragma unroll
                for (int c = 0; c < CC; ++c) acc[c] += e.w * s_x[j * CC + c];
                if (FIELD) {
                    const float mg = e.mg(q);
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

// the items of `cells` cells over `num_points` points, then the pair kernel
template <bool BOX>
int launch_pairs(const EwaldPairParams &q, int64_t cells, int64_t num_points, bool with_field, const float *pos, const float *xr,
                 const int *start, const int64_t *index, float *z, float *f, void *items, hipStream_t stream)
{
    if (int rc = launch_nearfield_items(cells, num_points, start, (int2 *)items, stream)) return rc;
    const dim3 grid((unsigned)nearfield_item_slots(cells, num_points)), block(kNearBlock);
    dispatch_flag(with_field, [&](auto FIELD) {
        dispatch_columns(q.Cr, [&](auto CC) {
            hipLaunchKernelGGL((ewald_near_kernel<CC(), FIELD() != 0, BOX>), grid, block, 0, stream, q, (const int2 *)items, pos,
                               xr, start, index, z, f);
        });
    });
    NFFT_HIP_CHECK(hipGetLastError());
    return 0;
}

int64_t ewald_cells(const nfft_hip_ewald_problem *p)
{
    return p->batch_size * p->cells_per_axis * p->cells_per_axis * p->cells_per_axis;
}

int64_t ewald_box_cells(const nfft_hip_ewald_box_problem *p)
{
    return p->batch_size * p->cells[0] * p->cells[1] * p->cells[2];
}

}  // namespace

int64_t ewald_near_item_slots(const nfft_hip_ewald_problem *p) { return nearfield_item_slots(ewald_cells(p), p->num_points); }

int64_t ewald_near_box_item_slots(const nfft_hip_ewald_box_problem *p)
{
    return nearfield_item_slots(ewald_box_cells(p), p->num_points);
}

int launch_ewald_near(const nfft_hip_ewald_problem *p, const float *pos, const float *xr, const int *start,
                      const int64_t *index, float *z, float *f, void *items, hipStream_t stream)
{
    const int G = p->cells_per_axis;
    const EwaldPairParams q = ewald_pair_params(G, G, G, p->num_columns, p->alpha, p->r_cut, nullptr);
    return launch_pairs<false>(q, ewald_cells(p), p->num_points, p->with_field != 0, pos, xr, start, index, z, f, items, stream);
}

int launch_ewald_near_box(const nfft_hip_ewald_box_problem *p, const float *pos, const float *xr, const int *start,
                          const int64_t *index, float *z, float *f, void *items, hipStream_t stream)
{
    const EwaldPairParams q = ewald_pair_params(p->cells[0], p->cells[1], p->cells[2], p->num_columns, p->alpha, p->r_cut, p->box);
    return launch_pairs<true>(q, ewald_box_cells(p), p->num_points, p->with_field != 0, pos, xr, start, index, z, f, items, stream);
}

}  // namespace nfft
