// Near part of the Ewald sum for the periodic 1/r in an orthorhombic or triclinic box: the sibling
// of ewald_near.hip for a cell with the lower-triangular matrix A (rows = lattice vectors).  The kernel holds FRACTIONAL
// positions s in [-1/2, 1/2)^3, x = s A, and sums over one point set on both sides
//
//     z[i, c]    =  sum_{j: 0 < r_ij < r_c} erfc(alpha r_ij) / r_ij  xr[j, c]
//     f[i, a, c] = -sum_{j: 0 < r_ij < r_c} g(r_ij^2) d_ij[a] xr[j, c],     g = K'(r) / r for K = erfc(alpha r) / r,
//
// d_ij = (ds - rint(ds)) A the Cartesian image of s_i - s_j and r_ij its length: alpha, r_c, z and f are in the box's own
// Cartesian units.  The frame is that of ewald_near.hip, which stays as it is -- points ordered by (point set, cell), work
// items of kNearBlock targets of one cell, one lane per target, the sources streamed through LDS in tiles of kNearTile as
// one float4 broadcast per pair, CC columns of sums in registers, no atomics -- with two differences:
//
// * cells per axis: G0 x G1 x G2 cells of fractional edge 1 / G_a, G_a <= w_a / r_c for the perpendicular width w_a of the
//   box along axis a, cell index c0 + G0 (c1 + G1 c2).  The rows wrap with G1 and G2, the ranges within a row use G0 (one
//   contiguous range for 0 < c0 < G0 - 1, two at either end).  Every G_a >= 3 makes the 27 cells distinct;
// * metric: ds is wrapped componentwise, then d = ds A (three products and three FMAs for the lower triangle).  Under
//   r_c <= w_a / 3 an image with |d| < r_c has |ds_a| <= |d| / w_a < 1/3 on every axis, so the componentwise wrap IS that
//   image, it is the only one, and it lies in one of the 27 cells: no lattice search at any tilt.
#include "nearfield.h"

namespace nfft {

namespace {

struct EwaldBoxParams {
    int G0, G1, G2;
    int64_t Cr;
    float alpha, neg_alpha2, rc2, slope;  // alpha, -alpha^2, r_c^2, 2 alpha / sqrt(pi)
    float a00, a10, a11, a20, a21, a22;   // the lower triangle of A
};

template <int CC, bool FIELD>
__global__ void __launch_bounds__(kNearBlock) ewald_near_box_kernel(EwaldBoxParams q, const int2 *__restrict__ items,
                                                                    const float *__restrict__ pos,
                                                                    const float *__restrict__ xr,
                                                                    const int *__restrict__ start,
                                                                    const int64_t *__restrict__ index, float *__restrict__ z,
                                                                    float *__restrict__ f)
{
    __shared__ float4 s_pos[kNearTile];
    __shared__ __attribute__((aligned(16))) float s_x[kNearTile * CC];
    const int2 item = items[blockIdx.x];
    if (item.x < 0) return;  // (uniform: an empty slot)
    const int tid = threadIdx.x;
    const int k = item.x;
    const int tend = min(item.y + kNearBlock, start[k + 1]);
    const int ti = item.y + tid;
    const bool active = ti < tend;
    const bool wave_active = item.y + (tid & ~63) < tend;
    const int G0 = q.G0, G1 = q.G1, G2 = q.G2;
    const int c0 = k % G0, c1 = (k / G0) % G1, c2 = (k / (G0 * G1)) % G2;
    const int set0 = k - (c2 * G1 + c1) * G0 - c0;  // first cell of the point set
    // (a lane without a target sums pairs of the origin and stores nothing)
    float tx = 0.f, ty = 0.f, tz = 0.f;
    if (active) {
        const float *tp = pos + (int64_t)ti * 3;
        tx = tp[0];
        ty = tp[1];
        tz = tp[2];
    }
    // the cells c0 - 1 .. c0 + 1 of a row as ranges of cells [lo, hi): one inside the row, two at its ends
    const bool split = c0 == 0 || c0 == G0 - 1;
    const int lo0 = c0 == 0 ? G0 - 1 : (c0 == G0 - 1 ? 0 : c0 - 1);
    const int hi0 = c0 == 0 ? G0 : (c0 == G0 - 1 ? 1 : c0 + 2);
    const int lo1 = c0 == 0 ? 0 : G0 - 2;
    const int hi1 = c0 == 0 ? 2 : G0;
    for (int64_t col0 = 0; col0 < q.Cr; col0 += CC) {
        float acc[CC];
        float fx[FIELD ? CC : 1], fy[FIELD ? CC : 1], fz[FIELD ? CC : 1];
#pragma unroll
        for (int c = 0; c < CC; ++c) acc[c] = 0.f;
#pragma unroll
        for (int c = 0; c < (FIELD ? CC : 1); ++c) fx[c] = fy[c] = fz[c] = 0.f;
        for (int d2 = -1; d2 <= 1; ++d2) {
            const int w2 = c2 + d2 < 0 ? G2 - 1 : (c2 + d2 >= G2 ? 0 : c2 + d2);
            for (int d1 = -1; d1 <= 1; ++d1) {
                const int w1 = c1 + d1 < 0 ? G1 - 1 : (c1 + d1 >= G1 ? 0 : c1 + d1);
                const int row = set0 + (w2 * G1 + w1) * G0;
                for (int part = 0; part < (split ? 2 : 1); ++part) {
                    const int first = start[row + (part ? lo1 : lo0)];
                    const int last = start[row + (part ? hi1 : hi0)];
                    for (int t0 = first; t0 < last; t0 += kNearTile) {
                        const int cnt = min(kNearTile, last - t0);
                        __syncthreads();
                        for (int j = tid; j < cnt; j += kNearBlock) {
                            const float *sp = pos + (int64_t)(t0 + j) * 3;
                            s_pos[j] = make_float4(sp[0], sp[1], sp[2], 0.f);
                            const float *xp = xr + (int64_t)(t0 + j) * q.Cr + col0;
#pragma unroll
                            for (int c = 0; c < CC; ++c) s_x[j * CC + c] = col0 + c < q.Cr ? xp[c] : 0.f;
                        }
                        __syncthreads();
                        if (!wave_active) continue;
#pragma unroll 2
                        for (int j = 0; j < cnt; ++j) {
                            const float4 s = s_pos[j];
                            float s0 = tx - s.x, s1 = ty - s.y, s2 = tz - s.z;
                            s0 -= rintf(s0);
                            s1 -= rintf(s1);
                            s2 -= rintf(s2);
                            // d = ds A, A lower triangular with rows = lattice vectors
                            const float dx = fmaf(s2, q.a20, fmaf(s1, q.a10, s0 * q.a00));
                            const float dy = fmaf(s2, q.a21, s1 * q.a11);
                            const float dz = s2 * q.a22;
                            const float rr = dx * dx + dy * dy + dz * dz;
                            // the lanes that fail the test sit the expansion out
                            if (!(rr > 0.f && rr < q.rc2)) continue;
                            const float ir = rsqrtf(rr);
                            const float w = erfcf(q.alpha * (rr * ir)) * ir;  // erfc(alpha r) / r
#pragma unroll
                            for (int c = 0; c < CC; ++c) acc[c] += w * s_x[j * CC + c];
                            if (FIELD) {
                                // -g = (erfc(alpha r) / r + (2 alpha / sqrt(pi)) e^(-alpha^2 r^2)) / r^2
                                const float mg = (w + q.slope * __expf(q.neg_alpha2 * rr)) * (ir * ir);
                                const float gx = mg * dx, gy = mg * dy, gz = mg * dz;
#pragma unroll
                                for (int c = 0; c < (FIELD ? CC : 1); ++c) {
                                    const float v = s_x[j * CC + c];
                                    fx[c] += gx * v;
                                    fy[c] += gy * v;
                                    fz[c] += gz * v;
                                }
                            }
                        }
                    }
                }
            }
        }
        if (active) {
            const int64_t row = index[ti];
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

template <bool FIELD>
void launch_box_pairs(const EwaldBoxParams &q, int64_t slots, const int2 *items, const float *pos, const float *xr,
                      const int *start, const int64_t *index, float *z, float *f, hipStream_t stream)
{
    const dim3 grid((unsigned)slots), block(kNearBlock);
#define EWALD_BOX_LAUNCH(CC) \
    hipLaunchKernelGGL((ewald_near_box_kernel<CC, FIELD>), grid, block, 0, stream, q, items, pos, xr, start, index, z, f)
    if (q.Cr == 1) EWALD_BOX_LAUNCH(1);
    else if (q.Cr == 2) EWALD_BOX_LAUNCH(2);
    else EWALD_BOX_LAUNCH(4);
#undef EWALD_BOX_LAUNCH
}

int64_t ewald_box_cells(const nfft_hip_ewald_box_problem *p)
{
    return p->batch_size * p->cells[0] * p->cells[1] * p->cells[2];
}

}  // namespace

int64_t ewald_near_box_item_slots(const nfft_hip_ewald_box_problem *p)
{
    return nearfield_item_slots(ewald_box_cells(p), p->num_points);
}

int launch_ewald_near_box(const nfft_hip_ewald_box_problem *p, const float *pos, const float *xr, const int *start,
                          const int64_t *index, float *z, float *f, void *items, hipStream_t stream)
{
    EwaldBoxParams q;
    q.G0 = p->cells[0];
    q.G1 = p->cells[1];
    q.G2 = p->cells[2];
    q.Cr = p->num_columns;
    q.alpha = (float)p->alpha;
    q.neg_alpha2 = (float)(-p->alpha * p->alpha);
    q.rc2 = (float)(p->r_cut * p->r_cut);
    q.slope = (float)(2.0 * p->alpha / 1.7724538509055160273);
    q.a00 = (float)p->box[0];
    q.a10 = (float)p->box[1];
    q.a11 = (float)p->box[2];
    q.a20 = (float)p->box[3];
    q.a21 = (float)p->box[4];
    q.a22 = (float)p->box[5];
    if (int rc = launch_nearfield_items(ewald_box_cells(p), p->num_points, start, (int2 *)items, stream)) return rc;
    const int64_t slots = ewald_near_box_item_slots(p);
    if (p->with_field) launch_box_pairs<true>(q, slots, (const int2 *)items, pos, xr, start, index, z, f, stream);
    else launch_box_pairs<false>(q, slots, (const int2 *)items, pos, xr, start, index, z, f, stream);
    NFFT_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace nfft
