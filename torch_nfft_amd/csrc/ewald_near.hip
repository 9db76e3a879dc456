// Near part of the Ewald sum for the periodic 1/r on the unit torus: for one point set on both
// sides, x in [-1/2, 1/2)^3,
//
//     z[i, c]    =  sum_{j: 0 < r_ij < r_c} erfc(alpha r_ij) / r_ij  xr[j, c]
//     f[i, a, c] = -sum_{j: 0 < r_ij < r_c} g(r_ij^2) d_ij[a] xr[j, c],     g = K'(r) / r for K = erfc(alpha r) / r,
//
// d_ij the minimum image of x_i - x_j and r_ij its length.  The frame is that of nearfield.hip -- points ordered by (point
// set, cell), work items of kNearBlock targets of one cell, one lane per target, the sources streamed through LDS in tiles
// of kNearTile as one float4 broadcast per pair, CC columns of sums in registers, no atomics -- with two differences:
//
// * the G^3 cells of edge 1/G >= r_c cover the WHOLE torus and the walk over the 27 neighbours wraps: the rows
//   (c1 + d1) mod G, (c2 + d2) mod G, and within a row the cells c0 - 1 .. c0 + 1, which are one contiguous range of
//   sources for 0 < c0 < G - 1 and two at either end of the row (the wrapped cell, then the two others).  G >= 3 makes the
//   27 cells distinct, so no pair is met twice;
// * the difference vector is reduced to its minimum image, d -= rintf(d), before the distance test.
//
// The loop is bound by the VALU: the expansion of erfcf (see DESIGN.md 7g for the measurement).
#include "nearfield.h"

namespace nfft {

namespace {

struct EwaldParams {
    int G;
    int64_t Cr;
    float alpha, neg_alpha2, rc2, slope;  // alpha, -alpha^2, r_c^2, 2 alpha / sqrt(pi)
};

template <int CC, bool FIELD>
__global__ void __launch_bounds__(kNearBlock) ewald_near_kernel(EwaldParams q, const int2 *__restrict__ items,
                                                                const float *__restrict__ pos, const float *__restrict__ xr,
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
    const int G = q.G;
    const int c0 = k % G, c1 = (k / G) % G, c2 = (k / (G * G)) % G;
    const int set0 = k - (c2 * G + c1) * G - c0;  // first cell of the point set
    // (a lane without a target sums pairs of the origin and stores nothing)
    float tx = 0.f, ty = 0.f, tz = 0.f;
    if (active) {
        const float *tp = pos + (int64_t)ti * 3;
        tx = tp[0];
        ty = tp[1];
        tz = tp[2];
    }
    // the cells c0 - 1 .. c0 + 1 of a row as ranges of cells [lo, hi): one inside the row, two at its ends
    const bool split = c0 == 0 || c0 == G - 1;
    const int lo0 = c0 == 0 ? G - 1 : (c0 == G - 1 ? 0 : c0 - 1);
    const int hi0 = c0 == 0 ? G : (c0 == G - 1 ? 1 : c0 + 2);
    const int lo1 = c0 == 0 ? 0 : G - 2;
    const int hi1 = c0 == 0 ? 2 : G;
    for (int64_t col0 = 0; col0 < q.Cr; col0 += CC) {
        float acc[CC];
        float fx[FIELD ? CC : 1], fy[FIELD ? CC : 1], fz[FIELD ? CC : 1];
#pragma unroll
        for (int c = 0; c < CC; ++c) acc[c] = 0.f;
#pragma unroll
        for (int c = 0; c < (FIELD ? CC : 1); ++c) fx[c] = fy[c] = fz[c] = 0.f;
        for (int d2 = -1; d2 <= 1; ++d2) {
            const int w2 = c2 + d2 < 0 ? G - 1 : (c2 + d2 >= G ? 0 : c2 + d2);
            for (int d1 = -1; d1 <= 1; ++d1) {
                const int w1 = c1 + d1 < 0 ? G - 1 : (c1 + d1 >= G ? 0 : c1 + d1);
                const int row = set0 + (w2 * G + w1) * G;
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
                            float dx = tx - s.x, dy = ty - s.y, dz = tz - s.z;
                            dx -= rintf(dx);
                            dy -= rintf(dy);
                            dz -= rintf(dz);
                            const float rr = dx * dx + dy * dy + dz * dz;
                            // about one pair in six of the 27 cells passes: the lanes that fail sit the expansion out
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
void launch_pairs(const EwaldParams &q, int64_t slots, const int2 *items, const float *pos, const float *xr, const int *start,
                  const int64_t *index, float *z, float *f, hipStream_t stream)
{
    const dim3 grid((unsigned)slots), block(kNearBlock);
#define EWALD_LAUNCH(CC) \
    hipLaunchKernelGGL((ewald_near_kernel<CC, FIELD>), grid, block, 0, stream, q, items, pos, xr, start, index, z, f)
    if (q.Cr == 1) EWALD_LAUNCH(1);
    else if (q.Cr == 2) EWALD_LAUNCH(2);
    else EWALD_LAUNCH(4);
#undef EWALD_LAUNCH
}

int64_t ewald_cells(const nfft_hip_ewald_problem *p)
{
    return p->batch_size * p->cells_per_axis * p->cells_per_axis * p->cells_per_axis;
}

}  // namespace

int64_t ewald_near_item_slots(const nfft_hip_ewald_problem *p) { return nearfield_item_slots(ewald_cells(p), p->num_points); }

int launch_ewald_near(const nfft_hip_ewald_problem *p, const float *pos, const float *xr, const int *start,
                      const int64_t *index, float *z, float *f, void *items, hipStream_t stream)
{
    EwaldParams q;
    q.G = p->cells_per_axis;
    q.Cr = p->num_columns;
    q.alpha = (float)p->alpha;
    q.neg_alpha2 = (float)(-p->alpha * p->alpha);
    q.rc2 = (float)(p->r_cut * p->r_cut);
    q.slope = (float)(2.0 * p->alpha / 1.7724538509055160273);
    if (int rc = launch_nearfield_items(ewald_cells(p), p->num_points, start, (int2 *)items, stream)) return rc;
    const int64_t slots = ewald_near_item_slots(p);
    if (p->with_field) launch_pairs<true>(q, slots, (const int2 *)items, pos, xr, start, index, z, f, stream);
    else launch_pairs<false>(q, slots, (const int2 *)items, pos, xr, start, index, z, f, stream);
    NFFT_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace nfft
