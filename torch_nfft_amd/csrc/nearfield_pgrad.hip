// Gradient with respect to the points of the near field of the fast summation for singular kernels.
// For z_i = sum_j (K - T_I)(r_ij) x_j and a loss with dy = dL/dz, the contraction over the columns happens inside the pair
// loop:
//
//     out[oindex[i], a] = sum_{j in the point set of i} w_ij (o_i - p_j)[a] ( sum_c u[i, c] v[j, c]
//                                                                            [ + sum_c v[i, c] u[j, c]   if SYM ] )
//     w_ij = g(r_ij^2) if 0 < r_ij^2 < eps_I^2, else exactly 0;   g(r^2) = (K'(r) - T_I'(r)) / r  as in nearfield_grad.hip
//
//   SYM = 0   u: the output side's values (CC per column pass, in registers), v: the streamed side's (in LDS next to the
//             position).  The targets' gradient has output = targets, u = dy, v = x; the sources' gradient has the two cell
//             orders in swapped places, u = x, v = dy.  The difference vector is "output - streamed" in both: no sign flip.
//   SYM = 1   both sides are ONE point set in one cell order; u and v are staged on both sides and the one sweep returns the
//             sum of the two gradients of point i.
// No reference counterpart.
//
// The kernel stands on the frame of pair_frame.h -- the lane decode, the open walk, the positions,
// the Horner form, sums in registers in the sorted order, no atomics -- except for the tile sweep, which is WRITTEN OUT
// here with its flat staging of SV values per streamed point: through sweep_range the compiler orders the LDS reads of the
// symmetric CC = 4 loop differently and that loop measured 2 % slower (profiles/r16_pair_frame.md).  A change to
// sweep_range has to be repeated in this file.  Its own: three sums per lane whatever the number of columns: they are
// zeroed once, and every pass of CC columns reloads
// u and v and keeps adding, so a point's result stays one sum in one fixed order.
#include "pair_frame.h"

namespace nfft {

namespace {

// PT: Horner terms, 4 or 8; the coefficients past `terms` are zero, which leaves the sum of the others bit for bit.
// sval [streamed points, Cr] and oval [output points, Cr] in cell order; out [output points, 3 or less = dim], row
// oindex[i] for the sorted output point i.  SYM: sval and oval are v and u of the one point set.
template <int KERNEL, int CC, int PT, int SYM>
__global__ void __launch_bounds__(kNearBlock) nearfield_pgrad_kernel(NearParams q, const int2 *__restrict__ items,
                                                                     const float *__restrict__ spos, const float *__restrict__ sval,
                                                                     const int *__restrict__ sstart, const float *__restrict__ opos,
                                                                     const float *__restrict__ oval,
                                                                     const int64_t *__restrict__ oindex,
                                                                     const int *__restrict__ ostart, float *__restrict__ out)
{
    constexpr int SV = SYM ? 2 * CC : CC;      // staged values per streamed point: v (and u behind it)
    constexpr int kUnroll = SV >= 8 ? 2 : 4;   // pairs in flight: 16 + 4 SV bytes of LDS reads each
    __shared__ float4 s_pos[kNearTile];
    __shared__ __attribute__((aligned(16))) float s_v[kNearTile * SV];
    const int2 item = items[blockIdx.x];
    if (item.x < 0) return;  // (uniform: an empty slot)
    const PairLane lane = pair_lane(item, ostart);
    const int tid = threadIdx.x;
    const OpenWalk walk(lane.cell, q.dim, q.G);
    // a lane without an output point sits far away: every pair fails the distance test
    const float4 t = lane_position(lane, opos, q.dim, 1e9f);
    float a[PT];
#pragma unroll
    for (int e = 0; e < PT; ++e) a[e] = q.poly[e];
    float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f;
    for (int64_t col0 = 0; col0 < q.Cr; col0 += CC) {
        // the lane's own values of this pass: u, and for SYM v behind it
        float own[SV];
#pragma unroll
        for (int e = 0; e < SV; ++e) {
            const int c = e < CC ? e : e - CC;
            const float *src = e < CC ? oval : sval;
            own[e] = lane.active && col0 + c < q.Cr ? src[(int64_t)lane.ti * q.Cr + col0 + c] : 0.f;
        }
        walk(sstart, [&](int first, int last) {
            for (int t0 = first; t0 < last; t0 += kNearTile) {
                const int cnt = min(kNearTile, last - t0);
                __syncthreads();
                for (int j = tid; j < cnt; j += kNearBlock) s_pos[j] = load_position(spos, t0 + j, q.dim);
                // the staged values, one per lane and step: element e of the streamed point j is v[e] for e < CC and
                // (SYM) u[e - CC] behind it
                for (int idx = tid; idx < cnt * SV; idx += kNearBlock) {
                    const int j = idx / SV, e = idx - j * SV;
                    const bool second = SYM != 0 && e >= CC;
                    const int c = second ? e - CC : e;
                    const float *src = second ? oval : sval;
                    s_v[idx] = col0 + c < q.Cr ? src[(int64_t)(t0 + j) * q.Cr + col0 + c] : 0.f;
                }
                __syncthreads();
                if (!lane.wave_active) continue;
#pragma unroll kUnroll
                for (int j = 0; j < cnt; ++j) {
                    const float4 s = s_pos[j];
                    const float dx = t.x - s.x, dy = t.y - s.y, dz = t.z - s.z;
                    const float rr = dx * dx + dy * dy + dz * dz;
                    const float ti = horner(a, rr * q.inv_eps2);
                    const float g = kernel_slope<KERNEL>(rr, q);
                    const float w = rr < q.eps2 && rr > 0.f ? g - ti : 0.f;
                    // u_i . v_j (+ v_i . u_j): the lane's u meets the staged v, its v the staged u
                    float dot = 0.f;
#pragma unroll
                    for (int c = 0; c < CC; ++c) dot += own[c] * s_v[j * SV + c];
                    if constexpr (SYM != 0) {
#pragma unroll
                        for (int c = 0; c < CC; ++c) dot += own[CC + c] * s_v[j * SV + CC + c];
                    }
                    const float wd = w * dot;
                    acc0 += wd * dx;
                    acc1 += wd * dy;
                    acc2 += wd * dz;
                }
            }
        });
    }
    if (lane.active) {
        float *zp = out + oindex[lane.ti] * q.dim;
        zp[0] = acc0;
        if (q.dim >= 2) zp[1] = acc1;
        if (q.dim >= 3) zp[2] = acc2;
    }
}

}  // namespace

int launch_nearfield_point_gradient(const nfft_hip_nearfield_problem *p, int symmetric, const double *gradient_poly,
                                    const float *spos, const float *sval, const int *sstart, const float *opos,
                                    const float *oval, const int64_t *oindex, const int *ostart, float *out, void *items,
                                    hipStream_t stream)
{
    const NearParams q = near_params(p, gradient_poly, p->poly_terms - 1);
    const int64_t slots = nearfield_item_slots(p);
    if (int rc = launch_nearfield_items(p, ostart, (int2 *)items, stream)) return rc;
    const dim3 grid((unsigned)slots), block(kNearBlock);
    dispatch_flag(symmetric != 0, [&](auto SYM) {
        dispatch_kernel(p->kernel, [&](auto K) {
            dispatch_columns(q.Cr, [&](auto CC) {
                dispatch_terms(q.terms, [&](auto PT) {
                    hipLaunchKernelGGL((nearfield_pgrad_kernel<K(), CC(), PT(), SYM()>), grid, block, 0, stream, q,
                                       (const int2 *)items, spos, sval, sstart, opos, oval, oindex, ostart, out);
                });
            });
        });
    });
    NFFT_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace nfft
