// Gradient at the targets of the near field of the fast summation for singular kernels, and its
// transpose:
//
//     G_i[a]  = sum_{j in the point set of i, 0 < r_ij < eps_I} g(r_ij^2) (t_i - s_j)[a] x_j          (gradient)
//     (G^T v)_j = sum_{i in the point set of j, 0 < r_ij < eps_I} g(r_ij^2) (t_i - s_j) . v_i           (transpose)
//
// with g(r^2) = (K'(r) - T_I'(r)) / r, both quotients functions of r^2: K'(r) / r in closed form per kernel and
// T_I'(r) / r = (2 / eps_I^2) sum_{k >= 1} k a_k u^(k-1), u = r^2 / eps_I^2, a Horner form whose coefficients the host
// makes in float64.  No reference counterpart.
//
// The design is that of the frame in pair_frame.h: a work item is up to kNearBlock cell-sorted output
// points of one cell, a lane owns one output point, the streamed points of 3^(dim-1) contiguous rows of cells pass through
// LDS in tiles of kNearTile, every lane reads the same streamed point (an LDS broadcast) and sums in registers in the sorted
// order.  No atomics.  The device code is WRITTEN OUT here and does not use the frame's templates: ported, its pair loops
// were the same instructions (some v_fma_f32 encoded as v_fmac_f32) and yet two of its timed rows fell outside the margin
// of the comparison with the code as it stands here (profiles/r16_pair_frame.md), so it stays as it was.  A fix to the
// frame's lane decode, open walk or tile sweep has to be repeated in this file.  Only the launch uses pair_frame.h.
//   gradient    output = targets, streamed = sources: LDS holds the position and CC columns of x; 3 CC sums per lane,
//               dim CC of them stored to out[row, a, col]
//   transpose   output = sources, streamed = targets: LDS holds the position and 3 CC values of v (axes past dim are
//               zero); CC sums per lane.  The caller hands the two cell orders in swapped, so the difference vector
//               "output - streamed" is s_j - t_i and the weight changes its sign.
// A pair with r = 0 weighs exactly zero (its difference vector is zero; K'(r) / r is not finite there), like the pairs at
// or beyond eps_I: selected, not branched over.
#include "pair_frame.h"

namespace nfft {

namespace {

constexpr int kNearTranspose = 1;  // MODE: 0 the gradient, 1 its transpose

// PT: Horner terms, 4 or 8; the coefficients past `terms` are zero, which leaves the sum of the others bit for bit.
// in: [streamed points, Cr] (gradient) or [streamed points, dim, Cr] (transpose); out: [output points, dim, Cr] (gradient)
// or [output points, Cr] (transpose), row oindex[i] for the sorted output point i.
template <int KERNEL, int CC, int PT, int MODE>
__global__ void __launch_bounds__(kNearBlock) nearfield_grad_kernel(NearParams q, const int2 *__restrict__ items,
                                                                    const float *__restrict__ spos, const float *__restrict__ in,
                                                                    const int *__restrict__ sstart, const float *__restrict__ opos,
                                                                    const int64_t *__restrict__ oindex,
                                                                    const int *__restrict__ ostart, float *__restrict__ out)
{
    constexpr int SV = MODE == kNearTranspose ? 3 * CC : CC;  // staged values per streamed point
    constexpr int NA = MODE == kNearTranspose ? 1 : 3;        // sums per column
    constexpr int kUnroll = SV >= 12 ? 2 : 4;                 // pairs in flight: 16 + 4 SV bytes of LDS reads each
    __shared__ float4 s_pos[kNearTile];
    __shared__ __attribute__((aligned(16))) float s_x[kNearTile * SV];
    const int2 item = items[blockIdx.x];
    if (item.x < 0) return;  // (uniform: an empty slot)
    const int tid = threadIdx.x;
    const int k = item.x;
    const int tend = min(item.y + kNearBlock, ostart[k + 1]);
    const int ti = item.y + tid;
    const bool active = ti < tend;
    const bool wave_active = item.y + (tid & ~63) < tend;
    const int G = q.G;
    const int c0 = k % G;
    const int c1 = q.dim >= 2 ? (k / G) % G : 0;
    const int c2 = q.dim >= 3 ? (k / (G * G)) % G : 0;
    // a lane without an output point sits far away: every pair fails the distance test
    float tx = 1e9f, ty = 0.f, tz = 0.f;
    if (active) {
        const float *tp = opos + (int64_t)ti * q.dim;
        tx = tp[0];
        if (q.dim >= 2) ty = tp[1];
        if (q.dim >= 3) tz = tp[2];
    }
    const int r1 = q.dim >= 2 ? 1 : 0, r2 = q.dim >= 3 ? 1 : 0;
    const int nd = MODE == kNearTranspose ? q.dim : 1;  // staged rows of `in` per streamed point
    const int64_t in_stride = nd * q.Cr;
    float a[PT];
#pragma unroll
    for (int e = 0; e < PT; ++e) a[e] = q.poly[e];
    for (int64_t col0 = 0; col0 < q.Cr; col0 += CC) {
        float acc[NA][CC];
#pragma unroll
        for (int d = 0; d < NA; ++d)
#pragma unroll
            for (int c = 0; c < CC; ++c) acc[d][c] = 0.f;
        for (int d2 = -r2; d2 <= r2; ++d2) {
            if (c2 + d2 < 0 || c2 + d2 >= G) continue;
            for (int d1 = -r1; d1 <= r1; ++d1) {
                if (c1 + d1 < 0 || c1 + d1 >= G) continue;
                const int row = k + (d2 * G + d1) * G;
                const int first = sstart[row - (c0 > 0 ? 1 : 0)];
                const int last = sstart[row + (c0 < G - 1 ? 1 : 0) + 1];
                for (int t0 = first; t0 < last; t0 += kNearTile) {
                    const int cnt = min(kNearTile, last - t0);
                    __syncthreads();
                    for (int j = tid; j < cnt; j += kNearBlock) {
                        const float *sp = spos + (int64_t)(t0 + j) * q.dim;
                        float4 v = make_float4(sp[0], 0.f, 0.f, 0.f);
                        if (q.dim >= 2) v.y = sp[1];
                        if (q.dim >= 3) v.z = sp[2];
                        s_pos[j] = v;
                    }
                    // the staged values, one per lane and step: element e = d CC + c of the streamed point j
                    for (int idx = tid; idx < cnt * SV; idx += kNearBlock) {
                        const int j = idx / SV, e = idx - j * SV;
                        const int d = e / CC, c = e - d * CC;
                        const bool there = d < nd && col0 + c < q.Cr;
                        s_x[idx] = there ? in[(int64_t)(t0 + j) * in_stride + d * q.Cr + col0 + c] : 0.f;
                    }
                    __syncthreads();
                    if (!wave_active) continue;
#pragma unroll kUnroll
                    for (int j = 0; j < cnt; ++j) {
                        const float4 s = s_pos[j];
                        const float dx = tx - s.x, dy = ty - s.y, dz = tz - s.z;
                        const float rr = dx * dx + dy * dy + dz * dz;
                        const float u = rr * q.inv_eps2;
                        float t = a[PT - 1];
#pragma unroll
                        for (int e = PT - 2; e >= 0; --e) t = t * u + a[e];
                        const float g = kernel_slope<KERNEL>(rr, q);
                        if constexpr (MODE == kNearTranspose) {
                            // t_i - s_j is streamed - output: the weight of -d
                            const float w = rr < q.eps2 && rr > 0.f ? t - g : 0.f;
#pragma unroll
                            for (int c = 0; c < CC; ++c)
                                acc[0][c] += w * (dx * s_x[j * SV + c] + dy * s_x[j * SV + CC + c] + dz * s_x[j * SV + 2 * CC + c]);
                        } else {
                            const float w = rr < q.eps2 && rr > 0.f ? g - t : 0.f;
                            const float wx = w * dx, wy = w * dy, wz = w * dz;
#pragma unroll
                            for (int c = 0; c < CC; ++c) {
                                const float xv = s_x[j * SV + c];
                                acc[0][c] += wx * xv;
                                acc[1][c] += wy * xv;
                                acc[2][c] += wz * xv;
                            }
                        }
                    }
                }
            }
        }
        if (active) {
            if constexpr (MODE == kNearTranspose) {
                float *zp = out + oindex[ti] * q.Cr + col0;
#pragma unroll
                for (int c = 0; c < CC; ++c)
                    if (col0 + c < q.Cr) zp[c] = acc[0][c];
            } else {
                float *zp = out + oindex[ti] * (q.dim * q.Cr) + col0;
#pragma unroll
                for (int d = 0; d < NA; ++d)
#pragma unroll
                    for (int c = 0; c < CC; ++c)
                        if (d < q.dim && col0 + c < q.Cr) zp[d * q.Cr + c] = acc[d][c];
            }
        }
    }
}

}  // namespace

int launch_nearfield_gradient(const nfft_hip_nearfield_problem *p, int transpose, const double *gradient_poly,
                              const float *spos, const float *in, const int *sstart, const float *opos, const int64_t *oindex,
                              const int *ostart, float *out, void *items, hipStream_t stream)
{
    const NearParams q = near_params(p, gradient_poly, p->poly_terms - 1);
    const int64_t slots = nearfield_item_slots(p);
    if (int rc = launch_nearfield_items(p, ostart, (int2 *)items, stream)) return rc;
    const dim3 grid((unsigned)slots), block(kNearBlock);
    dispatch_flag(transpose != 0, [&](auto MODE) {
        dispatch_kernel(p->kernel, [&](auto K) {
            dispatch_columns(q.Cr, [&](auto CC) {
                dispatch_terms(q.terms, [&](auto PT) {
                    hipLaunchKernelGGL((nearfield_grad_kernel<K(), CC(), PT(), MODE()>), grid, block, 0, stream, q,
                                       (const int2 *)items, spos, in, sstart, opos, oindex, ostart, out);
                });
            });
        });
    });
    NFFT_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace nfft
