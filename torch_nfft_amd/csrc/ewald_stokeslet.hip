// Periodic Stokeslet sum (Hasimoto's Ewald sum): the pair sweep and the spectral step.
//
// Source j carries a Cartesian force f_j.  With d = d_ij the minimum image of x_i - x_j, r = |d|, m = d . f_j, the Smith
// functions B_0, B_1, B_2 and g = (2 alpha / sqrt(pi)) e^(-alpha^2 r^2) (StokesletPairWeight, pair_frame.h), over the pairs
// 0 < r < r_c of one point set:
//
//     u[i, a]    = sum_j  (B_0 - g) f_j,a + B_1 m d_a
//     G[i, a, b] = sum_j  (2 alpha^2 g - B_1) f_j,a d_b + B_1 (d_a f_j,b + m delta_ab) - B_2 m d_a d_b       (G_ab = d u_a / d x_b)
//
// ORDER = 1 gives the three sums of u per column, ORDER = 2 adds the nine of G, row-major in ab (G is not symmetric):
// out [n, 3 or 12, Cr] in the caller's point order.
//
// The pair kernel is the twin of ewald_dipole_near_kernel (ewald_dipole.hip, section 7l): the same frame of pair_frame.h,
// the same wrapped walk, image and distance branch, no atomics.  Its own: the pair weights, the staging policy StageForces
// -- the three values of a staged point and column are one float4 of LDS (f, 0), read as one 16-byte broadcast per pair and
// column -- and 3 or 12 sums per column.
//
// The spectral step turns the adjoint transform of the forces, band [B, N, N, N, 3, C], into the 3 or 12 spectra whose
// forward transform is the far part of (u, G): the projection onto the plane across the wave vector, one read and one
// write of every frequency.
#include "spectral_frame.h"

namespace nfft {

namespace {

// staging policy: (f_x, f_y, f_z, 0) of CC columns from col0 on of xs [points, 3, Cr] per staged point, zero past Cr
template <int CC>
struct StageForces {
    float4 *s_x;
    const float *__restrict__ xs;
    int64_t Cr, col0;
    __device__ __forceinline__ void point(int j, int64_t i) const
    {
        const float *xp = xs + i * 3 * Cr + col0;
#pragma unroll
        for (int c = 0; c < CC; ++c)
            s_x[j * CC + c] = col0 + c < Cr ? make_float4(xp[c], xp[Cr + c], xp[2 * Cr + c], 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
};

template <int CC, int ORDER, bool BOX>
__global__ void __launch_bounds__(kNearBlock) ewald_stokeslet_near_kernel(EwaldPairParams q, const int2 *__restrict__ items,
                                                                          const float *__restrict__ pos,
                                                                          const float *__restrict__ xs,
                                                                          const int *__restrict__ start,
                                                                          const int64_t *__restrict__ index,
                                                                          float *__restrict__ out)
{
    constexpr int SUMS = ORDER == 2 ? 12 : 3;
    __shared__ float4 s_pos[kNearTile];
    __shared__ float4 s_x[kNearTile * CC];
    const int2 item = items[blockIdx.x];
    if (item.x < 0) return;  // (uniform: an empty slot)
    const PairLane lane = pair_lane(item, start);
    const WrappedWalk walk(lane.cell, q.G0, BOX ? q.G1 : q.G0, BOX ? q.G2 : q.G0);  // (cubic: one count, one division)
    // (a lane without a target sums pairs of the origin and stores nothing)
    const float4 t = lane_position(lane, pos, 3, 0.f);
    for (int64_t col0 = 0; col0 < q.Cr; col0 += CC) {
        float acc[SUMS][CC];
#pragma unroll
        for (int s = 0; s < SUMS; ++s)
#pragma unroll
            for (int c = 0; c < CC; ++c) acc[s][c] = 0.f;
        const StageForces<CC> stage = {s_x, xs, q.Cr, col0};
        walk(start, [&](int first, int last) {
            sweep_range<2>(first, last, lane, s_pos, pos, 3, stage, [&](int j) {
                const PairSep d = ewald_image<BOX>(t, s_pos[j], q);
                if (!(d.rr > 0.f && d.rr < q.rc2)) return;
                const StokesletPairWeight<ORDER> w(d.rr, q);
                const float dd[3] = {d.dx, d.dy, d.dz};
                const float p[3] = {w.c * d.dx, w.c * d.dy, w.c * d.dz};  // (2 alpha^2 g - B_1) d: the same for every column
#pragma unroll
                for (int c = 0; c < CC; ++c) {
                    const float4 v = s_x[j * CC + c];  // (f, 0)
                    const float f[3] = {v.x, v.y, v.z};
                    const float m = fmaf(v.z, d.dz, fmaf(v.y, d.dy, v.x * d.dx));
                    const float mB1 = m * w.B1;
#pragma unroll
                    for (int a = 0; a < 3; ++a) acc[a][c] += fmaf(mB1, dd[a], w.a * f[a]);
                    if constexpr (ORDER == 2) {
                        // G_ab = f_a p_b + d_a e_b + B_1 m delta_ab,   e = B_1 f - B_2 m d
                        const float mB2 = m * w.B2;
                        float e[3];
#pragma unroll
                        for (int b = 0; b < 3; ++b) e[b] = fmaf(w.B1, f[b], -(mB2 * dd[b]));
#pragma unroll
                        for (int a = 0; a < 3; ++a)
#pragma unroll
                            for (int b = 0; b < 3; ++b) {
                                const float g = fmaf(dd[a], e[b], f[a] * p[b]);
                                acc[3 + 3 * a + b][c] += a == b ? g + mB1 : g;
                            }
                    }
                }
            });
        });
        if (lane.active) {
            float *op = out + index[lane.ti] * SUMS * q.Cr + col0;
#pragma unroll
            for (int c = 0; c < CC; ++c)
                if (col0 + c < q.Cr) {
#pragma unroll
                    for (int s = 0; s < SUMS; ++s) op[s * q.Cr + c] = acc[s][c];
                }
        }
    }
}

// the items of `cells` cells over `num_points` points into `slots` slots, then the pair kernel
template <bool BOX>
int launch_pairs(const EwaldPairParams &q, int64_t cells, int64_t slots, int64_t num_points, int order, const float *pos,
                 const float *xs, const int *start, const int64_t *index, float *out, void *items, hipStream_t stream)
{
    if (int rc = launch_nearfield_items(cells, num_points, start, (int2 *)items, stream)) return rc;
    const dim3 grid((unsigned)slots), block(kNearBlock);
    dispatch_flag(order == 2, [&](auto SECOND) {
        dispatch_columns(q.Cr, [&](auto CC) {
            hipLaunchKernelGGL((ewald_stokeslet_near_kernel<CC(), 1 + SECOND(), BOX>), grid, block, 0, stream, q,
                               (const int2 *)items, pos, xs, start, index, out);
        });
    });
    NFFT_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- the spectral step ------------------------------------------------------------------------------------------------

// One thread per (frequency, column) of the point set blockIdx.y (spectral_element of spectral_frame.h).  With
// tau = 2 pi kappa and rho the three rows of band,
//     U = c_k (rho - tau (tau . rho) / |tau|^2)          (the quotient is 0 where |tau|^2 = 0)
//     out[a] = U_a,   out[3 + 3 a + b] = -i tau_b U_a
// in the transforms' sign convention: the adjoint sums e^(+2 pi i k.s) and the forward e^(-2 pi i k.s), whose derivative
// along x_b is the factor -i tau_b (EwaldSplitting.field_coeffs carries the same flip for E = -grad phi).
template <int ORDER>
__global__ void __launch_bounds__(kSpectralBlock) ewald_stokeslet_spectral_kernel(SpectralElementParams q,
                                                                                   const float2 *__restrict__ band,
                                                                                   const float *__restrict__ coeffs,
                                                                                   float2 *__restrict__ out)
{
    constexpr int SUMS = ORDER == 2 ? 12 : 3;
    SpectralElement el;
    if (!spectral_element(q, el)) return;
    const unsigned C = q.C, c = el.c;
    const float ck = coeffs[el.k];
    const float tau[3] = {el.tau.x, el.tau.y, el.tau.z};
    const float t2 = fmaf(tau[2], tau[2], fmaf(tau[1], tau[1], tau[0] * tau[0]));
    const float it2 = t2 > 0.f ? 1.f / t2 : 0.f;
    const float2 *bp = band + el.cell * 3 * C + c;
    const float2 v[3] = {bp[0], bp[C], bp[2 * C]};
    const float pre = fmaf(tau[2], v[2].x, fmaf(tau[1], v[1].x, tau[0] * v[0].x)) * it2;
    const float pim = fmaf(tau[2], v[2].y, fmaf(tau[1], v[1].y, tau[0] * v[0].y)) * it2;
    float2 *op = out + el.cell * SUMS * C + c;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float2 U = make_float2(ck * fmaf(-tau[a], pre, v[a].x), ck * fmaf(-tau[a], pim, v[a].y));
        op[a * C] = U;
        if constexpr (ORDER == 2) {
#pragma unroll
            for (int b = 0; b < 3; ++b) op[(3 + 3 * a + b) * C] = make_float2(tau[b] * U.y, -(tau[b] * U.x));
        }
    }
}

}  // namespace

// (the cell counts and the item slots are those of ewald_near.hip: one workspace serves every sweep)
int launch_ewald_stokeslet_near(const nfft_hip_ewald_problem *p, int order, const float *pos, const float *xs, const int *start,
                                const int64_t *index, float *out, void *items, hipStream_t stream)
{
    const int G = p->cells_per_axis;
    const EwaldPairParams q = ewald_pair_params(G, G, G, p->num_columns, p->alpha, p->r_cut, nullptr);
    return launch_pairs<false>(q, p->batch_size * G * G * G, ewald_near_item_slots(p), p->num_points, order, pos, xs, start,
                               index, out, items, stream);
}

int launch_ewald_stokeslet_near_box(const nfft_hip_ewald_box_problem *p, int order, const float *pos, const float *xs,
                                    const int *start, const int64_t *index, float *out, void *items, hipStream_t stream)
{
    const EwaldPairParams q = ewald_pair_params(p->cells[0], p->cells[1], p->cells[2], p->num_columns, p->alpha, p->r_cut, p->box);
    return launch_pairs<true>(q, p->batch_size * p->cells[0] * p->cells[1] * p->cells[2], ewald_near_box_item_slots(p),
                              p->num_points, order, pos, xs, start, index, out, items, stream);
}

int launch_ewald_stokeslet_spectral(int64_t N, int64_t batch_size, int64_t num_columns, int order, const void *band,
                                    const float *coeffs, const double *box_inverse, void *out, hipStream_t stream)
{
    return launch_spectral_elements(order == 2 ? ewald_stokeslet_spectral_kernel<2> : ewald_stokeslet_spectral_kernel<1>, N,
                                    batch_size, num_columns, band, coeffs, box_inverse, out, stream);
}

}  // namespace nfft
