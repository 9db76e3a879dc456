// Ewald sum for point charges and point dipoles: the pair sweep and the spectral step.
//
// Source j carries (q_j, mu_j), mu Cartesian.  With d = d_ij the minimum image of x_i - x_j, r = |d|, m = mu_j . d and the
// Smith functions B_l(r) (DipolePairWeight, pair_frame.h), over the pairs 0 < r < r_c of one point set:
//
//     phi[i]     = sum_j  q_j B_0 + m B_1
//     E[i, a]    = sum_j  s_1 d_a - mu_j,a B_1                                    s_1 = q_j B_1 + m B_2
//     T[i, a, b] = sum_j  s_1 delta_ab - s_2 d_a d_b + (mu_j,a d_b + mu_j,b d_a) B_2   s_2 = q_j B_2 + m B_3
//
// E = -grad phi and T_ab = d E_a / d x_b.  ORDER = 1 gives the four sums (phi, Ex, Ey, Ez) per column, ORDER = 2 adds the six
// of T in the order xx, yy, zz, yz, xz, xy: out [n, 4 or 10, Cr] in the caller's point order.
//
// The pair kernel is the twin of ewald_near_kernel (ewald_near.hip, sections 7g and 7h), which says what BOX = false (the
// unit torus) and BOX = true (fractional positions in a lower-triangular box) mean: the same frame of pair_frame.h, the same
// wrapped walk, image and distance branch, no atomics.  Its own: the pair weights, the staging policy StageDipoles -- the
// four values (q, mu) of a staged point and column are one float4 of LDS, read as one 16-byte broadcast per pair and
// column -- and 4 or 10 sums per column.
//
// The spectral step turns the adjoint transform of the packed sources, band [B, N, N, N, 4, C], into the 4 or 10 spectra
// whose forward transform is the far part of (phi, E, T): one read and one write of every frequency.
#include "spectral_frame.h"

namespace nfft {

namespace {

// staging policy: (q, mu_x, mu_y, mu_z) of CC columns from col0 on of xs [points, 4, Cr] per staged point, zero past Cr
template <int CC>
struct StageDipoles {
    float4 *s_x;
    const float *__restrict__ xs;
    int64_t Cr, col0;
    __device__ __forceinline__ void point(int j, int64_t i) const
    {
        const float *xp = xs + i * 4 * Cr + col0;
#pragma unroll
        for (int c = 0; c < CC; ++c)
            s_x[j * CC + c] = col0 + c < Cr ? make_float4(xp[c], xp[Cr + c], xp[2 * Cr + c], xp[3 * Cr + c])
                                            : make_float4(0.f, 0.f, 0.f, 0.f);
    }
};

template <int CC, int ORDER, bool BOX>
__global__ void __launch_bounds__(kNearBlock) ewald_dipole_near_kernel(EwaldPairParams q, const int2 *__restrict__ items,
                                                                       const float *__restrict__ pos, const float *__restrict__ xs,
                                                                       const int *__restrict__ start,
                                                                       const int64_t *__restrict__ index, float *__restrict__ out)
{
    constexpr int SUMS = ORDER == 2 ? 10 : 4;
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
        const StageDipoles<CC> stage = {s_x, xs, q.Cr, col0};
        walk(start, [&](int first, int last) {
            sweep_range<2>(first, last, lane, s_pos, pos, 3, stage, [&](int j) {
                const PairSep d = ewald_image<BOX>(t, s_pos[j], q);
                if (!(d.rr > 0.f && d.rr < q.rc2)) return;
                const DipolePairWeight<ORDER + 1> w(d.rr, q);
                const float B0 = w.B[0], B1 = w.B[1], B2 = w.B[2];
#pragma unroll
                for (int c = 0; c < CC; ++c) {
                    const float4 v = s_x[j * CC + c];  // (q, mu)
                    const float m = fmaf(v.w, d.dz, fmaf(v.z, d.dy, v.y * d.dx));
                    const float s1 = fmaf(m, B2, v.x * B1);
                    acc[0][c] += fmaf(m, B1, v.x * B0);
                    acc[1][c] += fmaf(s1, d.dx, -(v.y * B1));
                    acc[2][c] += fmaf(s1, d.dy, -(v.z * B1));
                    acc[3][c] += fmaf(s1, d.dz, -(v.w * B1));
                    if constexpr (ORDER == 2) {
                        const float s2 = fmaf(m, w.B[3], v.x * B2);
                        const float ux = v.y * B2, uy = v.z * B2, uz = v.w * B2;     // mu B_2
                        const float px = s2 * d.dx, py = s2 * d.dy, pz = s2 * d.dz;  // s_2 d
                        acc[4][c] += s1 + (2.f * ux - px) * d.dx;
                        acc[5][c] += s1 + (2.f * uy - py) * d.dy;
                        acc[6][c] += s1 + (2.f * uz - pz) * d.dz;
                        acc[7][c] += fmaf(uy - py, d.dz, uz * d.dy);  // yz
                        acc[8][c] += fmaf(ux - px, d.dz, uz * d.dx);  // xz
                        acc[9][c] += fmaf(ux - px, d.dy, uy * d.dx);  // xy
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
            hipLaunchKernelGGL((ewald_dipole_near_kernel<CC(), 1 + SECOND(), BOX>), grid, block, 0, stream, q, (const int2 *)items,
                               pos, xs, start, index, out);
        });
    });
    NFFT_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- the spectral step ------------------------------------------------------------------------------------------------

// One thread per (frequency, column) of the point set blockIdx.y (spectral_element of spectral_frame.h): rho = band_q +
// 2 pi i kappa . band_mu (the transforms' sign convention: the adjoint sums e^(+2 pi i k.s), EwaldSplitting.field_coeffs),
// R = b_k rho, and with tau = 2 pi kappa
//     out[0] = R,   out[1 + a] = i tau_a R,   out[4 + e] = tau_a tau_b R  (e: xx, yy, zz, yz, xz, xy).
template <int ORDER>
__global__ void __launch_bounds__(kSpectralBlock) ewald_dipole_spectral_kernel(SpectralElementParams q, const float2 *__restrict__ band,
                                                                                const float *__restrict__ coeffs,
                                                                                float2 *__restrict__ out)
{
    constexpr int SUMS = ORDER == 2 ? 10 : 4;
    SpectralElement el;
    if (!spectral_element(q, el)) return;
    const unsigned C = q.C, c = el.c;
    const float bk = coeffs[el.k];
    const float tx = el.tau.x, ty = el.tau.y, tz = el.tau.z;
    const float2 *bp = band + el.cell * 4 * C + c;
    const float2 vq = bp[0], vx = bp[C], vy = bp[2 * C], vz = bp[3 * C];
    const float mre = fmaf(tz, vz.x, fmaf(ty, vy.x, tx * vx.x)), mim = fmaf(tz, vz.y, fmaf(ty, vy.y, tx * vx.y));
    const float2 R = make_float2(bk * (vq.x - mim), bk * (vq.y + mre));
    float2 *op = out + el.cell * SUMS * C + c;
    op[0] = R;
    op[C] = times_i(tx, R);
    op[2 * C] = times_i(ty, R);
    op[3 * C] = times_i(tz, R);
    if constexpr (ORDER == 2) {
        const float w[6] = {tx * tx, ty * ty, tz * tz, ty * tz, tx * tz, tx * ty};
#pragma unroll
        for (int s = 0; s < 6; ++s) op[(4 + s) * C] = make_float2(w[s] * R.x, w[s] * R.y);
    }
}

}  // namespace

// (the cell counts and the item slots are those of ewald_near.hip: one workspace serves every sweep)
int launch_ewald_dipole_near(const nfft_hip_ewald_problem *p, int order, const float *pos, const float *xs, const int *start,
                             const int64_t *index, float *out, void *items, hipStream_t stream)
{
    const int G = p->cells_per_axis;
    const EwaldPairParams q = ewald_pair_params(G, G, G, p->num_columns, p->alpha, p->r_cut, nullptr);
    return launch_pairs<false>(q, p->batch_size * G * G * G, ewald_near_item_slots(p), p->num_points, order, pos, xs, start,
                               index, out, items, stream);
}

int launch_ewald_dipole_near_box(const nfft_hip_ewald_box_problem *p, int order, const float *pos, const float *xs,
                                 const int *start, const int64_t *index, float *out, void *items, hipStream_t stream)
{
    const EwaldPairParams q = ewald_pair_params(p->cells[0], p->cells[1], p->cells[2], p->num_columns, p->alpha, p->r_cut, p->box);
    return launch_pairs<true>(q, p->batch_size * p->cells[0] * p->cells[1] * p->cells[2], ewald_near_box_item_slots(p),
                              p->num_points, order, pos, xs, start, index, out, items, stream);
}

int launch_ewald_dipole_spectral(int64_t N, int64_t batch_size, int64_t num_columns, int order, const void *band,
                                 const float *coeffs, const double *box_inverse, void *out, hipStream_t stream)
{
    return launch_spectral_elements(order == 2 ? ewald_dipole_spectral_kernel<2> : ewald_dipole_spectral_kernel<1>, N, batch_size,
                                    num_columns, band, coeffs, box_inverse, out, stream);
}

}  // namespace nfft
