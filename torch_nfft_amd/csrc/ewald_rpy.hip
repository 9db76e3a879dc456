// Periodic Rotne-Prager-Yamakawa sum (Beenakker's Ewald sum): the pair sweep.
//
// Source j is a sphere of radius a with a Cartesian force f_j.  With d = d_ij the minimum image of x_i - x_j, r = |d|,
// m = d . f_j and the weights W1, W2, D1 = W1' / r, D2 = W2' / r of RpyPairWeight below, over the pairs 0 < r < r_c of one
// point set:
//
//     u[i, a]    = sum_j  W1 f_j,a + W2 m d_a
//     G[i, a, b] = sum_j  D1 f_j,a d_b + D2 m d_a d_b + W2 (m delta_ab + d_a f_j,b)                          (G_ab = d u_a / d x_b)
//
// ORDER = 1 gives the three sums of u per column, ORDER = 2 adds the nine of G, row-major in ab: out [n, 3 or 12, Cr] in the
// caller's point order.  Coincident points (r = 0) do not see each other, as in every sibling; the sphere's own mobility is
// the self term of the Python layer.
//
// The pair kernel is the twin of ewald_stokeslet_near_kernel (ewald_stokeslet.hip, section 7m): the same frame of
// pair_frame.h, the same wrapped walk, image and distance branch, the same float4 staging of the forces and the same pair body,
// no atomics.  Its own: the weights, which carry the finite-size terms in a^2 and, for overlapping spheres r < 2 a, a second
// branch; the radius and (2 a)^2 travel as kernel arguments beside the block of the Ewald pair kernels.  The far part is the
// Stokeslet sum's spectral kernel with another coefficient table.
#include "pair_frame.h"

namespace nfft {

namespace {

// staging policy: (f_x, f_y, f_z, 0) of CC columns from col0 on of xs [points, 3, Cr] per staged point, zero past Cr (that of
// ewald_stokeslet.hip, restated: pair_frame.h and the existing pair kernels stay as they are)
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

// The pair weights of the RPY sum from rr = r^2 > 0.  With the Smith functions B_0 = erfc(alpha r) / r,
// B_l = ((2l - 1) B_(l-1) + (2 alpha^2)^(l-1) g) / r^2, g = (2 alpha / sqrt(pi)) e^(-alpha^2 r^2), and q = a^2 / 3, the screened part of
// (1 + q lap) S:
//     W1 = (B_0 - g) + q (2 B_1 + (8 alpha^2 - 4 alpha^4 r^2) g)                 weighs f
//     W2 = B_1 + q (4 alpha^4 g - 2 B_2)                                      weighs (d . f) d
//     D1 = W1' / r = (2 alpha^2 g - B_1) + q (-2 B_2 + (8 alpha^6 r^2 - 24 alpha^4) g)
//     D2 = W2' / r = -B_2 + q (2 B_3 - 8 alpha^6 g)                                                      (ORDER = 2)
// For overlapping spheres, rr < (2 a)^2, the tensor is (4 / (3 a)) ((1 - 9 r / (32 a)) I + 3 d d^T / (32 a r)) and the weight is
// that form minus the far kernel, written with the complementary functions E_0 = (1 - erfc(alpha r)) / r,
// E_l = ((2l - 1) E_(l-1) - (2 alpha^2)^(l-1) g) / r^2 (E_l = (2l - 1)!! / r^(2l+1) - B_l), h = 1 / (8 a^2):
//     W1 = 4 / (3 a) - 3 h r - (E_0 + g) - q (2 E_1 - (8 alpha^2 - 4 alpha^4 r^2) g)      W2 = h / r - E_1 + q (2 E_2 + 4 alpha^4 g)
//     D1 = -3 h / r + (E_1 + 2 alpha^2 g) + q (2 E_2 + (8 alpha^6 r^2 - 24 alpha^4) g)      D2 = -h / r^3 + E_2 - q (2 E_3 + 8 alpha^6 g)
// Adding the difference to the unscreened tensor as powers of 1 / r instead cancels terms of the size a^2 / r^3 against a
// result of the size 1 / a and is five times worse in float32 at r = a / 2 (section 7n has both figures).
// One erfcf, one __expf, one rsqrtf; the branch is around the overlap terms only.

// what the weights take of the radius, formed once per work item from the kernel's two arguments
struct RpyRadius {
    float q, four_a2, lead, h;  // a^2 / 3, (2 a)^2, 4 / (3 a), 1 / (8 a^2)
    __device__ __forceinline__ RpyRadius(float radius, float four_a2_)
        : q(radius * radius * (1.f / 3.f)), four_a2(four_a2_), lead(4.f / (3.f * radius)), h(0.125f / (radius * radius))
    {
    }
};

template <int ORDER>
struct RpyPairWeight {
    float W1, W2, D1, D2;
    __device__ __forceinline__ RpyPairWeight(float rr, const EwaldPairParams &p, const RpyRadius &s)
    {
        const float ir = rsqrtf(rr), ir2 = ir * ir, r = rr * ir;
        const float two_alpha2 = -2.f * p.neg_alpha2;
        const float q = s.q;
        const float g = p.slope * __expf(p.neg_alpha2 * rr);
        const float g2 = two_alpha2 * g, g4 = two_alpha2 * g2, g6 = two_alpha2 * g4;  // 2 alpha^2 g, 4 alpha^4 g, 8 alpha^6 g
        const float ec = erfcf(p.alpha * r);
        const float s1 = fmaf(-g4, rr, 4.f * g2);      // (8 alpha^2 - 4 alpha^4 r^2) g
        const float s2 = fmaf(g6, rr, -6.f * g4);      // (8 alpha^6 r^2 - 24 alpha^4) g
        const float B0 = ec * ir;
        const float B1 = (B0 + g) * ir2;
        const float B2 = fmaf(3.f, B1, g2) * ir2;
        W1 = fmaf(q, fmaf(2.f, B1, s1), B0 - g);
        W2 = fmaf(q, fmaf(-2.f, B2, g4), B1);
        if (ORDER == 2) {
            const float B3 = fmaf(5.f, B2, g4) * ir2;
            D1 = fmaf(q, fmaf(-2.f, B2, s2), g2 - B1);
            D2 = fmaf(q, fmaf(2.f, B3, -g6), -B2);
        } else {
            D1 = D2 = 0.f;
        }
        if (rr < s.four_a2) {
            const float h = s.h, lead = s.lead;
            const float E0 = (1.f - ec) * ir;
            const float E1 = (E0 - g) * ir2;
            const float E2 = fmaf(3.f, E1, -g2) * ir2;
            W1 = fmaf(-3.f * h, r, lead) - fmaf(q, fmaf(2.f, E1, -s1), E0 + g);
            W2 = h * ir - fmaf(-q, fmaf(2.f, E2, g4), E1);
            if (ORDER == 2) {
                const float E3 = fmaf(5.f, E2, -g4) * ir2;
                D1 = fmaf(q, fmaf(2.f, E2, s2), E1 + g2) - 3.f * h * ir;
                D2 = fmaf(-q, fmaf(2.f, E3, g6), E2) - h * ir * ir2;
            }
        }
    }
};

template <int CC, int ORDER, bool BOX>
__global__ void __launch_bounds__(kNearBlock) ewald_rpy_near_kernel(EwaldPairParams q, float radius, float four_a2,
                                                                    const int2 *__restrict__ items,
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
    const RpyRadius sphere(radius, four_a2);
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
                const RpyPairWeight<ORDER> w(d.rr, q, sphere);
                const float dd[3] = {d.dx, d.dy, d.dz};
                const float p[3] = {w.D1 * d.dx, w.D1 * d.dy, w.D1 * d.dz};  // D1 d: the same for every column
#pragma unroll
                for (int c = 0; c < CC; ++c) {
                    const float4 v = s_x[j * CC + c];  // (f, 0)
                    const float f[3] = {v.x, v.y, v.z};
                    const float m = fmaf(v.z, d.dz, fmaf(v.y, d.dy, v.x * d.dx));
                    const float mW2 = m * w.W2;
#pragma unroll
                    for (int a = 0; a < 3; ++a) acc[a][c] += fmaf(mW2, dd[a], w.W1 * f[a]);
                    if constexpr (ORDER == 2) {
                        // G_ab = f_a p_b + d_a e_b + W2 m delta_ab,   e = W2 f + D2 m d
                        const float mD2 = m * w.D2;
                        float e[3];
#pragma unroll
                        for (int b = 0; b < 3; ++b) e[b] = fmaf(w.W2, f[b], mD2 * dd[b]);
#pragma unroll
                        for (int a = 0; a < 3; ++a)
#pragma unroll
                            for (int b = 0; b < 3; ++b) {
                                const float g = fmaf(dd[a], e[b], f[a] * p[b]);
                                acc[3 + 3 * a + b][c] += a == b ? g + mW2 : g;
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
int launch_pairs(const EwaldPairParams &q, double radius, int64_t cells, int64_t slots, int64_t num_points, int order,
                 const float *pos, const float *xs, const int *start, const int64_t *index, float *out, void *items,
                 hipStream_t stream)
{
    if (int rc = launch_nearfield_items(cells, num_points, start, (int2 *)items, stream)) return rc;
    const dim3 grid((unsigned)slots), block(kNearBlock);
    const float a = (float)radius, four_a2 = (float)(4.0 * radius * radius);
    dispatch_flag(order == 2, [&](auto SECOND) {
        dispatch_columns(q.Cr, [&](auto CC) {
            hipLaunchKernelGGL((ewald_rpy_near_kernel<CC(), 1 + SECOND(), BOX>), grid, block, 0, stream, q, a, four_a2,
                               (const int2 *)items, pos, xs, start, index, out);
        });
    });
    NFFT_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace

// (the cell counts and the item slots are those of ewald_near.hip: one workspace serves every sweep)
int launch_ewald_rpy_near(const nfft_hip_ewald_problem *p, int order, double radius, const float *pos, const float *xs,
                          const int *start, const int64_t *index, float *out, void *items, hipStream_t stream)
{
    const int G = p->cells_per_axis;
    const EwaldPairParams q = ewald_pair_params(G, G, G, p->num_columns, p->alpha, p->r_cut, nullptr);
    return launch_pairs<false>(q, radius, p->batch_size * G * G * G, ewald_near_item_slots(p), p->num_points, order, pos, xs,
                               start, index, out, items, stream);
}

int launch_ewald_rpy_near_box(const nfft_hip_ewald_box_problem *p, int order, double radius, const float *pos, const float *xs,
                              const int *start, const int64_t *index, float *out, void *items, hipStream_t stream)
{
    const EwaldPairParams q = ewald_pair_params(p->cells[0], p->cells[1], p->cells[2], p->num_columns, p->alpha, p->r_cut, p->box);
    return launch_pairs<true>(q, radius, p->batch_size * p->cells[0] * p->cells[1] * p->cells[2], ewald_near_box_item_slots(p),
                              p->num_points, order, pos, xs, start, index, out, items, stream);
}

}  // namespace nfft
