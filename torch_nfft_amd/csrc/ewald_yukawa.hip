// Near part of the Ewald sum for the periodic screened Coulomb (Yukawa) potential e^(-lambda r) / r: for
// one point set on both sides, with beta = lambda / (2 alpha),
//
//     z[i, c]    =  sum_{j: 0 < r_ij < r_c} w(r_ij) xr[j, c],            w(r)  = (P + M) / (2 r),
//     f[i, a, c] =  sum_{j: 0 < r_ij < r_c} mg(r_ij) d_ij[a] xr[j, c],   mg(r) = -w'(r) / r = (w + lambda (M - P) / 2 + g) / r^2,
//     P = e^(lambda r) erfc(alpha r + beta),  M = e^(-lambda r) erfc(alpha r - beta),  g = (2 alpha / sqrt(pi)) e^(-alpha^2 r^2 - beta^2),
//
// d_ij the minimum image of x_i - x_j and r_ij its length, and the pair part of the virial tensor of the same sum,
//
//     near[b, 0, c]  = 1/2 sum_{i in set b} x_ic sum_{j: 0 < r_ij < r_c} w(r_ij) x_jc                            (energy)
//     near[b, e, c]  = 1/2 sum_i x_ic sum_j mg(r_ij) d_ij,a d_ij,b x_jc,   e = 1 .. 6: ab = xx, yy, zz, yz, xz, xy.
//
// ewald_yukawa_near_kernel         the twin of ewald_near_kernel and ewald_disp_near_kernel (ewald_near.hip, sections 7g and 7h,
//                                  which say what BOX = false and BOX = true mean): the same frame of pair_frame.h, the same
//                                  wrapped walk, image, distance branch, staging and epilogue.
// virial_near_kernel<CC, YukawaVirialWeight>  the pair reduction of virial_frame.h with this sum's
//                                  weights (until 7w: ewald_yukawa_virial_near_kernel<CC>); the second level and the
//                                  workspace are those of ewald_virial.hip.
// Their own is the pair weight (YukawaPairWeight in pair_frame.h, which says which float32 form it takes and why): one erfcf,
// one erfcxf, one rsqrtf and two exponentials.  At lambda = 0 it is the Coulomb weight.  The spectral part of the virial is
// launch_ewald_dispersion_virial_far with this sum's two grids: there is no spectral kernel here.
//
// No atomics anywhere and every order of addition is fixed by the launch geometry: two calls give the same bits.
#include "virial_frame.h"

namespace nfft {

namespace {

template <int CC, bool FIELD, bool BOX>
__global__ void __launch_bounds__(kNearBlock) ewald_yukawa_near_kernel(EwaldPairParams q, YukawaPairParams y,
                                                                       const int2 *__restrict__ items,
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
                const YukawaPairWeight e(d.rr, q, y);
#pragma unroll
                for (int c = 0; c < CC; ++c) acc[c] += e.w * s_x[j * CC + c];
                if (FIELD) {
                    const float mg = e.mg(y);
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

// the pair weight of the screened sum (virial_frame.h has what a weight is): YukawaPairWeight with its block
struct YukawaVirialWeight {
    typedef YukawaPairParams Params;
    static __device__ __forceinline__ void weights(float rr, const EwaldPairParams &q, const Params &y, float &w, float &mg)
    {
        const YukawaPairWeight e(rr, q, y);
        w = e.w;
        mg = e.mg(y);
    }
};

// the items of `cells` cells over `num_points` points into `slots` slots, then the pair kernel
template <bool BOX>
int launch_pairs(const EwaldPairParams &q, const YukawaPairParams &y, int64_t cells, int64_t slots, int64_t num_points,
                 bool with_field, const float *pos, const float *xr, const int *start, const int64_t *index, float *z, float *f,
                 void *items, hipStream_t stream)
{
    if (int rc = launch_nearfield_items(cells, num_points, start, (int2 *)items, stream)) return rc;
    const dim3 grid((unsigned)slots), block(kNearBlock);
    dispatch_flag(with_field, [&](auto FIELD) {
        dispatch_columns(q.Cr, [&](auto CC) {
            hipLaunchKernelGGL((ewald_yukawa_near_kernel<CC(), FIELD() != 0, BOX>), grid, block, 0, stream, q, y,
                               (const int2 *)items, pos, xr, start, index, z, f);
        });
    });
    NFFT_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace

// (the cell counts and the item slots are those of ewald_near.hip: one workspace serves all the sweeps)
int launch_ewald_yukawa_near(const nfft_hip_ewald_problem *p, double screening, const float *pos, const float *xr, const int *start,
                             const int64_t *index, float *z, float *f, void *items, hipStream_t stream)
{
    const int G = p->cells_per_axis;
    const EwaldPairParams q = ewald_pair_params(G, G, G, p->num_columns, p->alpha, p->r_cut, nullptr);
    return launch_pairs<false>(q, yukawa_pair_params(p->alpha, screening), p->batch_size * G * G * G, ewald_near_item_slots(p),
                               p->num_points, p->with_field != 0, pos, xr, start, index, z, f, items, stream);
}

int launch_ewald_yukawa_near_box(const nfft_hip_ewald_box_problem *p, double screening, const float *pos, const float *xr,
                                 const int *start, const int64_t *index, float *z, float *f, void *items, hipStream_t stream)
{
    const EwaldPairParams q = ewald_pair_params(p->cells[0], p->cells[1], p->cells[2], p->num_columns, p->alpha, p->r_cut, p->box);
    return launch_pairs<true>(q, yukawa_pair_params(p->alpha, screening), p->batch_size * p->cells[0] * p->cells[1] * p->cells[2],
                              ewald_near_box_item_slots(p), p->num_points, p->with_field != 0, pos, xr, start, index, z, f, items,
                              stream);
}

int launch_ewald_yukawa_virial_near(const nfft_hip_ewald_box_problem *p, double screening, const float *pos, const float *xr,
                                    const int *start, double *out, void *workspace, hipStream_t stream)
{
    return launch_virial_near<YukawaVirialWeight>(p, yukawa_pair_params(p->alpha, screening), pos, xr, start, out, workspace, stream);
}

}  // namespace nfft
