// Fused step of the Ewald sum for the periodic 1/r: what a constant-pressure step needs -- the
// potential, the field, the energy and the virial tensor -- from one walk over the pairs and one pass over the spectrum,
// in place of the sweep of ewald_near.hip plus the two reductions of ewald_virial.hip (sections 7g to 7i have the formulas).
// Both kernels are written from the pieces of virial_frame.h and spectral_frame.h (section 7w).
//
// ewald_step_near_kernel      ewald_near_kernel<CC, true, BOX> and virial_near_kernel<CC, CoulombVirialWeight> in one: the
//                             same items, lanes, LDS tiles, 27-cell walk, image, branch and pair weights, and per passing pair
//                             and column ten float32 sums: w v, the three mg d_a v and the six mg d_a d_b v (xx, yy, zz, yz,
//                             xz, xy).  At the end of a column pass a lane with a target stores z and f through `index` as the
//                             field sweep does, and seven of the sums (w, xx .. xy) go through the pair reductions' epilogue
//                             (pair_sums_to_partial).  One partial [7, Cr] per item slot.
// ewald_step_spectral_kernel  virial_far_kernel<CC, CoulombStrain> -- the same sweep, loads, weights and sums, hence the same
//                             order of additions -- which also writes, for every cell, the four spectra b_k band and
//                             (2 pi i kappa_a) b_k band whose forward transform is the far part of (phi, E):
//                             spectra [B, N, N, N, 4, C].  Zeros where b_k = 0.  2 pi kappa is formed in float32 from the
//                             float64 inverse, as the dipole sum's spectral step does.
//
// The second level of both is launch_virial_sum_terms of ewald_virial.hip, and the workspaces are that file's.  No atomics
// anywhere and every order of addition is fixed by the launch geometry: two calls give the same bits.
#include "spectral_frame.h"

namespace nfft {

namespace {

constexpr int kStepSums = 10;  // w; mg d_x, d_y, d_z; mg d_a d_b in the order of the virial's terms

template <int CC, bool BOX>
__global__ void __launch_bounds__(kNearBlock) ewald_step_near_kernel(EwaldPairParams q, const int2 *__restrict__ items,
                                                                     const float *__restrict__ pos, const float *__restrict__ xr,
                                                                     const int *__restrict__ start,
                                                                     const int64_t *__restrict__ index, float *__restrict__ z,
                                                                     float *__restrict__ f, double *__restrict__ partial)
{
    __shared__ float4 s_pos[kNearTile];
    __shared__ __attribute__((aligned(16))) float s_x[kNearTile * CC];
    __shared__ double s_red[kNearBlock / 64][kVirialTerms * CC];
    const int2 item = items[blockIdx.x];
    if (item.x < 0) return;  // (uniform: an empty slot; the second level skips it)
    const PairLane lane = pair_lane(item, start);
    const WrappedWalk walk(lane.cell, q.G0, BOX ? q.G1 : q.G0, BOX ? q.G2 : q.G0);
    // (a lane without a target sums pairs of the origin; it stores nothing and its sums are replaced by zero)
    const float4 t = lane_position(lane, pos, 3, 0.f);
    for (int64_t col0 = 0; col0 < q.Cr; col0 += CC) {
        float acc[kStepSums][CC];
#pragma unroll
        for (int e = 0; e < kStepSums; ++e)
#pragma unroll
            for (int c = 0; c < CC; ++c) acc[e][c] = 0.f;
        const StageColumns<CC> stage = {s_x, xr, q.Cr, col0};
        walk(start, [&](int first, int last) {
            sweep_range<2>(first, last, lane, s_pos, pos, 3, stage, [&](int j) {
                const PairSep d = ewald_image<BOX>(t, s_pos[j], q);
                // the lanes that fail the test sit the expansion out
                if (!(d.rr > 0.f && d.rr < q.rc2)) return;
                const EwaldPairWeight e(d.rr, q);
                const float w = e.w, mg = e.mg(q);
                const float gx = mg * d.dx, gy = mg * d.dy, gz = mg * d.dz;
                const float pxx = gx * d.dx, pyy = gy * d.dy, pzz = gz * d.dz;
                const float pyz = gy * d.dz, pxz = gx * d.dz, pxy = gx * d.dy;
#pragma unroll
                for (int c = 0; c < CC; ++c) {
                    const float v = s_x[j * CC + c];
                    acc[0][c] += w * v;
                    acc[1][c] += gx * v;
                    acc[2][c] += gy * v;
                    acc[3][c] += gz * v;
                    acc[4][c] += pxx * v;
                    acc[5][c] += pyy * v;
                    acc[6][c] += pzz * v;
                    acc[7][c] += pyz * v;
                    acc[8][c] += pxz * v;
                    acc[9][c] += pxy * v;
                }
            });
        });
        if (lane.active) {
            const int64_t row = index[lane.ti];
            float *zp = z + row * q.Cr + col0;
            float *fp = f + row * 3 * q.Cr + col0;
#pragma unroll
            for (int c = 0; c < CC; ++c)
                if (col0 + c < q.Cr) {
                    zp[c] = acc[0][c];
                    fp[c] = acc[1][c];
                    fp[q.Cr + c] = acc[2][c];
                    fp[2 * q.Cr + c] = acc[3][c];
                }
        }
        // (the virial's terms: the sums 0 and 4 to 9)
        pair_sums_to_partial<CC>(lane, xr, q.Cr, col0, [&](int e, int c) { return acc[e ? 3 + e : 0][c]; }, s_red, partial);
    }
}

template <int CC>
__global__ void __launch_bounds__(kVirialBlock) ewald_step_spectral_kernel(SpectralHead h, BoxInverse inv, CoulombStrain strain,
                                                                           TwoPiInverse tpi, const float2 *__restrict__ band,
                                                                           const float *__restrict__ coeffs,
                                                                           float2 *__restrict__ spectra,
                                                                           double *__restrict__ partial)
{
    __shared__ double s_red[kVirialBlock / 64][kVirialTerms * CC];
    const int64_t cells = (int64_t)h.N * h.N * h.N;
    const int set = blockIdx.x / h.blocks;  // (the workgroup's point set)
    const float2 *bb = band + (int64_t)set * cells * h.C;
    float2 *ss = spectra + (int64_t)set * cells * 4 * h.C;
    for (int64_t col0 = 0; col0 < h.C; col0 += CC) {
        double acc[kVirialTerms * CC];
#pragma unroll
        for (int n = 0; n < kVirialTerms * CC; ++n) acc[n] = 0.0;
        for (CellSweep sweep(h.N, h.blocks); sweep.more(); sweep.advance()) {
            const int64_t cell = sweep.cell;
            const float bk = coeffs[cell];
            int k0, k1, k2;
            sweep.frequency(k0, k1, k2);
            float2 v[CC];
            float2 *sp = ss + cell * 4 * h.C + col0;
            const bool whole = load_cell<CC>(bb + cell * h.C + col0, h.C, col0, h.wide, v);  // (aligned on both sides)
            // the four spectra of every column: R = b_k band, then i tau_a R with tau = 2 pi kappa in float32.  b_k = 0
            // (k = 0 and the zeroed planes k_a = -N/2) gives zeros, whatever band holds there
            const float3 tau = tpi.tau((float)k0, (float)k1, (float)k2);
            float2 o[4][CC];
#pragma unroll
            for (int c = 0; c < CC; ++c) {
                const float2 R = bk == 0.f ? make_float2(0.f, 0.f) : make_float2(bk * v[c].x, bk * v[c].y);
                o[0][c] = R;
                o[1][c] = times_i(tau.x, R);
                o[2][c] = times_i(tau.y, R);
                o[3][c] = times_i(tau.z, R);
            }
            if (whole) {  // (4 CC complex numbers in a row)
                float4 *sp4 = reinterpret_cast<float4 *>(sp);
#pragma unroll
                for (int n = 0; n < 2 * CC; ++n) {
                    const float2 a = o[(2 * n) / CC][(2 * n) % CC], b = o[(2 * n + 1) / CC][(2 * n + 1) % CC];
                    sp4[n] = make_float4(a.x, a.y, b.x, b.y);
                }
            } else {
#pragma unroll
                for (int c = 0; c < CC; ++c)
                    if (col0 + c < h.C) {
#pragma unroll
                        for (int s = 0; s < 4; ++s) sp[s * h.C + c] = o[s][c];
                    }
            }
            if (bk == 0.f) continue;
            const double3 kap = inv.kappa(k0, k1, k2);
            const double b = (double)bk;
            const double t = strain(cell, b, kap.x, kap.y, kap.z);
            double wgt[kVirialTerms];
            strain_weights(b, t, kap.x, kap.y, kap.z, wgt);
#pragma unroll
            for (int c = 0; c < CC; ++c) {
                const double p = (double)v[c].x * (double)v[c].x + (double)v[c].y * (double)v[c].y;
#pragma unroll
                for (int e = 0; e < kVirialTerms; ++e) acc[e * CC + c] += wgt[e] * p;
            }
        }
        block_sums_to_partial<kVirialTerms, CC>(acc, s_red, 0.5, h.C, col0, partial);
    }
}

}  // namespace

// (the unit cube runs as the identity box, as the virial's pair reduction does: one instantiation per column count)
int launch_ewald_step_near(const nfft_hip_ewald_box_problem *p, const float *pos, const float *xr, const int *start,
                           const int64_t *index, float *z, float *f, double *out, void *workspace, hipStream_t stream)
{
    const EwaldPairParams q = ewald_pair_params(p->cells[0], p->cells[1], p->cells[2], p->num_columns, p->alpha, p->r_cut, p->box);
    return launch_pair_reduction(p, kVirialTerms, q.Cr, start, out, workspace, stream,
                                 [&](dim3 grid, const int2 *items, double *partial) {
                                     dispatch_columns(q.Cr, [&](auto CC) {
                                         hipLaunchKernelGGL((ewald_step_near_kernel<CC(), true>), grid, dim3(kNearBlock), 0, stream, q,
                                                            items, pos, xr, start, index, z, f, partial);
                                     });
                                 });
}

int launch_ewald_step_spectral(int64_t N, int64_t batch_size, int64_t num_columns, const void *band, const float *coeffs,
                               const double *box_inverse, double pi2_over_alpha2, void *spectra, double *out, void *workspace,
                               hipStream_t stream)
{
    return launch_spectral_reduction(
        N, batch_size, num_columns, (uintptr_t)band | (uintptr_t)spectra, kVirialTerms, out, workspace, stream,
        [&](dim3 grid, const SpectralHead &h, double *partial) {
            dispatch_columns(h.C, [&](auto CC) {
                hipLaunchKernelGGL((ewald_step_spectral_kernel<CC()>), grid, dim3(kVirialBlock), 0, stream, h, BoxInverse(box_inverse),
                                   CoulombStrain{pi2_over_alpha2}, TwoPiInverse(box_inverse), (const float2 *)band, coeffs,
                                   (float2 *)spectra, partial);
            });
        });
}

}  // namespace nfft
