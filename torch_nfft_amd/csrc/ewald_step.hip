// Fused step of the Ewald sum for the periodic 1/r: what a constant-pressure step needs -- the
// potential, the field, the energy and the virial tensor -- from one walk over the pairs and one pass over the spectrum,
// in place of the sweep of ewald_near.hip plus the two reductions of ewald_virial.hip (sections 7g to 7i have the formulas).
//
// ewald_step_near_kernel      ewald_near_kernel<CC, true, BOX> and ewald_virial_near_kernel<CC> in one: the same items,
//                             lanes, LDS tiles, 27-cell walk, image, branch and pair weights, and per passing pair and column
//                             ten float32 sums: w v, the three mg d_a v and the six mg d_a d_b v (xx, yy, zz, yz, xz, xy).
//                             At the end of a column pass a lane with a target stores z and f through `index` as the
//                             field sweep does, and every lane multiplies seven of its sums (w, xx .. xy) by x_i / 2 of
//                             its own target (exactly zero for a lane without one), in float64 from there on; the
//                             workgroup adds its lanes as the virial sweep does.  One partial [7, Cr] per item slot.
// ewald_step_spectral_kernel  ewald_virial_far_kernel -- the same thread-to-cell mapping, carried index digits, loads,
//                             weights and sums, hence the same order of additions -- which also writes, for every cell,
//                             the four spectra b_k band and (2 pi i kappa_a) b_k band whose forward transform is the far
//                             part of (phi, E): spectra [B, N, N, N, 4, C].  Zeros where b_k = 0.  2 pi kappa is formed
//                             in float32 from the float64 inverse, as the dipole sum's spectral step does.
//
// The second level of both is launch_virial_sum of ewald_virial.hip, and the workspaces are that file's.  No atomics
// anywhere and every order of addition is fixed by the launch geometry: two calls give the same bits.
#include "pair_frame.h"

namespace nfft {

namespace {

constexpr int kVirialTerms = 7;    // energy, xx, yy, zz, yz, xz, xy
constexpr int kVirialBlock = 256;  // lanes of the spectral kernel (and of the second level in ewald_virial.hip)
constexpr int kStepSums = 10;      // w; mg d_x, d_y, d_z; mg d_a d_b in the order of the virial's terms

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
        // x_i / 2 of the lane's own target, float64 from here on; a lane without a target adds exactly zero
        double red[kVirialTerms * CC];
#pragma unroll
        for (int c = 0; c < CC; ++c) {
            const bool live = lane.active && col0 + c < q.Cr;
            const double h = live ? 0.5 * (double)xr[(int64_t)lane.ti * q.Cr + col0 + c] : 0.0;
            red[c] = live ? h * (double)acc[0][c] : 0.0;
#pragma unroll
            for (int e = 1; e < kVirialTerms; ++e) red[e * CC + c] = live ? h * (double)acc[3 + e][c] : 0.0;
        }
        const double v = block_sum_f64(red, s_red);
        const int tid = threadIdx.x;
        if (tid < kVirialTerms * CC) {
            const int e = tid / CC, c = tid % CC;
            if (col0 + c < q.Cr) partial[((int64_t)blockIdx.x * kVirialTerms + e) * q.Cr + col0 + c] = v;
        }
    }
}

struct StepSpectralParams {
    int N, blocks;  // frequencies per axis; workgroups per point set
    int wide;       // band and spectra are 16-byte aligned: cells of one, two or four columns move in 16-byte pieces
    int64_t C;
    double i00, i10, i11, i20, i21, i22;  // the lower triangle of A^-1
    double p2a2;                          // pi^2 / alpha^2
    float t00, t10, t11, t20, t21, t22;   // 2 pi times the lower triangle of A^-1
};

// (x + i y) times the imaginary i t
__device__ __forceinline__ float2 times_i(float t, float2 r) { return make_float2(-t * r.y, t * r.x); }

template <int CC>
__global__ void __launch_bounds__(kVirialBlock) ewald_step_spectral_kernel(StepSpectralParams q, const float2 *__restrict__ band,
                                                                           const float *__restrict__ coeffs,
                                                                           float2 *__restrict__ spectra,
                                                                           double *__restrict__ partial)
{
    __shared__ double s_red[kVirialBlock / 64][kVirialTerms * CC];
    const int tid = threadIdx.x;
    const int N = q.N, half = q.N / 2;
    const int64_t cells = (int64_t)N * N * N;
    const int set = blockIdx.x / q.blocks, blk = blockIdx.x % q.blocks;  // (point set, workgroup within it)
    const float2 *bb = band + (int64_t)set * cells * q.C;
    float2 *ss = spectra + (int64_t)set * cells * 4 * q.C;
    for (int64_t col0 = 0; col0 < q.C; col0 += CC) {
        double acc[kVirialTerms * CC];
#pragma unroll
        for (int n = 0; n < kVirialTerms * CC; ++n) acc[n] = 0.0;
        // the cells blk * 256 + tid, + stride, + 2 stride, ...: their index (i0, i1, i2) is kept beside them and advanced
        // by the stride's own digits with carries, so that no division runs per cell
        const int stride = q.blocks * kVirialBlock;
        const unsigned first = (unsigned)blk * kVirialBlock + tid;
        int i2 = (int)(first % (unsigned)N), i1 = (int)((first / (unsigned)N) % (unsigned)N), i0 = (int)(first / ((unsigned)N * N));
        const int s2 = stride % N, s1 = (stride / N) % N, s0 = stride / (N * N);
        for (int64_t cell = first; cell < cells; cell += stride) {
            const float bk = coeffs[cell];
            const int k0 = i0 - half, k1 = i1 - half, k2 = i2 - half;
            i2 += s2;
            if (i2 >= N) {
                i2 -= N;
                ++i1;
            }
            i1 += s1;
            if (i1 >= N) {
                i1 -= N;
                ++i0;
            }
            i0 += s0;
            float2 v[CC];
            const float2 *bp = bb + cell * q.C + col0;
            float2 *sp = ss + cell * 4 * q.C + col0;
            bool whole = false;  // the cell's columns are these CC, and 16-byte aligned on both sides
            if constexpr (CC == 1) whole = q.C == 1 && q.wide;
            if constexpr (CC == 2) {
                if (q.C == 2 && q.wide) {  // (16 bytes per cell, aligned: one load)
                    const float4 u = *reinterpret_cast<const float4 *>(bp);
                    v[0] = make_float2(u.x, u.y);
                    v[1] = make_float2(u.z, u.w);
                    whole = true;
                }
            }
            if constexpr (CC == 4) {
                if (q.C == 4 && q.wide) {  // (32 bytes per cell, aligned: two loads)
                    const float4 u0 = reinterpret_cast<const float4 *>(bp)[0], u1 = reinterpret_cast<const float4 *>(bp)[1];
                    v[0] = make_float2(u0.x, u0.y);
                    v[1] = make_float2(u0.z, u0.w);
                    v[2] = make_float2(u1.x, u1.y);
                    v[3] = make_float2(u1.z, u1.w);
                    whole = true;
                }
            }
            if (CC == 1 || !whole) {
#pragma unroll
                for (int c = 0; c < CC; ++c) v[c] = col0 + c < q.C ? bp[c] : make_float2(0.f, 0.f);
            }
            // the four spectra of every column: R = b_k band, then i tau_a R with tau = 2 pi kappa in float32.  b_k = 0
            // (k = 0 and the zeroed planes k_a = -N/2) gives zeros, whatever band holds there
            const float kf0 = (float)k0, kf1 = (float)k1, kf2 = (float)k2;
            const float tx = q.t00 * kf0;
            const float ty = fmaf(q.t11, kf1, q.t10 * kf0);
            const float tz = fmaf(q.t22, kf2, fmaf(q.t21, kf1, q.t20 * kf0));
            float2 o[4][CC];
#pragma unroll
            for (int c = 0; c < CC; ++c) {
                const float2 R = bk == 0.f ? make_float2(0.f, 0.f) : make_float2(bk * v[c].x, bk * v[c].y);
                o[0][c] = R;
                o[1][c] = times_i(tx, R);
                o[2][c] = times_i(ty, R);
                o[3][c] = times_i(tz, R);
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
                    if (col0 + c < q.C) {
#pragma unroll
                        for (int s = 0; s < 4; ++s) sp[s * q.C + c] = o[s][c];
                    }
            }
            if (bk == 0.f) continue;
            // kappa = A^-1 k, A^-1 lower triangular
            const double kx = q.i00 * k0;
            const double ky = q.i10 * k0 + q.i11 * k1;
            const double kz = q.i20 * k0 + q.i21 * k1 + q.i22 * k2;
            const double kk = kx * kx + ky * ky + kz * kz;
            const double b = (double)bk;
            const double t = -2.0 * (1.0 / kk + q.p2a2) * b;
            double wgt[kVirialTerms];
            wgt[0] = b;
            wgt[1] = b + t * kx * kx;
            wgt[2] = b + t * ky * ky;
            wgt[3] = b + t * kz * kz;
            wgt[4] = t * ky * kz;
            wgt[5] = t * kx * kz;
            wgt[6] = t * kx * ky;
#pragma unroll
            for (int c = 0; c < CC; ++c) {
                const double p = (double)v[c].x * (double)v[c].x + (double)v[c].y * (double)v[c].y;
#pragma unroll
                for (int e = 0; e < kVirialTerms; ++e) acc[e * CC + c] += wgt[e] * p;
            }
        }
        const double v = block_sum_f64(acc, s_red);
        if (tid < kVirialTerms * CC) {
            const int e = tid / CC, c = tid % CC;
            if (col0 + c < q.C) partial[((int64_t)blockIdx.x * kVirialTerms + e) * q.C + col0 + c] = 0.5 * v;
        }
    }
}

}  // namespace

// (the unit cube runs as the identity box, as the virial's pair reduction does: one instantiation per column count)
int launch_ewald_step_near(const nfft_hip_ewald_box_problem *p, const float *pos, const float *xr, const int *start,
                           const int64_t *index, float *z, float *f, double *out, void *workspace, hipStream_t stream)
{
    const EwaldPairParams q = ewald_pair_params(p->cells[0], p->cells[1], p->cells[2], p->num_columns, p->alpha, p->r_cut, p->box);
    const int64_t cells_per_set = (int64_t)p->cells[0] * p->cells[1] * p->cells[2];
    const int64_t slots = ewald_virial_near_item_slots(p);
    int2 *items = (int2 *)workspace;
    double *partial = ewald_virial_near_partials(p, workspace);
    if (int rc = launch_nearfield_items(p->batch_size * cells_per_set, p->num_points, start, items, stream)) return rc;
    const dim3 grid((unsigned)slots), block(kNearBlock);
    dispatch_columns(q.Cr, [&](auto CC) {
        hipLaunchKernelGGL((ewald_step_near_kernel<CC(), true>), grid, block, 0, stream, q, (const int2 *)items, pos, xr, start,
                           index, z, f, partial);
    });
    NFFT_HIP_CHECK(hipGetLastError());
    return launch_virial_sum(partial, p->batch_size, q.Cr, 0, items, start, (int)cells_per_set, out, stream);
}

int launch_ewald_step_spectral(int64_t N, int64_t batch_size, int64_t num_columns, const void *band, const float *coeffs,
                               const double *box_inverse, double pi2_over_alpha2, void *spectra, double *out, void *workspace,
                               hipStream_t stream)
{
    const double two_pi = 6.28318530717958647692;
    StepSpectralParams q;
    q.N = (int)N;
    q.blocks = ewald_virial_far_blocks(N);
    q.C = num_columns;
    q.wide = (((uintptr_t)band | (uintptr_t)spectra) & 15) == 0 ? 1 : 0;  // (otherwise 8-byte pieces, which complex64 allows)
    q.i00 = box_inverse[0];
    q.i10 = box_inverse[1];
    q.i11 = box_inverse[2];
    q.i20 = box_inverse[3];
    q.i21 = box_inverse[4];
    q.i22 = box_inverse[5];
    q.p2a2 = pi2_over_alpha2;
    q.t00 = (float)(two_pi * box_inverse[0]);
    q.t10 = (float)(two_pi * box_inverse[1]);
    q.t11 = (float)(two_pi * box_inverse[2]);
    q.t20 = (float)(two_pi * box_inverse[3]);
    q.t21 = (float)(two_pi * box_inverse[4]);
    q.t22 = (float)(two_pi * box_inverse[5]);
    double *partial = (double *)workspace;
    const dim3 grid((unsigned)(q.blocks * batch_size)), block(kVirialBlock);
    dispatch_columns(q.C, [&](auto CC) {
        hipLaunchKernelGGL((ewald_step_spectral_kernel<CC()>), grid, block, 0, stream, q, (const float2 *)band, coeffs,
                           (float2 *)spectra, partial);
    });
    NFFT_HIP_CHECK(hipGetLastError());
    return launch_virial_sum(partial, batch_size, q.C, q.blocks, nullptr, nullptr, 0, out, stream);
}

}  // namespace nfft
