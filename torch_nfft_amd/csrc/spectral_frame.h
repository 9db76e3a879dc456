// The frame of the spectral kernels of the Ewald sums: what the kernels that walk the N^3 frequencies
// of a band [B, N, N, N, ..., C] share.
//
// The reductions -- virial_far_kernel<CC, Strain> below (ewald_virial.hip, ewald_disp_virial.hip), ewald_step_spectral_kernel
// (ewald_step.hip) and lj_step_spectral_kernel (ewald_lj_step.hip) -- run `blocks` workgroups of kVirialBlock lanes per point
// set.  A lane walks the cells blk * 256 + tid, + stride, + 2 stride, ... (CellSweep), forms kappa = A^-1 k in float64
// (BoxInverse) and the seven weights b, b + t kappa_a kappa_a, t kappa_a kappa_b of a cell once (strain_weights), reads the
// cell's columns (load_cell) and keeps float64 sums per thread; block_sums_to_partial of virial_frame.h halves the workgroup's
// sums into one partial per workgroup, and the second level is launch_virial_sum_terms of ewald_virial.hip
// (launch_spectral_reduction).  No atomics anywhere and every order of addition is fixed by the launch geometry.
//
// A STRAIN POLICY says where t_k = (d b_k / d |kappa|) / |kappa| comes from: a closed form (the Coulomb sum) or a grid of its
// own (the dispersion and Yukawa sums).  It is a kernel argument by value with
//     double operator()(cell, b, kx, ky, kz)       t of that cell; b = b_k != 0
//
// The kernels with one thread per (frequency, column) -- ewald_dipole_spectral_kernel, ewald_stokeslet_spectral_kernel -- share
// their block, the thread's element and their launch (SpectralElementParams, spectral_element, launch_spectral_elements).
//
// tau = 2 pi kappa is formed in float32 from the float64 inverse (TwoPiInverse) wherever a spectrum is multiplied by it.
// -ffp-contract=on fuses within one expression only: the expressions below stand as the kernels had them, statement by statement.
#pragma once
#include "virial_frame.h"

namespace nfft {

constexpr int kSpectralBlock = 256;  // lanes of the kernels with one thread per (frequency, column)

// the lower triangle of A^-1 in float64
struct BoxInverse {
    double i00, i10, i11, i20, i21, i22;
    explicit BoxInverse(const double *box_inverse)
        : i00(box_inverse[0]), i10(box_inverse[1]), i11(box_inverse[2]), i20(box_inverse[3]), i21(box_inverse[4]), i22(box_inverse[5])
    {
    }
    // kappa = A^-1 k
    __device__ __forceinline__ double3 kappa(int k0, int k1, int k2) const
    {
        double3 kap;
        kap.x = i00 * k0;
        kap.y = i10 * k0 + i11 * k1;
        kap.z = i20 * k0 + i21 * k1 + i22 * k2;
        return kap;
    }
};

// 2 pi times the lower triangle of A^-1, rounded to float32
struct TwoPiInverse {
    float t00, t10, t11, t20, t21, t22;
    explicit TwoPiInverse(const double *box_inverse)
    {
        const double two_pi = 6.28318530717958647692;
        t00 = (float)(two_pi * box_inverse[0]);
        t10 = (float)(two_pi * box_inverse[1]);
        t11 = (float)(two_pi * box_inverse[2]);
        t20 = (float)(two_pi * box_inverse[3]);
        t21 = (float)(two_pi * box_inverse[4]);
        t22 = (float)(two_pi * box_inverse[5]);
    }
    // tau = 2 pi kappa of the frequency (kf0, kf1, kf2)
    __device__ __forceinline__ float3 tau(float kf0, float kf1, float kf2) const
    {
        float3 t;
        t.x = t00 * kf0;
        t.y = fmaf(t11, kf1, t10 * kf0);
        t.z = fmaf(t22, kf2, fmaf(t21, kf1, t20 * kf0));
        return t;
    }
};

// (x + i y) times the imaginary i t
__device__ __forceinline__ float2 times_i(float t, float2 r) { return make_float2(-t * r.y, t * r.x); }

// ---- the reductions ---------------------------------------------------------------------------------------------------

// the head of a reduction's block
struct SpectralHead {
    int N, blocks;  // frequencies per axis; workgroups per point set
    int wide;       // the band (and the spectra) are 16-byte aligned: a cell of two or four columns moves in 16-byte pieces
    int64_t C;      // columns of the band and of the sums (the Lennard-Jones step: its band's two are fixed, one column of sums)
};

// The cells blk * 256 + tid, + stride, + 2 stride, ... of the N^3, blk = blockIdx.x % blocks the workgroup within its point
// set: `for (CellSweep sweep(N, blocks); sweep.more(); sweep.advance())` with sweep.cell and sweep.frequency(k0, k1, k2) in
// the body.  The index (i0, i1, i2) is kept beside the cell and advanced by the stride's own digits with carries, so that no
// division runs per cell.  (A loop in the kernel, not a callable per cell: with the body inlined as a callable the Coulomb
// step's spectral kernel ran 1.3 to 1.5 times as long, profiles/r21_reduction_frames.md.)
struct CellSweep {
    int N, half, stride, s0, s1, s2, i0, i1, i2;
    int64_t cells, cell;
    __device__ __forceinline__ CellSweep(int n, int blocks) : N(n), half(n / 2), stride(blocks * kVirialBlock)
    {
        cells = (int64_t)N * N * N;
        const unsigned first = (blockIdx.x % blocks) * kVirialBlock + threadIdx.x;
        i2 = (int)(first % (unsigned)N), i1 = (int)((first / (unsigned)N) % (unsigned)N), i0 = (int)(first / ((unsigned)N * N));
        s2 = stride % N, s1 = (stride / N) % N, s0 = stride / (N * N);
        cell = first;
    }
    __device__ __forceinline__ bool more() const { return cell < cells; }
    // on to the next cell, its digits with it
    __device__ __forceinline__ void advance()
    {
        cell += stride;
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
    }
    // the frequency of `cell`
    __device__ __forceinline__ void frequency(int &k0, int &k1, int &k2) const { k0 = i0 - half, k1 = i1 - half, k2 = i2 - half; }
};

// The CC columns from col0 on of the cell at bp (its column col0), zero past C.  Returns `whole`: the cell's columns are
// these CC and it is 16-byte aligned, so that it moves in 16-byte pieces (read so here for two and four columns)
template <int CC>
__device__ __forceinline__ bool load_cell(const float2 *__restrict__ bp, int64_t C, int64_t col0, int wide, float2 (&v)[CC])
{
    bool whole = false;
    if constexpr (CC == 1) whole = C == 1 && wide;
    if constexpr (CC == 2) {
        if (C == 2 && wide) {  // (16 bytes per cell, aligned: one load)
            const float4 u = *reinterpret_cast<const float4 *>(bp);
            v[0] = make_float2(u.x, u.y);
            v[1] = make_float2(u.z, u.w);
            whole = true;
        }
    }
    if constexpr (CC == 4) {
        if (C == 4 && wide) {  // (32 bytes per cell, aligned: two loads)
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
        for (int c = 0; c < CC; ++c) v[c] = col0 + c < C ? bp[c] : make_float2(0.f, 0.f);
    }
    return whole;
}

// the seven weights of a cell: b for the energy, b delta_ab + t kappa_a kappa_b for xx, yy, zz, yz, xz, xy
__device__ __forceinline__ void strain_weights(double b, double t, double kx, double ky, double kz, double (&wgt)[kVirialTerms])
{
    wgt[0] = b;
    wgt[1] = b + t * kx * kx;
    wgt[2] = b + t * ky * ky;
    wgt[3] = b + t * kz * kz;
    wgt[4] = t * ky * kz;
    wgt[5] = t * kx * kz;
    wgt[6] = t * kx * ky;
}

// t_k of the Coulomb sum, b_k = exp(-pi^2 kappa^2 / alpha^2) / (pi V kappa^2): -2 (1 / kappa^2 + pi^2 / alpha^2) b_k; kappa != 0
__device__ __forceinline__ double coulomb_strain(double b, double kx, double ky, double kz, double p2a2)
{
    const double kk = kx * kx + ky * ky + kz * kz;
    return -2.0 * (1.0 / kk + p2a2) * b;
}

// strain policies: the closed form of the Coulomb sum with pi^2 / alpha^2 ...
struct CoulombStrain {
    double p2a2;
    __device__ __forceinline__ double operator()(int64_t, double b, double kx, double ky, double kz) const
    {
        return coulomb_strain(b, kx, ky, kz, p2a2);
    }
};

// ... and a grid [N, N, N] that the host side evaluated in float64
struct TableStrain {
    const float *__restrict__ strain;
    __device__ __forceinline__ double operator()(int64_t cell, double, double, double, double) const { return (double)strain[cell]; }
};

// One thread per grid cell, the columns innermost as stored: kappa from the index, the seven weights in float64 once per
// cell, |band|^2 per column, float64 sums per thread, the workgroup's sum.  One partial [7, C] per workgroup.  Cells with
// b_k = 0 are skipped: the zeroed planes k_a = -N/2, coefficients below float32, and k = 0 where the table has a zero there
template <int CC, class Strain>
__global__ void __launch_bounds__(kVirialBlock) virial_far_kernel(SpectralHead h, BoxInverse inv, Strain strain,
                                                                  const float2 *__restrict__ band, const float *__restrict__ coeffs,
                                                                  double *__restrict__ partial)
{
    __shared__ double s_red[kVirialBlock / 64][kVirialTerms * CC];
    const int64_t cells = (int64_t)h.N * h.N * h.N;
    const float2 *bb = band + (int64_t)(blockIdx.x / h.blocks) * cells * h.C;  // (the workgroup's point set)
    for (int64_t col0 = 0; col0 < h.C; col0 += CC) {
        double acc[kVirialTerms * CC];
#pragma unroll
        for (int n = 0; n < kVirialTerms * CC; ++n) acc[n] = 0.0;
        for (CellSweep sweep(h.N, h.blocks); sweep.more(); sweep.advance()) {
            const int64_t cell = sweep.cell;
            const float bk = coeffs[cell];
            int k0, k1, k2;
            sweep.frequency(k0, k1, k2);
            if (bk == 0.f) continue;
            const double3 kap = inv.kappa(k0, k1, k2);
            const double b = (double)bk;
            const double t = strain(cell, b, kap.x, kap.y, kap.z);
            double wgt[kVirialTerms];
            strain_weights(b, t, kap.x, kap.y, kap.z, wgt);
            float2 v[CC];
            load_cell<CC>(bb + cell * h.C + col0, h.C, col0, h.wide, v);
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

// The launch sequence of a reduction over band [batch_size, N, N, N, ..]: the head (`addresses`: the band's, or'ed with
// that of the spectra where the kernel writes some), launch(grid, head, partial) -- the caller's kernel -- and the second
// level over the `blocks` partials [terms, C] of every point set: out [batch_size, terms, C].  `workspace`: those partials
template <typename Launch>
int launch_spectral_reduction(int64_t N, int64_t batch_size, int64_t C, uintptr_t addresses, int terms, double *out, void *workspace,
                              hipStream_t stream, Launch &&launch)
{
    // (not aligned: 8-byte pieces, which complex64 data always allows)
    const SpectralHead h = {(int)N, ewald_virial_far_blocks(N), (addresses & 15) == 0 ? 1 : 0, C};
    double *partial = (double *)workspace;
    launch(dim3((unsigned)(h.blocks * batch_size)), h, partial);
    NFFT_HIP_CHECK(hipGetLastError());
    return launch_virial_sum_terms(partial, terms, batch_size, C, h.blocks, nullptr, nullptr, 0, out, stream);
}

// ... of virial_far_kernel with the strain policy `strain`
template <class Strain>
int launch_virial_far(int64_t N, int64_t batch_size, int64_t num_columns, const void *band, const float *coeffs,
                      const double *box_inverse, const Strain &strain, double *out, void *workspace, hipStream_t stream)
{
    return launch_spectral_reduction(N, batch_size, num_columns, (uintptr_t)band, kVirialTerms, out, workspace, stream,
                                     [&](dim3 grid, const SpectralHead &h, double *partial) {
                                         dispatch_columns(h.C, [&](auto CC) {
                                             hipLaunchKernelGGL((virial_far_kernel<CC(), Strain>), grid, dim3(kVirialBlock), 0, stream, h,
                                                                BoxInverse(box_inverse), strain, (const float2 *)band, coeffs, partial);
                                         });
                                     });
}

// ---- one thread per (frequency, column) -------------------------------------------------------------------------------

struct SpectralElementParams {
    unsigned N, C, count;  // frequencies per axis; columns; N^3 C
    TwoPiInverse inv;
};

// the thread's frequency k (in the order of the grid), column c, cell (k with the point set blockIdx.y) and tau = 2 pi kappa
struct SpectralElement {
    unsigned k, c;
    int64_t cell;
    float3 tau;
};

// false: the thread has no element
__device__ __forceinline__ bool spectral_element(const SpectralElementParams &q, SpectralElement &el)
{
    const unsigned e = blockIdx.x * kSpectralBlock + threadIdx.x;
    if (e >= q.count) return false;
    const unsigned N = q.N, C = q.C;
    const unsigned k = e / C, c = e - k * C;
    const unsigned i2 = k % N, i01 = k / N, i1 = i01 % N, i0 = i01 / N;
    const int half = (int)(N / 2);
    const float k0 = (float)((int)i0 - half), k1 = (float)((int)i1 - half), k2 = (float)((int)i2 - half);
    el.k = k;
    el.c = c;
    el.cell = (int64_t)blockIdx.y * (q.count / C) + k;
    el.tau = q.inv.tau(k0, k1, k2);
    return true;
}

typedef void (*spectral_element_kernel)(SpectralElementParams, const float2 *, const float *, float2 *);

// `kernel` on every (frequency, column) of band [batch_size, N, N, N, .., num_columns]
inline int launch_spectral_elements(spectral_element_kernel kernel, int64_t N, int64_t batch_size, int64_t num_columns,
                                    const void *band, const float *coeffs, const double *box_inverse, void *out, hipStream_t stream)
{
    // (count < 2^31: the entry point's check)
    const SpectralElementParams q = {(unsigned)N, (unsigned)num_columns, (unsigned)(N * N * N * num_columns), TwoPiInverse(box_inverse)};
    const dim3 grid((q.count + kSpectralBlock - 1) / kSpectralBlock, (unsigned)batch_size), block(kSpectralBlock);
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, q, (const float2 *)band, coeffs, (float2 *)out);
    NFFT_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace nfft
