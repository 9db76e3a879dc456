// Nonbonded step of a Lennard-Jones + Coulomb model: forces, the two energies and the virial tensor of
//
//     U = U_C + U_LJ,   U_C  = the Ewald sum of q_i q_j / r            (sections 7g to 7i, 7q),
//                       U_LJ = 1/2 sum_ij a_i a_j / r^12 [r < r_c]  -  the Ewald sum of c_i c_j / r^6   (sections 7j, 7k)
//
// (geometric mixing for both powers: C12_ij = a_i a_j, C6_ij = c_i c_j) from one walk over the pairs and one pass over the
// spectrum, where the Coulomb step, the dispersion sweep and the dispersion virial walk the pairs three times and read the
// spectrum twice.  The repulsion is plainly truncated at r_c and has no spectral part.
//
// The pair walk is step_near_kernel of step_frame.h with the PRODUCT LAW below, u = a_i a_j / r^12: the streamed values of a
// point are (q_j, c_j, a_j) packed as xs [n, 3].  Without a list they are staged by StageColumns<4> with its zero pad and no
// index is read per staged point; with one (the list kernel is in ewald_lj_excl.hip) StageLjIndexed puts
// the streamed point's caller-order index, as integer bits, in the pad's place.  From the reciprocal that the dispersion
// weight forms, p = (a_i r^-6) (a_j r^-6) = a_i a_j / r^12 and the slope is 12 p / r^2; s^L scales a_j.
//
// lj_step_spectral_kernel  ewald_step_spectral_kernel's thread-to-cell mapping and carried index digits on band [B, N, N, N, 2]
//                          = the adjoint transform of (q, c): writes the six spectra i tau_a b^C S^q and i tau_a b^D S^c
//                          (zeros where the table is zero) and sums, in float64, 1/2 b^C |S^q|^2, -1/2 b^D |S^c|^2 and the
//                          six virial terms -- the Coulomb weights of section 7i minus the dispersion weights of section 7k.
//                          One partial [8] per workgroup.
//
// The smallest separation: the dispersion weight's r^-8 leaves float32 below r ~ 1.6e-5 whatever the coefficients are (and
// 0 * inf is not a number), and the repulsion's slope, formed as (a_i r^-6) (a_j r^-6) r^-2 so that the coefficients keep it
// in range, stays finite while 12 a_i a_j / r^14 < 3.4e38: r > 1.8e-3 (a_i a_j)^(1/14), e.g. 9e-5 at a = 1e-9 (sigma = 0.03).
//
// The second level of both is launch_virial_sum_terms of ewald_virial.hip with eight terms.  No atomics anywhere and every
// order of addition is fixed by the launch geometry: two calls give the same bits.
#include "step_frame.h"

namespace nfft {

namespace {

constexpr int kLjTerms = kStepTerms;
constexpr int kVirialBlock = 256;  // lanes of the spectral kernel (and of the second level in ewald_virial.hip)

// staging policy: (q_j, c_j, a_j) of xs [n, 3] and the caller-order index of the streamed point as integer bits
struct StageLjIndexed {
    float *s_x;
    const float *__restrict__ xs;
    const int64_t *__restrict__ index;
    __device__ __forceinline__ void point(int j, int64_t i) const
    {
        const float *xp = xs + i * 3;
        s_x[j * 4 + 0] = xp[0];
        s_x[j * 4 + 1] = xp[1];
        s_x[j * 4 + 2] = xp[2];
        s_x[j * 4 + 3] = __int_as_float((int)index[i]);
    }
};

// the product law (step_frame.h has what a law is): C12_ij = a_i a_j, no table and no block
struct LjProductLaw {
    static constexpr int kValues = 3;  // q, c, a
    struct Params {};
    typedef float Own;  // a_i
    struct Coef {
        float ai, aj;
        __device__ __forceinline__ void scale(float sl) { aj *= sl; }
        __device__ __forceinline__ void terms(const EwaldPairWeight &, const DispersionPairWeight &w6, float &slope, float &u) const
        {
            const float p = (ai * w6.ir6) * (aj * w6.ir6);  // (s^L) a_i a_j / r^12
            slope = 12.f * p * w6.ir2;
            u = p;
        }
    };
    __device__ __forceinline__ LjProductLaw(const Params &) {}
    template <bool MASKED>
    __device__ __forceinline__ auto stage(float *s_x, const float *xs, const int64_t *index) const
    {
        if constexpr (MASKED) return StageLjIndexed{s_x, xs, index};
        else return StageColumns<4>{s_x, xs, kValues, 0};
    }
    __device__ __forceinline__ Own own(const float *xp, int) const { return xp[2]; }
    __device__ __forceinline__ Coef coef(Own ai, const float4 &v) const { return {ai, v.z}; }
};

struct LjSpectralParams {
    int N, blocks;  // frequencies per axis; workgroups per point set
    int wide;       // band and spectra are 16-byte aligned: a cell moves as one 16-byte load and three 16-byte stores
    double i00, i10, i11, i20, i21, i22;  // the lower triangle of A^-1
    double p2a2;                          // pi^2 / alpha_C^2
    float t00, t10, t11, t20, t21, t22;   // 2 pi times the lower triangle of A^-1
};

// (x + i y) times the imaginary i t
__device__ __forceinline__ float2 times_i(float t, float2 r) { return make_float2(-t * r.y, t * r.x); }

__global__ void __launch_bounds__(kVirialBlock) lj_step_spectral_kernel(LjSpectralParams q, const float2 *__restrict__ band,
                                                                        const float *__restrict__ coeffs_c,
                                                                        const float *__restrict__ coeffs_d,
                                                                        const float *__restrict__ strain_d,
                                                                        float2 *__restrict__ spectra, double *__restrict__ partial)
{
    __shared__ double s_red[kVirialBlock / 64][kLjTerms];
    const int tid = threadIdx.x;
    const int N = q.N, half = q.N / 2;
    const int64_t cells = (int64_t)N * N * N;
    const int set = blockIdx.x / q.blocks, blk = blockIdx.x % q.blocks;  // (point set, workgroup within it)
    const float2 *bb = band + (int64_t)set * cells * 2;
    float2 *ss = spectra + (int64_t)set * cells * 6;
    double acc[kLjTerms];
#pragma unroll
    for (int n = 0; n < kLjTerms; ++n) acc[n] = 0.0;
    // the cells blk * 256 + tid, + stride, + 2 stride, ...: their index (i0, i1, i2) is kept beside them and advanced
    // by the stride's own digits with carries, so that no division runs per cell
    const int stride = q.blocks * kVirialBlock;
    const unsigned first = (unsigned)blk * kVirialBlock + tid;
    int i2 = (int)(first % (unsigned)N), i1 = (int)((first / (unsigned)N) % (unsigned)N), i0 = (int)(first / ((unsigned)N * N));
    const int s2 = stride % N, s1 = (stride / N) % N, s0 = stride / (N * N);
    for (int64_t cell = first; cell < cells; cell += stride) {
        const float bc = coeffs_c[cell], bd = coeffs_d[cell];
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
        const float2 *bp = bb + cell * 2;
        float2 *sp = ss + cell * 6;
        float2 sq, sc;  // S^q_k, S^c_k
        if (q.wide) {   // (16 bytes per cell, aligned: one load)
            const float4 u = *reinterpret_cast<const float4 *>(bp);
            sq = make_float2(u.x, u.y);
            sc = make_float2(u.z, u.w);
        } else {
            sq = bp[0];
            sc = bp[1];
        }
        // the six spectra: i tau_a R with R = b_k S_k and tau = 2 pi kappa in float32.  A zero in a table (k = 0 for the
        // Coulomb one, the zeroed planes k_a = -N/2 for both) gives zeros, whatever band holds there
        const float kf0 = (float)k0, kf1 = (float)k1, kf2 = (float)k2;
        const float tx = q.t00 * kf0;
        const float ty = fmaf(q.t11, kf1, q.t10 * kf0);
        const float tz = fmaf(q.t22, kf2, fmaf(q.t21, kf1, q.t20 * kf0));
        const float2 zero = make_float2(0.f, 0.f);
        const float2 Rq = bc == 0.f ? zero : make_float2(bc * sq.x, bc * sq.y);
        const float2 Rc = bd == 0.f ? zero : make_float2(bd * sc.x, bd * sc.y);
        const float2 o0 = times_i(tx, Rq), o1 = times_i(ty, Rq), o2 = times_i(tz, Rq);
        const float2 o3 = times_i(tx, Rc), o4 = times_i(ty, Rc), o5 = times_i(tz, Rc);
        if (q.wide) {  // (48 bytes per cell, aligned: three stores)
            float4 *sp4 = reinterpret_cast<float4 *>(sp);
            sp4[0] = make_float4(o0.x, o0.y, o1.x, o1.y);
            sp4[1] = make_float4(o2.x, o2.y, o3.x, o3.y);
            sp4[2] = make_float4(o4.x, o4.y, o5.x, o5.y);
        } else {
            sp[0] = o0;
            sp[1] = o1;
            sp[2] = o2;
            sp[3] = o3;
            sp[4] = o4;
            sp[5] = o5;
        }
        if (bc == 0.f && bd == 0.f) continue;
        // kappa = A^-1 k, A^-1 lower triangular
        const double kx = q.i00 * k0;
        const double ky = q.i10 * k0 + q.i11 * k1;
        const double kz = q.i20 * k0 + q.i21 * k1 + q.i22 * k2;
        if (bc != 0.f) {  // (not k = 0: kappa^2 > 0)
            const double kk = kx * kx + ky * ky + kz * kz;
            const double b = (double)bc;
            const double t = -2.0 * (1.0 / kk + q.p2a2) * b;
            const double p = (double)sq.x * (double)sq.x + (double)sq.y * (double)sq.y;
            acc[0] += b * p;
            acc[2] += (b + t * kx * kx) * p;
            acc[3] += (b + t * ky * ky) * p;
            acc[4] += (b + t * kz * kz) * p;
            acc[5] += (t * ky * kz) * p;
            acc[6] += (t * kx * kz) * p;
            acc[7] += (t * kx * ky) * p;
        }
        if (bd != 0.f) {  // (k = 0 counts: t_0 is finite and multiplies kappa kappa = 0)
            const double b = (double)bd;
            const double t = (double)strain_d[cell];
            const double p = (double)sc.x * (double)sc.x + (double)sc.y * (double)sc.y;
            acc[1] -= b * p;
            acc[2] -= (b + t * kx * kx) * p;
            acc[3] -= (b + t * ky * ky) * p;
            acc[4] -= (b + t * kz * kz) * p;
            acc[5] -= (t * ky * kz) * p;
            acc[6] -= (t * kx * kz) * p;
            acc[7] -= (t * kx * ky) * p;
        }
    }
    const double v = block_sum_f64(acc, s_red);
    if (tid < kLjTerms) partial[(int64_t)blockIdx.x * kLjTerms + tid] = 0.5 * v;
}

}  // namespace

// the workspace of every step walk: the work items, then (256-byte aligned, where ewald_virial_near_partials points) one
// partial [8] per item slot
int64_t ewald_step8_near_workspace(const nfft_hip_ewald_box_problem *p)
{
    const int64_t slots = ewald_virial_near_item_slots(p);
    return round256(slots * (int64_t)sizeof(int2)) + slots * kStepTerms * (int64_t)sizeof(double);
}

int64_t ewald_lj_step_spectral_workspace(int64_t N, int64_t batch_size)
{
    return batch_size * ewald_virial_far_blocks(N) * kLjTerms * (int64_t)sizeof(double);
}

// (the unit cube runs as the identity box, as the Coulomb step does; no types and no table)
int launch_ewald_lj_step_near(const nfft_hip_ewald_box_problem *p, double alpha_dispersion, int64_t, int64_t num_entries,
                              const float *pos, const float *xs, const int *, const float *, const int *start, const int64_t *index,
                              const int *row_start, const int *col, const float *weight_coulomb, const float *weight_lj, float *f,
                              double *out, void *workspace, hipStream_t stream)
{
    return launch_step_near<LjProductLaw>(p, alpha_dispersion, {}, 0, num_entries, pos, xs, start, index, row_start, col,
                                          weight_coulomb, weight_lj, f, out, workspace, stream);
}

int launch_ewald_lj_step_spectral(int64_t N, int64_t batch_size, const void *band, const float *coeffs_coulomb,
                                  const float *coeffs_dispersion, const float *strain_dispersion, const double *box_inverse,
                                  double pi2_over_alpha2, void *spectra, double *out, void *workspace, hipStream_t stream)
{
    const double two_pi = 6.28318530717958647692;
    LjSpectralParams q;
    q.N = (int)N;
    q.blocks = ewald_virial_far_blocks(N);
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
    hipLaunchKernelGGL(lj_step_spectral_kernel, dim3((unsigned)(q.blocks * batch_size)), dim3(kVirialBlock), 0, stream, q,
                       (const float2 *)band, coeffs_coulomb, coeffs_dispersion, strain_dispersion, (float2 *)spectra, partial);
    NFFT_HIP_CHECK(hipGetLastError());
    return launch_virial_sum_terms(partial, kLjTerms, batch_size, 1, q.blocks, nullptr, nullptr, 0, out, stream);
}

}  // namespace nfft
