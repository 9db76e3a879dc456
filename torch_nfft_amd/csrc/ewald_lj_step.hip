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
// lj_step_spectral_kernel  written from the pieces of spectral_frame.h: ewald_step_spectral_kernel's
//                          sweep, load and tau on band [B, N, N, N, 2] = the adjoint transform of (q, c): writes the six
//                          spectra i tau_a b^C S^q and i tau_a b^D S^c (zeros where the table is zero) and sums, in float64, 1/2 b^C |S^q|^2, -1/2 b^D |S^c|^2 and the
//                          six virial terms -- the Coulomb weights of section 7i minus the dispersion weights of section 7k.
//                          One partial [8] per workgroup.
//
// The smallest separation: the dispersion weight's r^-8 leaves float32 below r ~ 1.6e-5 whatever the coefficients are (and
// 0 * inf is not a number), and the repulsion's slope, formed as (a_i r^-6) (a_j r^-6) r^-2 so that the coefficients keep it
// in range, stays finite while 12 a_i a_j / r^14 < 3.4e38: r > 1.8e-3 (a_i a_j)^(1/14), e.g. 9e-5 at a = 1e-9 (sigma = 0.03).
//
// The second level of both is launch_virial_sum_terms of ewald_virial.hip with eight terms.  No atomics anywhere and every
// order of addition is fixed by the launch geometry: two calls give the same bits.
#include "spectral_frame.h"
#include "step_frame.h"

namespace nfft {

namespace {

constexpr int kLjTerms = kStepTerms;

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

__global__ void __launch_bounds__(kVirialBlock) lj_step_spectral_kernel(SpectralHead h, BoxInverse inv, CoulombStrain strain_c,
                                                                        TwoPiInverse tpi, const float2 *__restrict__ band,
                                                                        const float *__restrict__ coeffs_c,
                                                                        const float *__restrict__ coeffs_d,
                                                                        const float *__restrict__ strain_d,
                                                                        float2 *__restrict__ spectra, double *__restrict__ partial)
{
    __shared__ double s_red[kVirialBlock / 64][kLjTerms];
    const int64_t cells = (int64_t)h.N * h.N * h.N;
    const int set = blockIdx.x / h.blocks;  // (the workgroup's point set)
    const float2 *bb = band + (int64_t)set * cells * 2;
    float2 *ss = spectra + (int64_t)set * cells * 6;
    double acc[kLjTerms];
#pragma unroll
    for (int n = 0; n < kLjTerms; ++n) acc[n] = 0.0;
    for (CellSweep sweep(h.N, h.blocks); sweep.more(); sweep.advance()) {
        const int64_t cell = sweep.cell;
        const float bc = coeffs_c[cell], bd = coeffs_d[cell];
        int k0, k1, k2;
        sweep.frequency(k0, k1, k2);
        float2 *sp = ss + cell * 6;
        float2 s[2];  // S^q_k, S^c_k (16 bytes per cell: one load where aligned)
        load_cell<2>(bb + cell * 2, 2, 0, h.wide, s);
        const float2 sq = s[0], sc = s[1];
        // the six spectra: i tau_a R with R = b_k S_k and tau = 2 pi kappa in float32.  A zero in a table (k = 0 for the
        // Coulomb one, the zeroed planes k_a = -N/2 for both) gives zeros, whatever band holds there
        const float3 tau = tpi.tau((float)k0, (float)k1, (float)k2);
        const float2 zero = make_float2(0.f, 0.f);
        const float2 Rq = bc == 0.f ? zero : make_float2(bc * sq.x, bc * sq.y);
        const float2 Rc = bd == 0.f ? zero : make_float2(bd * sc.x, bd * sc.y);
        const float2 o0 = times_i(tau.x, Rq), o1 = times_i(tau.y, Rq), o2 = times_i(tau.z, Rq);
        const float2 o3 = times_i(tau.x, Rc), o4 = times_i(tau.y, Rc), o5 = times_i(tau.z, Rc);
        if (h.wide) {  // (48 bytes per cell, aligned: three stores)
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
        // (the seven weights of strain_weights, each multiplied in where it is formed: kept in an array of their own first,
        // as the other reductions have them, they cost this kernel two VGPRs)
        const double3 kap = inv.kappa(k0, k1, k2);
        const double kx = kap.x, ky = kap.y, kz = kap.z;
        if (bc != 0.f) {  // (not k = 0: kappa^2 > 0)
            const double b = (double)bc;
            const double t = strain_c(cell, b, kx, ky, kz);
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
    block_sums_to_partial<kLjTerms, 1>(acc, s_red, 0.5, 1, 0, partial);
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
    // (one column of eight sums)
    return launch_spectral_reduction(
        N, batch_size, 1, (uintptr_t)band | (uintptr_t)spectra, kLjTerms, out, workspace, stream,
        [&](dim3 grid, const SpectralHead &h, double *partial) {
            hipLaunchKernelGGL(lj_step_spectral_kernel, grid, dim3(kVirialBlock), 0, stream, h, BoxInverse(box_inverse),
                               CoulombStrain{pi2_over_alpha2}, TwoPiInverse(box_inverse), (const float2 *)band, coeffs_coulomb,
                               coeffs_dispersion, strain_dispersion, (float2 *)spectra, partial);
        });
}

}  // namespace nfft
