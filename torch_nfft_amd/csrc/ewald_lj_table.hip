// Lennard-Jones + Coulomb step with per-type-pair parameters: the pair walk of sections 7r and 7s for
// force fields whose C6_ij and C12_ij are not products of per-point numbers (Lorentz-Berthelot mixing, fitted cross terms).
// A point carries a charge q_j, a GRID coefficient c_j and a type t_j in [0, T); a table [T, T] of (C12, dC6) holds, per pair
// of types, the repulsion coefficient and what the pair's C6 has above the product that the grid carries,
// dC6(t, t') = C6(t, t') - g_t g_t' with c_j = g_(t_j).  The far field and the list kernel of 7s see c alone and are unchanged:
// inside r_c a pair interacts with its exact C6_ij, beyond with c_i c_j.
//
// The walk is step_near_kernel of step_frame.h with the law below.  The table is loaded once per workgroup (one 8-byte load
// per entry: `table` is 8-byte aligned, which the entry point checks) into dynamic LDS as float2 (C12, dC6): 8 T S bytes with
// S = T | 1 (T = 32: 8448).  A passing pair takes one 8-byte LDS read at t_i S + t_j.  t_j is the same in every lane and t_i
// is not: the read is data-dependent, its banks are 2 (t_i S + t_j) mod 64 within a half wave, and with S odd the up to 32
// rows of a half wave fall on 32 different bank pairs -- no conflict for any mix of types, where S = T = 32 would put every
// row on ONE bank pair (32-way).  Lanes of one type read one address (a broadcast).  Per passing pair
//     p12 = (C12 ir6) ir6,   p6 = dC6 ir6,   slope = 12 (C12 ir6) (ir6 ir2) - 6 p6 ir2,   u = p12 - p6
// and s^L scales C12 and dC6.
//
// The smallest separation.  The coefficient is multiplied in before the powers meet, so what must stay below 3.4e38 are
// r^-8 (r > 1.6e-5, as for the dispersion weight of 7j), C12 r^-6, 6 |dC6| r^-8 (r > 1.9e-5 |dC6|^(1/8)) and the slope itself,
// 12 C12 r^-14: r > 2.1e-3 C12^(1/14), e.g. 1.2e-4 at C12 = 2e-18 (sigma = 0.03, epsilon = 1).  Below that: not numbers.
#include "step_frame.h"

namespace nfft {

namespace {

struct LjTableLaw : TableLaw<float2> {
    struct Coef {
        float c12, dc6;
        __device__ __forceinline__ void scale(float sl)
        {
            c12 *= sl;
            dc6 *= sl;
        }
        __device__ __forceinline__ void terms(const EwaldPairWeight &, const DispersionPairWeight &w6, float &slope, float &u) const
        {
            const float a6 = c12 * w6.ir6;  // C12 / r^6: the coefficient goes in first
            const float p12 = a6 * w6.ir6, p6 = dc6 * w6.ir6;
            slope = fmaf(12.f * a6, w6.ir6 * w6.ir2, -6.f * p6 * w6.ir2);
            u = p12 - p6;
        }
    };
    __device__ __forceinline__ LjTableLaw(const Params &p) : TableLaw(p, [](float2 *s, int at, float2 v) { s[at] = v; }) {}
    __device__ __forceinline__ Coef coef(Own tiS, const float4 &v) const
    {
        const float2 tab = s_tab[tiS + __float_as_int(v.z)];  // (C12, dC6) of the two types
        return {tab.x, tab.y};
    }
};

}  // namespace

int launch_ewald_lj_table_near(const nfft_hip_ewald_box_problem *p, double alpha_dispersion, int64_t num_types, int64_t num_entries,
                               const float *pos, const float *xs, const int *types, const float *table, const int *start,
                               const int64_t *index, const int *row_start, const int *col, const float *weight_coulomb,
                               const float *weight_lj, float *f, double *out, void *workspace, hipStream_t stream)
{
    if (num_types < 1 || num_types > kMaxTypes) return NFFT_HIP_EINVAL;  // (the entry point has said why)
    const LjTableLaw::Params tt = {types, (const float2 *)table, (int)num_types, (int)num_types | 1};
    return launch_step_near<LjTableLaw>(p, alpha_dispersion, tt, (size_t)tt.T * tt.S * sizeof(float2), num_entries, pos, xs, start,
                                        index, row_start, col, weight_coulomb, weight_lj, f, out, workspace, stream);
}

}  // namespace nfft
