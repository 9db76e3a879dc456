// Buckingham / Born-Mayer-Huggins + Coulomb step with per-type-pair parameters: the pair walk of section
// 7t for force fields whose repulsion is an exponential -- Tosi-Fumi alkali halides, BKS silica, the Buckingham ceramics.
// A point carries a charge q_j, a GRID coefficient c_j and a type t_j in [0, T); a table [T, T] of (A, B, dC6, C8) holds, per
// pair of types, u(r) = A e^(-B r) - C6 / r^6 - C8 / r^8 with dC6(t, t') = C6(t, t') - g_t g_t' what the pair's C6 has above the
// product that the grid carries, c_j = g_(t_j).  The far field and the list kernel of 7s see c alone and are unchanged; with
// c = 0 (no long-range dispersion, the usual route of these force fields) cc w_D and cc mg_D are exact zeros.
//
// The walk is step_near_kernel of step_frame.h with the law below.  Per passing pair, with r = rr rsqrt(rr) as EwaldPairWeight
// has it,
//     E = A exp(-B r),   p6 = dC6 ir6,   p8 = (C8 ir6) ir2,   slope = B E ir - (6 p6 + 8 p8) ir2,   u = E - p6 - p8
// and s^L scales A, dC6 and C8.
//
// The exponential is expf, not __expf.  __expf is v_exp_f32 of the float32 product B r log2(e): that product's rounding,
// 2^-24 (B r log2 e) relative to itself, is an ABSOLUTE error of the exponent and so a relative error 6e-8 B r of E.  The
// argument is not small here as alpha^2 r^2 is in the Gaussian factors of the Ewald weights (at most 20 at the cut, where the factor
// itself is 1e-9 of the sum): B r is 12 to 15 at the pair potential's minimum, where E is as large as the attraction that
// it balances, and B r_c beyond (30 to 60 for the published alkali-halide and oxide tables at r_c of 8 to 12 Angstrom).  That
// is 7e-7 to 4e-6 of the term that dominates the close pairs' force, above the 5e-7 that the whole walk of 7t shows.  expf
// reduces the argument with a compensated product and keeps 1 ulp for every B r; it costs about ten more VALU operations
// per passing pair and no register that the kernel's occupancy notices (the table below).  YukawaPairWeight made the same choice
// for e^(-lambda r) on the same ground.  Beyond B r = 87.3 the exponential leaves the normal range and below 103.9 it is
// flushed to zero, as it should be.
//
// The table in LDS.  An entry has 16 bytes, and 7t's bank argument does not carry over to one 16-byte read: ds_read_b128 is
// served in four groups of 16 lanes, each over the 16 sixteen-byte slots of the 64 banks, so a group's slots are
// (t_i S + t_j) mod 16, t_j the same in every lane; with S = T | 1 odd, types that differ by 16 meet in one slot.  A float4 table
// is conflict-free for T <= 16 only and 2-way above: 4 LDS cycles, 8 at T = 32 with mixed types.  Chosen instead: TWO float2
// PLANES, (A, B) and (dC6, C8), each [T][S] with rows S = T | 1 entries apart and the second plane T S entries after the first.
// A ds_read_b64 is served in two halves of 32 lanes over 32 eight-byte slots, a half's slots are (t_i S + t_j) mod 32, and S odd
// makes t_i -> t_i S mod 32 a bijection on [0, 32): the up to 32 rows of a half wave fall on 32 different slots, no conflict
// for any T <= 32 and any mix of types (7t's arithmetic, unchanged; lanes of one type read one address, a broadcast).  Two reads
// of 2 cycles each: the 4 cycles of the conflict-free float4 read at every T, never its 8.  The price is one more LDS
// instruction and one address addition per passing pair.  This is arithmetic on the documented bank structure: NO CONFLICT
// COUNTER WAS READ.  The planes take 16 T S bytes of dynamic LDS (T = 32: 16 896) and are filled once per workgroup with one
// 16-byte global load per entry: `table` is 16-byte aligned, which the entry point checks.
//
// The smallest separation.  Each coefficient is multiplied in before the powers meet.  What must stay below 3.4e38: r^-8
// (r > 1.6e-5, the dispersion weight of 7j), 6 |dC6| r^-8 (r > 1.9e-5 |dC6|^(1/8)) and 8 C8 r^-10 (r > 1.8e-4 C8^(1/10)).
// The exponential term is finite everywhere, A at most.  Below those separations: not numbers.  Long before, at the maximum of
// A e^(-B r) - C6 / r^6 (the Buckingham turnover), the model itself turns attractive without bound; nothing here guards it.
#include "step_frame.h"

namespace nfft {

namespace {

// two planes [T][S] of float2: (A, B), then (dC6, C8)
struct BmhTableLaw : TableLaw<float4> {
    struct Coef {
        float a, b, dc6, c8;
        __device__ __forceinline__ void scale(float sl)
        {
            a *= sl;
            dc6 *= sl;
            c8 *= sl;
        }
        __device__ __forceinline__ void terms(const EwaldPairWeight &e, const DispersionPairWeight &w6, float &slope, float &u) const
        {
            const float E = a * expf(-b * (e.rr * e.ir));  // A e^(-B r): expf, see the header
            const float p6 = dc6 * w6.ir6;                 // the coefficients go in first
            const float p8 = (c8 * w6.ir6) * w6.ir2;
            slope = fmaf(b * E, e.ir, -fmaf(8.f, p8, 6.f * p6) * w6.ir2);
            u = E - p6 - p8;
        }
    };
    int plane;
    // (one 16-byte load per entry)
    __device__ __forceinline__ BmhTableLaw(const Params &p)
        : TableLaw(p, [plane = p.T * p.S](float2 *s, int at, float4 v) {
              s[at] = make_float2(v.x, v.y);
              s[plane + at] = make_float2(v.z, v.w);
          }),
          plane(p.T * p.S)
    {
    }
    __device__ __forceinline__ Coef coef(Own tiS, const float4 &v) const
    {
        const int at = tiS + __float_as_int(v.z);
        const float2 ab = s_tab[at];          // (A, B) of the two types
        const float2 cd = s_tab[plane + at];  // (dC6, C8)
        return {ab.x, ab.y, cd.x, cd.y};
    }
};

}  // namespace

int launch_ewald_bmh_table_near(const nfft_hip_ewald_box_problem *p, double alpha_dispersion, int64_t num_types, int64_t num_entries,
                                const float *pos, const float *xs, const int *types, const float *table, const int *start,
                                const int64_t *index, const int *row_start, const int *col, const float *weight_coulomb,
                                const float *weight_lj, float *f, double *out, void *workspace, hipStream_t stream)
{
    if (num_types < 1 || num_types > kMaxTypes) return NFFT_HIP_EINVAL;  // (the entry point has said why)
    const BmhTableLaw::Params tt = {types, (const float4 *)table, (int)num_types, (int)num_types | 1};
    return launch_step_near<BmhTableLaw>(p, alpha_dispersion, tt, (size_t)2 * tt.T * tt.S * sizeof(float2), num_entries, pos, xs,
                                         start, index, row_start, col, weight_coulomb, weight_lj, f, out, workspace, stream);
}

}  // namespace nfft
