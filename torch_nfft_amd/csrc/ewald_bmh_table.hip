// Buckingham / Born-Mayer-Huggins + Coulomb step with per-type-pair parameters: the pair walk of section
// 7t for force fields whose repulsion is an exponential -- Tosi-Fumi alkali halides, BKS silica, the Buckingham ceramics.
// A point carries a charge q_j, a GRID coefficient c_j and a type t_j in [0, T); a table [T, T] of (A, B, dC6, C8) holds, per
// pair of types, u(r) = A e^(-B r) - C6 / r^6 - C8 / r^8 with dC6(t, t') = C6(t, t') - g_t g_t' what the pair's C6 has above the
// product that the grid carries, c_j = g_(t_j).  The far field and the list kernel of 7s see c alone and are unchanged; with
// c = 0 (no long-range dispersion, the usual route of these force fields) cc w_D and cc mg_D are exact zeros.
//
// bmh_table_near_kernel<MASKED>  lj_table_near_kernel<MASKED>'s items, lanes, walk, tiles, image, test 0 < rr < rc2, staging of
//                        (q_j, c_j, clamped type bits, caller index bits) in one float4, eleven float32 sums and epilogue;
//                        8320 bytes of static LDS as before.  Per passing pair, with r = rr rsqrt(rr) as EwaldPairWeight has it,
//                            E = A exp(-B r),   p6 = dC6 ir6,   p8 = (C8 ir6) ir2,
//                            slope = B E ir - (6 p6 + 8 p8) ir2,
//                            s = qq mg_C - cc mg_D + slope,   energies qq w_C and E - p6 - p8 - cc w_D.
//                        MASKED adds 7s's interval test and find_in_row on the lane's CSR row: on a hit qq is scaled by s^C
//                        and cc, A, dC6, C8 by s^L; a pair with both scales zero returns before any weight is formed.  The
//                        unmasked instantiation holds none of that code and reads no list.  With an empty list the masked
//                        one gives the unmasked bits.
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
//
// The second level is launch_virial_sum_terms of ewald_virial.hip with eight terms.  No atomics anywhere and every order of
// addition is fixed by the launch geometry: two calls give the same bits.
#include "pair_frame.h"

namespace nfft {

namespace {

constexpr int kBmhTerms = 8;    // U_C, U_sr, xx, yy, zz, yz, xz, xy
constexpr int kBmhSums = 11;    // s d_x, d_y, d_z; s d_a d_b in the order of the virial's terms; the two energies
constexpr int kBmhValues = 2;   // q, c
constexpr int kMaxTypes = 32;   // T at most: 16 T (T | 1) = 16896 bytes of LDS

// the CSR list on the device (MASKED only)
struct ExclList {
    const int *__restrict__ row_start;
    const int *__restrict__ col;
    const float *__restrict__ wc;
    const float *__restrict__ wl;
    int n, entries;
};

// the types and their table
struct TypeTable {
    const int *__restrict__ types;     // [n] in cell order
    const float4 *__restrict__ table;  // [T, T]: (A, B, dC6, C8), 16-byte aligned
    int T, S;                          // types; entries between two rows of a plane in LDS, T | 1
};

__device__ __forceinline__ int clamp_type(int t, int T) { return min(max(t, 0), T - 1); }

// staging policy: (q_j, c_j) of xs [n, 2], then the clamped type and the caller-order index of the streamed point as bits
struct StageTyped {
    float *s_x;
    const float *__restrict__ xs;
    const int *__restrict__ types;
    const int64_t *__restrict__ index;
    int T;
    __device__ __forceinline__ void point(int j, int64_t i) const
    {
        const float *xp = xs + i * kBmhValues;
        s_x[j * 4 + 0] = xp[0];
        s_x[j * 4 + 1] = xp[1];
        s_x[j * 4 + 2] = __int_as_float(clamp_type(types[i], T));
        s_x[j * 4 + 3] = __int_as_float((int)index[i]);
    }
};

// the entry of the ascending row [first, last) whose column is j, or -1
__device__ __forceinline__ int find_in_row(const int *__restrict__ col, int first, int last, int j)
{
    while (first < last) {
        const int mid = first + ((last - first) >> 1);
        const int c = col[mid];
        if (c == j) return mid;
        if (c < j) first = mid + 1;
        else last = mid;
    }
    return -1;
}

template <bool MASKED>
__global__ void __launch_bounds__(kNearBlock) bmh_table_near_kernel(EwaldPairParams qc, EwaldPairParams qd, TypeTable tt, ExclList ex,
                                                                    const int2 *__restrict__ items, const float *__restrict__ pos,
                                                                    const float *__restrict__ xs, const int *__restrict__ start,
                                                                    const int64_t *__restrict__ index, float *__restrict__ f,
                                                                    double *__restrict__ partial)
{
    __shared__ float4 s_pos[kNearTile];
    __shared__ __attribute__((aligned(16))) float s_x[kNearTile * 4];
    __shared__ double s_red[kNearBlock / 64][kBmhTerms];
    extern __shared__ float2 s_tab[];  // two planes [T][S]: (A, B), then (dC6, C8); rows by the lane's type
    const int2 item = items[blockIdx.x];
    if (item.x < 0) return;  // (uniform: an empty slot; the second level skips it)
    const int plane = tt.T * tt.S;
    // (32 lanes per row, T <= 32 of them with an entry: no division, one 16-byte load per entry)
    for (int k = threadIdx.x; k < tt.T * kMaxTypes; k += kNearBlock) {
        const int row = k / kMaxTypes, col = k % kMaxTypes;
        if (col < tt.T) {
            const float4 v = tt.table[row * tt.T + col];
            s_tab[row * tt.S + col] = make_float2(v.x, v.y);
            s_tab[plane + row * tt.S + col] = make_float2(v.z, v.w);
        }
    }
    __syncthreads();
    const PairLane lane = pair_lane(item, start);
    const WrappedWalk walk(lane.cell, qc.G0, qc.G1, qc.G2);
    // (a lane without a target sums pairs of the origin with zero parameters and type 0; it stores nothing)
    const float4 t = lane_position(lane, pos, 3, 0.f);
    float qi = 0.f, ci = 0.f;
    int tiS = 0;
    int64_t gi = 0;
    int row0 = 0, row1 = 0, lo = 1, hi = 0;  // (no row: an empty interval)
    if (lane.active) {
        const float *xp = xs + (int64_t)lane.ti * kBmhValues;
        qi = xp[0];
        ci = xp[1];
        tiS = clamp_type(tt.types[lane.ti], tt.T) * tt.S;
        gi = index[lane.ti];
        if (MASKED && gi >= 0 && gi < ex.n) {
            row0 = max(ex.row_start[gi], 0);
            row1 = min(ex.row_start[gi + 1], ex.entries);
            if (row0 < row1) {
                lo = ex.col[row0];
                hi = ex.col[row1 - 1];
            }
        }
    }
    float acc[kBmhSums];
#pragma unroll
    for (int e = 0; e < kBmhSums; ++e) acc[e] = 0.f;
    const StageTyped stage = {s_x, xs, tt.types, index, tt.T};
    walk(start, [&](int first, int last) {
        sweep_range<2>(first, last, lane, s_pos, pos, 3, stage, [&](int j) {
            const PairSep d = ewald_image<true>(t, s_pos[j], qc);
            // the lanes that fail the test sit the expansion out
            if (!(d.rr > 0.f && d.rr < qc.rc2)) return;
            const float4 v = *reinterpret_cast<const float4 *>(s_x + j * 4);  // (q_j, c_j, the type's bits, the index's bits)
            const int at = tiS + __float_as_int(v.z);
            const float2 ab = s_tab[at];          // (A, B) of the two types
            const float2 cd = s_tab[plane + at];  // (dC6, C8)
            float qq = qi * v.x, cc = ci * v.y, a = ab.x, dc6 = cd.x, c8 = cd.y;
            if (MASKED) {
                const int jg = __float_as_int(v.w);
                if (jg >= lo && jg <= hi) {
                    const int k = find_in_row(ex.col, row0, row1, jg);
                    if (k >= 0) {
                        const float sc = 1.f - ex.wc[k], sl = 1.f - ex.wl[k];
                        if (sc == 0.f && sl == 0.f) return;  // fully excluded: nothing is formed
                        qq *= sc;
                        cc *= sl;
                        a *= sl;
                        dc6 *= sl;
                        c8 *= sl;
                    }
                }
            }
            const EwaldPairWeight e(d.rr, qc);
            const DispersionPairWeight w6(d.rr, qd);
            const float E = a * expf(-ab.y * (e.rr * e.ir));  // A e^(-B r): expf, see the header
            const float p6 = dc6 * w6.ir6;                    // the coefficients go in first
            const float p8 = (c8 * w6.ir6) * w6.ir2;
            const float slope = fmaf(ab.y * E, e.ir, -fmaf(8.f, p8, 6.f * p6) * w6.ir2);
            const float s = fmaf(qq, e.mg(qc), fmaf(-cc, w6.mg(), slope));
            const float gx = s * d.dx, gy = s * d.dy, gz = s * d.dz;
            acc[0] += gx;
            acc[1] += gy;
            acc[2] += gz;
            acc[3] += gx * d.dx;
            acc[4] += gy * d.dy;
            acc[5] += gz * d.dz;
            acc[6] += gy * d.dz;
            acc[7] += gx * d.dz;
            acc[8] += gx * d.dy;
            acc[9] += qq * e.w;
            acc[10] += fmaf(-cc, w6.w, E - p6 - p8);
        });
    });
    if (lane.active) {
        float *fp = f + gi * 3;
        fp[0] = acc[0];
        fp[1] = acc[1];
        fp[2] = acc[2];
    }
    // every pair is seen from both ends: halved, float64 from here on; a lane without a target adds exactly zero
    double red[kBmhTerms];
    red[0] = lane.active ? 0.5 * (double)acc[9] : 0.0;
    red[1] = lane.active ? 0.5 * (double)acc[10] : 0.0;
#pragma unroll
    for (int e = 0; e < 6; ++e) red[2 + e] = lane.active ? 0.5 * (double)acc[3 + e] : 0.0;
    const double v = block_sum_f64(red, s_red);
    const int tid = threadIdx.x;
    if (tid < kBmhTerms) partial[(int64_t)blockIdx.x * kBmhTerms + tid] = v;
}

int64_t round256(int64_t bytes) { return (bytes + 255) & ~int64_t(255); }

}  // namespace

// the workspace is that of the walks of 7r, 7s and 7t: the work items, then one partial [8] per item slot
int64_t ewald_bmh_table_near_workspace(const nfft_hip_ewald_box_problem *p)
{
    const int64_t slots = ewald_virial_near_item_slots(p);
    return round256(slots * (int64_t)sizeof(int2)) + slots * kBmhTerms * (int64_t)sizeof(double);
}

// row_start == nullptr: no list, the unmasked instantiation
int launch_ewald_bmh_table_near(const nfft_hip_ewald_box_problem *p, double alpha_dispersion, int64_t num_types, int64_t num_entries,
                                const float *pos, const float *xs, const int *types, const float *table, const int *start,
                                const int64_t *index, const int *row_start, const int *col, const float *weight_coulomb,
                                const float *weight_lj, float *f, double *out, void *workspace, hipStream_t stream)
{
    if (num_types < 1 || num_types > kMaxTypes) return NFFT_HIP_EINVAL;  // (the entry point has said why)
    const EwaldPairParams qc = ewald_pair_params(p->cells[0], p->cells[1], p->cells[2], kBmhValues, p->alpha, p->r_cut, p->box);
    const EwaldPairParams qd = ewald_pair_params(p->cells[0], p->cells[1], p->cells[2], kBmhValues, alpha_dispersion, p->r_cut, p->box);
    const TypeTable tt = {types, (const float4 *)table, (int)num_types, (int)num_types | 1};
    const ExclList ex = {row_start, col, weight_coulomb, weight_lj, (int)p->num_points, (int)num_entries};
    const size_t lds = (size_t)2 * tt.T * tt.S * sizeof(float2);
    const int64_t cells_per_set = (int64_t)p->cells[0] * p->cells[1] * p->cells[2];
    const int64_t slots = ewald_virial_near_item_slots(p);
    int2 *items = (int2 *)workspace;
    double *partial = ewald_virial_near_partials(p, workspace);
    if (int rc = launch_nearfield_items(p->batch_size * cells_per_set, p->num_points, start, items, stream)) return rc;
    if (row_start)
        hipLaunchKernelGGL((bmh_table_near_kernel<true>), dim3((unsigned)slots), dim3(kNearBlock), lds, stream, qc, qd, tt, ex,
                           (const int2 *)items, pos, xs, start, index, f, partial);
    else
        hipLaunchKernelGGL((bmh_table_near_kernel<false>), dim3((unsigned)slots), dim3(kNearBlock), lds, stream, qc, qd, tt, ex,
                           (const int2 *)items, pos, xs, start, index, f, partial);
    NFFT_HIP_CHECK(hipGetLastError());
    return launch_virial_sum_terms(partial, kBmhTerms, p->batch_size, 1, 0, items, start, (int)cells_per_set, out, stream);
}

}  // namespace nfft
