// Lennard-Jones + Coulomb step with per-type-pair parameters: the pair walk of sections 7r and 7s for
// force fields whose C6_ij and C12_ij are not products of per-point numbers (Lorentz-Berthelot mixing, fitted cross terms).
// A point carries a charge q_j, a GRID coefficient c_j and a type t_j in [0, T); a table [T, T] of (C12, dC6) holds, per pair
// of types, the repulsion coefficient and what the pair's C6 has above the product that the grid carries,
// dC6(t, t') = C6(t, t') - g_t g_t' with c_j = g_(t_j).  The far field and the list kernel of 7s see c alone and are unchanged:
// inside r_c a pair interacts with its exact C6_ij, beyond with c_i c_j.
//
// lj_table_near_kernel<MASKED>  lj_step_near_kernel<true>'s items, lanes, walk, tiles, image, test 0 < rr < rc2, eleven float32
//                        sums and epilogue.  The staging policy StageTyped puts (q_j, c_j) of xs [n, 2] and, as integer bits,
//                        the streamed point's type (clamped into [0, T): not trusted) and its caller-order index into one
//                        float4: one 16-byte LDS read per pair, 8320 bytes of static LDS as before.  The table is loaded once
//                        per workgroup (one 8-byte load per entry: `table` is 8-byte aligned, which the entry point checks)
//                        into dynamic LDS as float2 (C12, dC6), a row per type of the LANE's point and rows
//                        S = T | 1 entries apart (8 T S bytes; T = 32: 8448).  A lane keeps t_i S in a register and a passing
//                        pair takes one 8-byte LDS read at t_i S + t_j.  t_j is the same in every lane and t_i is not: the
//                        read is data-dependent, its banks are 2 (t_i S + t_j) mod 64 within a half wave, and with S odd
//                        the up to 32 rows of a half wave fall on 32 different bank pairs -- no conflict for any mix of
//                        types, where S = T = 32 would put every row on ONE bank pair (32-way).  Lanes of one type read one
//                        address (a broadcast).  Per passing pair
//                            p12 = (C12 ir6) ir6,   p6 = dC6 ir6,   slope = 12 (C12 ir6) (ir6 ir2) - 6 p6 ir2,
//                            s = qq mg_C - cc mg_D + slope,   energies qq w_C and p12 - p6 - cc w_D.
//                        MASKED adds 7s's interval test and find_in_row on the lane's CSR row: on a hit qq is scaled by s^C
//                        and cc, C12, dC6 by s^L; a pair with both scales zero returns before any weight is formed.  The
//                        unmasked instantiation holds none of that code and reads no list.  With an empty list the masked
//                        one gives the unmasked bits.
//
// The smallest separation.  The coefficient is multiplied in before the powers meet, so what must stay below 3.4e38 are
// r^-8 (r > 1.6e-5, as for the dispersion weight of 7j), C12 r^-6, 6 |dC6| r^-8 (r > 1.9e-5 |dC6|^(1/8)) and the slope itself,
// 12 C12 r^-14: r > 2.1e-3 C12^(1/14), e.g. 1.2e-4 at C12 = 2e-18 (sigma = 0.03, epsilon = 1).  Below that: not numbers.
//
// The second level is launch_virial_sum_terms of ewald_virial.hip with eight terms.  No atomics anywhere and every order of
// addition is fixed by the launch geometry: two calls give the same bits.
#include "pair_frame.h"

namespace nfft {

namespace {

constexpr int kLjTerms = 8;    // U_C, U_LJ, xx, yy, zz, yz, xz, xy
constexpr int kLjSums = 11;    // s d_x, d_y, d_z; s d_a d_b in the order of the virial's terms; the two energies
constexpr int kLjValues = 2;   // q, c
constexpr int kMaxTypes = 32;  // T at most: 8 T (T | 1) = 8448 bytes of LDS

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
    const int *__restrict__ types;    // [n] in cell order
    const float2 *__restrict__ table;  // [T, T]: (C12, dC6), 8-byte aligned
    int T, S;                         // types; entries between two rows in LDS, T | 1
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
        const float *xp = xs + i * kLjValues;
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
__global__ void __launch_bounds__(kNearBlock) lj_table_near_kernel(EwaldPairParams qc, EwaldPairParams qd, TypeTable tt, ExclList ex,
                                                                   const int2 *__restrict__ items, const float *__restrict__ pos,
                                                                   const float *__restrict__ xs, const int *__restrict__ start,
                                                                   const int64_t *__restrict__ index, float *__restrict__ f,
                                                                   double *__restrict__ partial)
{
    __shared__ float4 s_pos[kNearTile];
    __shared__ __attribute__((aligned(16))) float s_x[kNearTile * 4];
    __shared__ double s_red[kNearBlock / 64][kLjTerms];
    extern __shared__ float2 s_tab[];  // [T][S]: (C12, dC6), rows by the lane's type
    const int2 item = items[blockIdx.x];
    if (item.x < 0) return;  // (uniform: an empty slot; the second level skips it)
    // (32 lanes per row, T <= 32 of them with an entry: no division, one 8-byte load per entry)
    for (int k = threadIdx.x; k < tt.T * kMaxTypes; k += kNearBlock) {
        const int row = k / kMaxTypes, col = k % kMaxTypes;
        if (col < tt.T) s_tab[row * tt.S + col] = tt.table[row * tt.T + col];
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
        const float *xp = xs + (int64_t)lane.ti * kLjValues;
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
    float acc[kLjSums];
#pragma unroll
    for (int e = 0; e < kLjSums; ++e) acc[e] = 0.f;
    const StageTyped stage = {s_x, xs, tt.types, index, tt.T};
    walk(start, [&](int first, int last) {
        sweep_range<2>(first, last, lane, s_pos, pos, 3, stage, [&](int j) {
            const PairSep d = ewald_image<true>(t, s_pos[j], qc);
            // the lanes that fail the test sit the expansion out
            if (!(d.rr > 0.f && d.rr < qc.rc2)) return;
            const float4 v = *reinterpret_cast<const float4 *>(s_x + j * 4);  // (q_j, c_j, the type's bits, the index's bits)
            const float2 tab = s_tab[tiS + __float_as_int(v.z)];              // (C12, dC6) of the two types
            float qq = qi * v.x, cc = ci * v.y, c12 = tab.x, dc6 = tab.y;
            if (MASKED) {
                const int jg = __float_as_int(v.w);
                if (jg >= lo && jg <= hi) {
                    const int k = find_in_row(ex.col, row0, row1, jg);
                    if (k >= 0) {
                        const float sc = 1.f - ex.wc[k], sl = 1.f - ex.wl[k];
                        if (sc == 0.f && sl == 0.f) return;  // fully excluded: nothing is formed
                        qq *= sc;
                        cc *= sl;
                        c12 *= sl;
                        dc6 *= sl;
                    }
                }
            }
            const EwaldPairWeight e(d.rr, qc);
            const DispersionPairWeight w6(d.rr, qd);
            const float a6 = c12 * w6.ir6;  // C12 / r^6: the coefficient goes in first
            const float p12 = a6 * w6.ir6, p6 = dc6 * w6.ir6;
            const float slope = fmaf(12.f * a6, w6.ir6 * w6.ir2, -6.f * p6 * w6.ir2);
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
            acc[10] += fmaf(-cc, w6.w, p12 - p6);
        });
    });
    if (lane.active) {
        float *fp = f + gi * 3;
        fp[0] = acc[0];
        fp[1] = acc[1];
        fp[2] = acc[2];
    }
    // every pair is seen from both ends: halved, float64 from here on; a lane without a target adds exactly zero
    double red[kLjTerms];
    red[0] = lane.active ? 0.5 * (double)acc[9] : 0.0;
    red[1] = lane.active ? 0.5 * (double)acc[10] : 0.0;
#pragma unroll
    for (int e = 0; e < 6; ++e) red[2 + e] = lane.active ? 0.5 * (double)acc[3 + e] : 0.0;
    const double v = block_sum_f64(red, s_red);
    const int tid = threadIdx.x;
    if (tid < kLjTerms) partial[(int64_t)blockIdx.x * kLjTerms + tid] = v;
}

int64_t round256(int64_t bytes) { return (bytes + 255) & ~int64_t(255); }

}  // namespace

// the workspace is that of the walks of 7r and 7s: the work items, then one partial [8] per item slot
int64_t ewald_lj_table_near_workspace(const nfft_hip_ewald_box_problem *p)
{
    const int64_t slots = ewald_virial_near_item_slots(p);
    return round256(slots * (int64_t)sizeof(int2)) + slots * kLjTerms * (int64_t)sizeof(double);
}

// row_start == nullptr: no list, the unmasked instantiation
int launch_ewald_lj_table_near(const nfft_hip_ewald_box_problem *p, double alpha_dispersion, int64_t num_types, int64_t num_entries,
                               const float *pos, const float *xs, const int *types, const float *table, const int *start,
                               const int64_t *index, const int *row_start, const int *col, const float *weight_coulomb,
                               const float *weight_lj, float *f, double *out, void *workspace, hipStream_t stream)
{
    if (num_types < 1 || num_types > kMaxTypes) return NFFT_HIP_EINVAL;  // (the entry point has said why)
    const EwaldPairParams qc = ewald_pair_params(p->cells[0], p->cells[1], p->cells[2], kLjValues, p->alpha, p->r_cut, p->box);
    const EwaldPairParams qd = ewald_pair_params(p->cells[0], p->cells[1], p->cells[2], kLjValues, alpha_dispersion, p->r_cut, p->box);
    const TypeTable tt = {types, (const float2 *)table, (int)num_types, (int)num_types | 1};
    const ExclList ex = {row_start, col, weight_coulomb, weight_lj, (int)p->num_points, (int)num_entries};
    const size_t lds = (size_t)tt.T * tt.S * sizeof(float2);
    const int64_t cells_per_set = (int64_t)p->cells[0] * p->cells[1] * p->cells[2];
    const int64_t slots = ewald_virial_near_item_slots(p);
    int2 *items = (int2 *)workspace;
    double *partial = ewald_virial_near_partials(p, workspace);
    if (int rc = launch_nearfield_items(p->batch_size * cells_per_set, p->num_points, start, items, stream)) return rc;
    if (row_start)
        hipLaunchKernelGGL((lj_table_near_kernel<true>), dim3((unsigned)slots), dim3(kNearBlock), lds, stream, qc, qd, tt, ex,
                           (const int2 *)items, pos, xs, start, index, f, partial);
    else
        hipLaunchKernelGGL((lj_table_near_kernel<false>), dim3((unsigned)slots), dim3(kNearBlock), lds, stream, qc, qd, tt, ex,
                           (const int2 *)items, pos, xs, start, index, f, partial);
    NFFT_HIP_CHECK(hipGetLastError());
    return launch_virial_sum_terms(partial, kLjTerms, p->batch_size, 1, 0, items, start, (int)cells_per_set, out, stream);
}

}  // namespace nfft
