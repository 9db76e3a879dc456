// The frame of the nonbonded step walks on top of pair_frame.h: ewald_lj_step.hip, ewald_lj_table.hip
// and ewald_bmh_table.hip each give a PAIR LAW -- the short-range energy of a pair within r_c and where its coefficients come
// from -- and step_near_kernel<Law, MASKED> is the walk around it, once:
//
//     ewald_step_near_kernel's items, lanes, LDS tiles, 27-cell walk, image and test 0 < rr < rc2.  A streamed point is staged
//     as ONE float4 by the law's policy, (q_j, c_j, ...): one 16-byte LDS read per pair, 8320 bytes of static LDS.  Per passing
//     pair: the law's coefficients; MASKED, the list (below); EwaldPairWeight at alpha_C, DispersionPairWeight at alpha_D, the
//     law's (slope, u); then s = q_i q_j mg_C - c_i c_j mg_D + slope and eleven float32 sums: s d_a (the force), s d_a d_b
//     (xx, yy, zz, yz, xz, xy), q_i q_j w_C and u - c_i c_j w_D.  A lane with a target stores its force through `index`; the
//     other eight sums are halved and summed in float64 over the workgroup: one partial [8] per item slot, in the order U_C,
//     U_sr, xx, yy, zz, yz, xz, xy.  The second level is launch_virial_sum_terms of ewald_virial.hip with eight terms.  No
//     atomics anywhere and every order of addition is fixed by the launch geometry: two calls give the same bits.
//
//     MASKED: the list is ExclusionList's CSR matrix over the points in the CALLER's order, and the staged float4 ends with
//     the streamed point's caller-order index as integer bits.  A lane reads its own caller index and its row bounds once and
//     keeps lo = col[first], hi = col[last - 1] (an empty row: an empty interval).  A passing pair whose index lies outside
//     [lo, hi] takes the unmasked expressions; inside, a binary search of the lane's row decides.  On a hit q_i q_j is scaled by
//     s^C = 1 - wc, c_i c_j and the law's coefficients by s^L = 1 - wl, and the same expressions follow; a pair with both scales
//     zero returns before its weights are formed and adds nothing.  Entries and row bounds out of range are skipped, not
//     trusted.  The unmasked instantiation holds none of that code and reads no list; with an empty list the masked one gives
//     the unmasked bits.
//
// A law has
//     kValues                   values per point in xs [n, kValues], (q, c) first
//     Params                    its block, a kernel argument by value; Law(params) runs once per workgroup, before the walk
//                               (the table laws fill their dynamic LDS there, with the barrier that ends it)
//     stage<MASKED>(s_x, xs, index)   the staging policy
//     Own own(xp, ti)           what a lane keeps of its own point (xp its row of xs, ti its place in cell order); Own{} is
//                               what a lane without a target keeps
//     Coef coef(own, v)         the pair's coefficients from that and the staged float4 v
//     Coef::scale(sl)           the coefficients that s^L multiplies
//     Coef::terms(e, w6, slope, u)    the short-range slope -u'(r) / r and energy u from the two weights
// -ffp-contract=on fuses within one expression only: a law's expressions live whole inside terms().
#pragma once
#include "virial_frame.h"

namespace nfft {

constexpr int kStepTerms = 8;   // U_C, U_sr, xx, yy, zz, yz, xz, xy
constexpr int kStepSums = 11;   // s d_x, d_y, d_z; s d_a d_b in the order of the virial's terms; the two energies
constexpr int kMaxTypes = 32;   // T of a type-pair table at most: the table lives in LDS

// the CSR list on the device
struct ExclList {
    const int *__restrict__ row_start;
    const int *__restrict__ col;
    const float *__restrict__ wc;
    const float *__restrict__ wl;
    int n, entries;
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
        const float *xp = xs + i * 2;
        s_x[j * 4 + 0] = xp[0];
        s_x[j * 4 + 1] = xp[1];
        s_x[j * 4 + 2] = __int_as_float(clamp_type(types[i], T));
        s_x[j * 4 + 3] = __int_as_float((int)index[i]);
    }
};

// the types and their table of Entry per pair of types: the block of a table law
template <class Entry>
struct TypeTable {
    const int *__restrict__ types;    // [n] in cell order
    const Entry *__restrict__ table;  // [T, T], aligned to an Entry: an entry moves as one load
    int T, S;                         // types; entries between two rows in LDS, T | 1
};

// What the table laws share.  A point carries (q, c) and a type (clamped into [0, T): not trusted), staged with the index
// bits in both instantiations.  The table sits in dynamic LDS as float2 entries, a row per type of the LANE's point and rows
// S = T | 1 entries apart; a lane keeps t_i S and a passing pair reads at t_i S + t_j
template <class Entry>
struct TableLaw {
    static constexpr int kValues = 2;
    typedef TypeTable<Entry> Params;
    typedef int Own;
    const Params tt;
    float2 *s_tab;
    // put(at, entry) for every entry, at = row S + col (32 lanes per row, T <= 32 of them with an entry: no division)
    template <class Put>
    __device__ __forceinline__ TableLaw(const Params &p, Put &&put) : tt(p)
    {
        extern __shared__ float2 s_dynamic[];
        s_tab = s_dynamic;
        for (int k = threadIdx.x; k < tt.T * kMaxTypes; k += kNearBlock) {
            const int row = k / kMaxTypes, col = k % kMaxTypes;
            if (col < tt.T) put(s_tab, row * tt.S + col, tt.table[row * tt.T + col]);
        }
        __syncthreads();
    }
    template <bool MASKED>
    __device__ __forceinline__ StageTyped stage(float *s_x, const float *xs, const int64_t *index) const
    {
        return {s_x, xs, tt.types, index, tt.T};
    }
    __device__ __forceinline__ Own own(const float *, int ti) const { return clamp_type(tt.types[ti], tt.T) * tt.S; }
};

// qc: the block of the Coulomb weights (alpha_C) and of the walk and the image; qd: that of the dispersion weights (alpha_D)
template <class Law, bool MASKED>
__global__ void __launch_bounds__(kNearBlock) step_near_kernel(EwaldPairParams qc, EwaldPairParams qd, typename Law::Params lp,
                                                               ExclList ex, const int2 *__restrict__ items,
                                                               const float *__restrict__ pos, const float *__restrict__ xs,
                                                               const int *__restrict__ start, const int64_t *__restrict__ index,
                                                               float *__restrict__ f, double *__restrict__ partial)
{
    __shared__ float4 s_pos[kNearTile];
    __shared__ __attribute__((aligned(16))) float s_x[kNearTile * 4];
    __shared__ double s_red[kNearBlock / 64][kStepTerms];
    const int2 item = items[blockIdx.x];
    if (item.x < 0) return;  // (uniform: an empty slot; the second level skips it)
    const Law law(lp);
    const PairLane lane = pair_lane(item, start);
    const WrappedWalk walk(lane.cell, qc.G0, qc.G1, qc.G2);
    // (a lane without a target sums pairs of the origin with zero parameters; it stores nothing)
    const float4 t = lane_position(lane, pos, 3, 0.f);
    float qi = 0.f, ci = 0.f;
    typename Law::Own own = {};
    int64_t gi = 0;
    int row0 = 0, row1 = 0, lo = 1, hi = 0;  // (no row: an empty interval)
    if (lane.active) {
        const float *xp = xs + (int64_t)lane.ti * Law::kValues;
        qi = xp[0];
        ci = xp[1];
        own = law.own(xp, lane.ti);
        if (MASKED) gi = index[lane.ti];  // (the row's number now; without a list the store reads it, and no register waits)
        if (MASKED && gi >= 0 && gi < ex.n) {
            row0 = max(ex.row_start[gi], 0);
            row1 = min(ex.row_start[gi + 1], ex.entries);
            if (row0 < row1) {
                lo = ex.col[row0];
                hi = ex.col[row1 - 1];
            }
        }
    }
    float acc[kStepSums];
#pragma unroll
    for (int e = 0; e < kStepSums; ++e) acc[e] = 0.f;
    const auto stage = law.template stage<MASKED>(s_x, xs, index);
    walk(start, [&](int first, int last) {
        sweep_range<2>(first, last, lane, s_pos, pos, 3, stage, [&](int j) {
            const PairSep d = ewald_image<true>(t, s_pos[j], qc);
            // the lanes that fail the test sit the expansion out
            if (!(d.rr > 0.f && d.rr < qc.rc2)) return;
            const float4 v = *reinterpret_cast<const float4 *>(s_x + j * 4);  // (q_j, c_j, the law's, the index's bits)
            typename Law::Coef k = law.coef(own, v);
            float qq = qi * v.x, cc = ci * v.y;
            if (MASKED) {
                const int jg = __float_as_int(v.w);
                if (jg >= lo && jg <= hi) {
                    const int at = find_in_row(ex.col, row0, row1, jg);
                    if (at >= 0) {
                        const float sc = 1.f - ex.wc[at], sl = 1.f - ex.wl[at];
                        if (sc == 0.f && sl == 0.f) return;  // fully excluded: nothing is formed
                        qq *= sc;
                        cc *= sl;
                        k.scale(sl);
                    }
                }
            }
            const EwaldPairWeight e(d.rr, qc);
            const DispersionPairWeight w6(d.rr, qd);
            float slope, u;
            k.terms(e, w6, slope, u);
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
            acc[10] += fmaf(-cc, w6.w, u);
        });
    });
    if (lane.active) {
        float *fp = f + (MASKED ? gi : index[lane.ti]) * 3;
        fp[0] = acc[0];
        fp[1] = acc[1];
        fp[2] = acc[2];
    }
    // every pair is seen from both ends: halved, float64 from here on; a lane without a target adds exactly zero
    double red[kStepTerms];
    red[0] = lane.active ? 0.5 * (double)acc[9] : 0.0;
    red[1] = lane.active ? 0.5 * (double)acc[10] : 0.0;
#pragma unroll
    for (int e = 0; e < 6; ++e) red[2 + e] = lane.active ? 0.5 * (double)acc[3 + e] : 0.0;
    block_sums_to_partial<kStepTerms, 1>(red, s_red, 1.0, 1, 0, partial);
}

// The launch of a step walk: the launch sequence of virial_frame.h around the walk (row_start == nullptr: no list, the
// unmasked instantiation) with `lds` bytes of dynamic LDS.  `workspace`: ewald_step8_near_workspace(p) bytes, 256-byte aligned
template <class Law>
int launch_step_near(const nfft_hip_ewald_box_problem *p, double alpha_dispersion, const typename Law::Params &lp, size_t lds,
                     int64_t num_entries, const float *pos, const float *xs, const int *start, const int64_t *index,
                     const int *row_start, const int *col, const float *weight_coulomb, const float *weight_lj, float *f,
                     double *out, void *workspace, hipStream_t stream)
{
    const EwaldPairParams qc = ewald_pair_params(p->cells[0], p->cells[1], p->cells[2], Law::kValues, p->alpha, p->r_cut, p->box);
    const EwaldPairParams qd = ewald_pair_params(p->cells[0], p->cells[1], p->cells[2], Law::kValues, alpha_dispersion, p->r_cut, p->box);
    const ExclList ex = {row_start, col, weight_coulomb, weight_lj, (int)p->num_points, (int)num_entries};
    return launch_pair_reduction(p, kStepTerms, 1, start, out, workspace, stream, [&](dim3 grid, const int2 *items, double *partial) {
        dispatch_flag(row_start != nullptr, [&](auto masked) {
            hipLaunchKernelGGL((step_near_kernel<Law, decltype(masked)::value != 0>), grid, dim3(kNearBlock), lds, stream, qc, qd, lp, ex,
                               items, pos, xs, start, index, f, partial);
        });
    });
}

}  // namespace nfft
