// The frame of the pair kernels: nearfield.hip (the open grid of the fast summation), ewald_near.hip,
// ewald_disp.hip, ewald_dipole.hip, ewald_stokeslet.hip, ewald_yukawa.hip, ewald_step.hip and the pair reductions and step
// walks of virial_frame.h and step_frame.h (the wrapped grid of the Ewald sums) stand on all of it, nearfield_pgrad.hip on all
// but the tile sweep, nearfield_grad.hip on the host dispatch only (section 7d says why).
// Both point sets come ordered by (point set, cell) with a start table.  A workgroup owns one work item -- up to kNearBlock
// output points of one cell -- and a lane one output point; a walk hands the contiguous ranges of streamed points of the
// neighbouring cells to a sweep, which passes them through LDS in tiles of kNearTile (the position as one float4, the
// values as the kernel's staging policy lays them out); every lane reads the same streamed point (an LDS broadcast) and
// keeps its sums in registers, in the order of the sorted points.  No atomics.  What a kernel adds is its pair body, its
// staging policy and its epilogue.
#pragma once
#include <type_traits>

#include "nearfield.h"

namespace nfft {

// ---- the lane of a work item ------------------------------------------------------------------------------------------

struct PairLane {
    int cell;          // the item's cell
    int ti;            // the lane's output point in cell order
    bool active;       // ... which exists
    bool wave_active;  // some lane of this wave has one
};

// the lane of the workgroup's item = items[blockIdx.x], (cell, first output point); the kernel returns on an empty slot
// (item.x < 0, uniform) before it asks
__device__ __forceinline__ PairLane pair_lane(int2 item, const int *__restrict__ ostart)
{
    const int tid = threadIdx.x;
    const int tend = min(item.y + kNearBlock, ostart[item.x + 1]);
    const int ti = item.y + tid;
    return {item.x, ti, ti < tend, item.y + (tid & ~63) < tend};
}

// point i of [points, dim] as a float4, the axes past dim zero
__device__ __forceinline__ float4 load_position(const float *__restrict__ pos, int64_t i, int dim)
{
    const float *sp = pos + i * dim;
    float4 v = make_float4(sp[0], 0.f, 0.f, 0.f);
    if (dim >= 2) v.y = sp[1];
    if (dim >= 3) v.z = sp[2];
    return v;
}

// the lane's own position; a lane without an output point sits at (away_x, 0, 0)
__device__ __forceinline__ float4 lane_position(const PairLane &l, const float *__restrict__ pos, int dim, float away_x)
{
    float4 t = make_float4(away_x, 0.f, 0.f, 0.f);
    if (l.active) t = load_position(pos, l.ti, dim);
    return t;
}

// ---- the two walks: each hands contiguous ranges [first, last) of streamed points to range(first, last) ---------------

// G^dim cells, clipped at the grid's edge: 3^(dim-1) rows, the cells c0 - 1 .. c0 + 1 of a row are one range
struct OpenWalk {
    int k, G, c0, c1, c2, r1, r2;
    __device__ __forceinline__ OpenWalk(int cell, int dim, int cells_per_axis) : k(cell), G(cells_per_axis)
    {
        c0 = k % G;
        c1 = dim >= 2 ? (k / G) % G : 0;
        c2 = dim >= 3 ? (k / (G * G)) % G : 0;
        r1 = dim >= 2 ? 1 : 0;
        r2 = dim >= 3 ? 1 : 0;
    }
    template <typename Range>
    __device__ __forceinline__ void operator()(const int *__restrict__ sstart, Range &&range) const
    {
        for (int d2 = -r2; d2 <= r2; ++d2) {
            if (c2 + d2 < 0 || c2 + d2 >= G) continue;
            for (int d1 = -r1; d1 <= r1; ++d1) {
                if (c1 + d1 < 0 || c1 + d1 >= G) continue;
                const int row = k + (d2 * G + d1) * G;
                range(sstart[row - (c0 > 0 ? 1 : 0)], sstart[row + (c0 < G - 1 ? 1 : 0) + 1]);
            }
        }
    }
};

// G0 x G1 x G2 cells that cover the whole torus, every G_a >= 3 (the 27 cells are distinct): the rows wrap with G1 and G2;
// the cells c0 - 1 .. c0 + 1 of a row are ranges of cells [lo, hi), one inside the row and two at its ends (the wrapped
// cell, then the two others)
struct WrappedWalk {
    int G0, G1, G2, c1, c2, set0, lo0, hi0, lo1, hi1;
    bool split;
    __device__ __forceinline__ WrappedWalk(int k, int g0, int g1, int g2) : G0(g0), G1(g1), G2(g2)
    {
        const int c0 = k % G0;
        c1 = (k / G0) % G1;
        c2 = (k / (G0 * G1)) % G2;
        set0 = k - (c2 * G1 + c1) * G0 - c0;  // first cell of the point set
        split = c0 == 0 || c0 == G0 - 1;
        lo0 = c0 == 0 ? G0 - 1 : (c0 == G0 - 1 ? 0 : c0 - 1);
        hi0 = c0 == 0 ? G0 : (c0 == G0 - 1 ? 1 : c0 + 2);
        lo1 = c0 == 0 ? 0 : G0 - 2;
        hi1 = c0 == 0 ? 2 : G0;
    }
    template <typename Range>
    __device__ __forceinline__ void operator()(const int *__restrict__ start, Range &&range) const
    {
        for (int d2 = -1; d2 <= 1; ++d2) {
            const int w2 = c2 + d2 < 0 ? G2 - 1 : (c2 + d2 >= G2 ? 0 : c2 + d2);
            for (int d1 = -1; d1 <= 1; ++d1) {
                const int w1 = c1 + d1 < 0 ? G1 - 1 : (c1 + d1 >= G1 ? 0 : c1 + d1);
                const int row = set0 + (w2 * G1 + w1) * G0;
                for (int part = 0; part < (split ? 2 : 1); ++part)
                    range(start[row + (part ? lo1 : lo0)], start[row + (part ? hi1 : hi0)]);
            }
        }
    }
};

// ---- the tile sweep ---------------------------------------------------------------------------------------------------

// The streamed points [first, last) in tiles of kNearTile: barrier, the positions into s_pos, the values by the kernel's
// staging policy, barrier, then pair(j) for every staged point j in order, UNROLL of them in flight; a wave without an
// output point takes part in the staging and the barriers only.  The policy has point(j, i), called next to the position
// of the staged point j = streamed point i.
template <int UNROLL, typename Stage, typename Pair>
__device__ __forceinline__ void sweep_range(int first, int last, const PairLane &lane, float4 *s_pos,
                                            const float *__restrict__ pos, int dim, const Stage &stage, Pair &&pair)
{
    const int tid = threadIdx.x;
    for (int t0 = first; t0 < last; t0 += kNearTile) {
        const int cnt = min(kNearTile, last - t0);
        __syncthreads();
        for (int j = tid; j < cnt; j += kNearBlock) {
            s_pos[j] = load_position(pos, t0 + j, dim);
            stage.point(j, t0 + j);
        }
        __syncthreads();
        if (!lane.wave_active) continue;
#pragma unroll UNROLL
        for (int j = 0; j < cnt; ++j) pair(j);
    }
}

// staging policy: CC columns from col0 on of x [points, Cr] per staged point, zero past Cr
template <int CC>
struct StageColumns {
    float *s_x;
    const float *__restrict__ x;
    int64_t Cr, col0;
    __device__ __forceinline__ void point(int j, int64_t i) const
    {
        const float *xp = x + i * Cr + col0;
#pragma unroll
        for (int c = 0; c < CC; ++c) s_x[j * CC + c] = col0 + c < Cr ? xp[c] : 0.f;
    }
};

// ---- pair arithmetic --------------------------------------------------------------------------------------------------

struct PairSep {
    float dx, dy, dz, rr;  // output - streamed, and its squared length
};

__device__ __forceinline__ PairSep pair_sep(float dx, float dy, float dz) { return {dx, dy, dz, dx * dx + dy * dy + dz * dz}; }

__device__ __forceinline__ PairSep open_sep(const float4 &t, const float4 &s) { return pair_sep(t.x - s.x, t.y - s.y, t.z - s.z); }

// T_I, or T_I' / r, as a Horner form in u = r^2 / eps_I^2 over PT terms
template <int PT>
__device__ __forceinline__ float horner(const float (&a)[PT], float u)
{
    float t = a[PT - 1];
#pragma unroll
    for (int e = PT - 2; e >= 0; --e) t = t * u + a[e];
    return t;
}

// the block of the Ewald pair kernels: cells per axis (cubic: three times G), the lower triangle of A (cubic: not read)
struct EwaldPairParams {
    int G0, G1, G2;
    int64_t Cr;
    float alpha, neg_alpha2, rc2, slope;  // alpha, -alpha^2, r_c^2, 2 alpha / sqrt(pi)
    float a00, a10, a11, a20, a21, a22;
};

// box == nullptr: the unit cube
inline EwaldPairParams ewald_pair_params(int g0, int g1, int g2, int64_t num_columns, double alpha, double r_cut,
                                         const double *box)
{
    static const double unit[6] = {1.0, 0.0, 1.0, 0.0, 0.0, 1.0};
    if (!box) box = unit;
    EwaldPairParams q;
    q.G0 = g0;
    q.G1 = g1;
    q.G2 = g2;
    q.Cr = num_columns;
    q.alpha = (float)alpha;
    q.neg_alpha2 = (float)(-alpha * alpha);
    q.rc2 = (float)(r_cut * r_cut);
    q.slope = (float)(2.0 * alpha / 1.7724538509055160273);
    q.a00 = (float)box[0];
    q.a10 = (float)box[1];
    q.a11 = (float)box[2];
    q.a20 = (float)box[3];
    q.a21 = (float)box[4];
    q.a22 = (float)box[5];
    return q;
}

// the image of t - s: wrapped componentwise, then (BOX) d = ds A, A lower triangular with rows = lattice vectors
template <bool BOX>
__device__ __forceinline__ PairSep ewald_image(const float4 &t, const float4 &s, const EwaldPairParams &q)
{
    float s0 = t.x - s.x, s1 = t.y - s.y, s2 = t.z - s.z;
    s0 -= rintf(s0);
    s1 -= rintf(s1);
    s2 -= rintf(s2);
    if (!BOX) return pair_sep(s0, s1, s2);
    return pair_sep(fmaf(s2, q.a20, fmaf(s1, q.a10, s0 * q.a00)), fmaf(s2, q.a21, s1 * q.a11), s2 * q.a22);
}

// the pair weights from rr = r^2 > 0: w = erfc(alpha r) / r, and on request its negated slope
// mg = -g = (erfc(alpha r) / r + (2 alpha / sqrt(pi)) e^(-alpha^2 r^2)) / r^2
struct EwaldPairWeight {
    float w, ir, rr;
    __device__ __forceinline__ EwaldPairWeight(float r2, const EwaldPairParams &q) : ir(rsqrtf(r2)), rr(r2)
    {
        w = erfcf(q.alpha * (rr * ir)) * ir;
    }
    __device__ __forceinline__ float mg(const EwaldPairParams &q) const { return (w + q.slope * __expf(q.neg_alpha2 * rr)) * (ir * ir); }
};

// the pair weights of the dipole sum from rr = r^2 > 0: the Smith functions B_0 = erfc(alpha r) / r and
// B_l = ((2l - 1) B_(l-1) + (2 alpha^2)^l / (alpha sqrt(pi)) e^(-alpha^2 r^2)) / r^2 up to l = TOP (B_1 is EwaldPairWeight::mg).
// One erfcf, one __expf, one rsqrtf; every term of the recurrence is positive: no cancellation.
template <int TOP>
struct DipolePairWeight {
    float B[TOP + 1];
    __device__ __forceinline__ DipolePairWeight(float rr, const EwaldPairParams &q)
    {
        const float ir = rsqrtf(rr), ir2 = ir * ir;
        const float two_alpha2 = -2.f * q.neg_alpha2;
        float g = q.slope * __expf(q.neg_alpha2 * rr);  // (2 alpha^2)^l / (alpha sqrt(pi)) e^(-alpha^2 r^2) at l = 1
        B[0] = erfcf(q.alpha * (rr * ir)) * ir;
#pragma unroll
        for (int l = 1; l <= TOP; ++l) {
            B[l] = fmaf((float)(2 * l - 1), B[l - 1], g) * ir2;
            g *= two_alpha2;
        }
    }
};

// the pair weights of the Stokeslet sum from rr = r^2 > 0, with the Smith functions B_0, B_1, B_2 above and
// their l = 1 inhomogeneity g = (2 alpha / sqrt(pi)) e^(-alpha^2 r^2): a = B_0 - g weighs f, B1 weighs (d . f) d, and for the
// velocity gradient (ORDER = 2) c = 2 alpha^2 g - B_1 = (d/dr)(B_0 - g) / r and B2 = (3 B_1 + 2 alpha^2 g) / r^2 = -(d/dr) B_1 / r.
// One erfcf, one __expf, one rsqrtf.  a changes sign near alpha r = 0.56: the difference loses digits there relative to
// itself, not relative to the sum, whose other term B_1 m d is of the size of B_0.
template <int ORDER>
struct StokesletPairWeight {
    float a, B1, c, B2;
    __device__ __forceinline__ StokesletPairWeight(float rr, const EwaldPairParams &q)
    {
        const float ir = rsqrtf(rr), ir2 = ir * ir;
        const float g = q.slope * __expf(q.neg_alpha2 * rr);
        const float B0 = erfcf(q.alpha * (rr * ir)) * ir;
        a = B0 - g;
        B1 = (B0 + g) * ir2;
        if (ORDER == 2) {
            const float g2 = -2.f * q.neg_alpha2 * g;  // 2 alpha^2 g
            c = g2 - B1;
            B2 = fmaf(3.f, B1, g2) * ir2;
        } else {
            c = B2 = 0.f;
        }
    }
};

// the pair weights of the dispersion sum from rr = r^2 > 0, a2 = alpha^2 r^2:
// w = e^(-a2) (1 + a2 + a2^2 / 2) / r^6, and on request its negated slope mg = -w'(r) / r = e^(-a2) (6 + 6 a2 + 3 a2^2 + a2^3) / r^8.
// One reciprocal, one exponential, two Horner forms; r^-8 leaves float32 below r ~ 1.6e-5.
struct DispersionPairWeight {
    float w, e, a2, ir2, ir6;
    __device__ __forceinline__ DispersionPairWeight(float r2, const EwaldPairParams &q) : ir2(__builtin_amdgcn_rcpf(r2))
    {
        const float x = q.neg_alpha2 * r2;
        a2 = -x;
        e = __expf(x);
        ir6 = ir2 * ir2 * ir2;
        w = e * ((0.5f * a2 + 1.f) * a2 + 1.f) * ir6;
    }
    __device__ __forceinline__ float mg() const { return e * (((a2 + 3.f) * a2 + 6.f) * a2 + 6.f) * (ir6 * ir2); }
};

// the constants of the Yukawa pair weight beside EwaldPairParams: the screening parameter lambda,
// beta = lambda / (2 alpha), e^(-beta^2) and (2 alpha / sqrt(pi)) e^(-beta^2)
struct YukawaPairParams {
    float lambda, beta, ebeta, gslope;
};

inline YukawaPairParams yukawa_pair_params(double alpha, double screening)
{
    const double beta = screening / (2.0 * alpha);
    YukawaPairParams y;
    y.lambda = (float)screening;
    y.beta = (float)beta;
    y.ebeta = (float)std::exp(-beta * beta);
    y.gslope = (float)(2.0 * alpha / 1.7724538509055160273 * std::exp(-beta * beta));
    return y;
}

// the pair weights of the screened Coulomb sum e^(-lambda r) / r from rr = r^2 > 0, with
// P = e^(lambda r) erfc(alpha r + beta) and M = e^(-lambda r) erfc(alpha r - beta): w = (P + M) / (2 r), and on request its
// negated slope mg = -w'(r) / r = (w + lambda (M - P) / 2 + g) / r^2, g = (2 alpha / sqrt(pi)) e^(-alpha^2 r^2 - beta^2); M >= P, so the
// three terms are positive and nothing cancels.  At lambda = 0 these are EwaldPairWeight's.
// A mixed form: M as written (erfcf takes a negative argument as it is), but P = e^(-alpha^2 r^2 - beta^2) erfcx(alpha r + beta),
// which is the same number since (alpha r + beta)^2 = alpha^2 r^2 + beta^2 + lambda r.  The plain product loses P where
// erfc(alpha r + beta) leaves float32 (alpha r + beta > 9.2, e.g. alpha r = beta = 4.6, lambda r = 42) although P is still 6 % of M
// there, and overflows past lambda r = 88; this one does neither, its erfcx argument is positive (the all-erfcx form would need
// erfcx at alpha r - beta < 0, a growing exponential again), and the exponential that it needs is the one g needs.  Cost: one
// erfcf, one erfcxf, one rsqrtf, one expf (e^(-lambda r): its argument reaches 50, where the fast exponential's rounding of
// lambda r log2(e) alone is 3e-6) and one __expf.  Section 7p has what a comparison with the plain form showed.
struct YukawaPairWeight {
    float w, ir, hd, e;  // hd = (M - P) / 2, e = e^(-alpha^2 r^2)
    __device__ __forceinline__ YukawaPairWeight(float rr, const EwaldPairParams &q, const YukawaPairParams &y) : ir(rsqrtf(rr))
    {
        const float r = rr * ir, ar = q.alpha * r;
        e = __expf(q.neg_alpha2 * rr);
        const float P = y.ebeta * e * erfcxf(ar + y.beta);
        const float M = expf(-y.lambda * r) * erfcf(ar - y.beta);
        w = 0.5f * (P + M) * ir;
        hd = 0.5f * (M - P);
    }
    __device__ __forceinline__ float mg(const YukawaPairParams &y) const { return (w + y.lambda * hd + y.gslope * e) * (ir * ir); }
};

// ---- float64 sum over a workgroup -------------------------------------------------------------------------------------

// Each of the N values summed over the WAVES waves of the workgroup: a butterfly inside each wave (the same bits in every
// lane), then the waves in order.  Thread t < N returns the sum of v[t], the others 0.  Every thread must be here.
template <int WAVES, int N>
__device__ __forceinline__ double block_sum_f64(const double (&v)[N], double (&s_red)[WAVES][N])
{
    const int tid = threadIdx.x;
    __syncthreads();  // (s_red of the call before has been read)
#pragma unroll
    for (int n = 0; n < N; ++n) {
        double s = v[n];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
        if ((tid & 63) == 0) s_red[tid >> 6][n] = s;
    }
    __syncthreads();
    double r = 0.0;
    if (tid < N) {
        r = s_red[0][tid];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) r += s_red[w][tid];
    }
    return r;
}

// ---- host: run-time values to compile-time constants ------------------------------------------------------------------
// f receives a std::integral_constant; a launch site nests them and names its kernel once.

template <int V>
using int_c = std::integral_constant<int, V>;

// columns per pass CC: 1, 2, or 4 for three and more
template <typename F>
void dispatch_columns(int64_t num_columns, F &&f)
{
    if (num_columns == 1) f(int_c<1>{});
    else if (num_columns == 2) f(int_c<2>{});
    else f(int_c<4>{});
}

// Horner terms PT: 4 or 8
template <typename F>
void dispatch_terms(int terms, F &&f)
{
    if (terms <= 4) f(int_c<4>{});
    else f(int_c<8>{});
}

template <typename F>
void dispatch_flag(bool flag, F &&f)
{
    if (flag) f(int_c<1>{});
    else f(int_c<0>{});
}

// NFFT_HIP_KERNEL_*
template <typename F>
void dispatch_kernel(int kernel, F &&f)
{
    switch (kernel) {
    case NFFT_HIP_KERNEL_ONE_OVER_MODULUS: f(int_c<NFFT_HIP_KERNEL_ONE_OVER_MODULUS>{}); break;
    case NFFT_HIP_KERNEL_ONE_OVER_SQUARE: f(int_c<NFFT_HIP_KERNEL_ONE_OVER_SQUARE>{}); break;
    case NFFT_HIP_KERNEL_LOGARITHM: f(int_c<NFFT_HIP_KERNEL_LOGARITHM>{}); break;
    case NFFT_HIP_KERNEL_THINPLATE_SPLINE: f(int_c<NFFT_HIP_KERNEL_THINPLATE_SPLINE>{}); break;
    case NFFT_HIP_KERNEL_MULTIQUADRIC: f(int_c<NFFT_HIP_KERNEL_MULTIQUADRIC>{}); break;
    case NFFT_HIP_KERNEL_INVERSE_MULTIQUADRIC: f(int_c<NFFT_HIP_KERNEL_INVERSE_MULTIQUADRIC>{}); break;
    case NFFT_HIP_KERNEL_GAUSSIAN: f(int_c<NFFT_HIP_KERNEL_GAUSSIAN>{}); break;
    default: f(int_c<NFFT_HIP_KERNEL_LAPLACIAN_RBF>{}); break;
    }
}

}  // namespace nfft
