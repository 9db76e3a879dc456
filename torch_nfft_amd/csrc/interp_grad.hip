// Gradient gather for gfx950: the derivative of the forward transform with respect to the points.
//
// For every real plane (b, cr) of a forward transform and every point i of set b,
//     G[cr, i, a] = w[i, cr] * d/dpos[i, a] sum_{l in [0,2m+2)^d} prod_k psi(t_k) * g[(b, cr), (shift_i + l) mod M]
//                 = w[i, cr] * M * sum_l psi'(t_a) prod_{k != a} psi(t_k) * g[...],     t_k = pos_k M - shift_k - l_k,
// with psi(t) = exp(-t^2 (3 pi / 4) / m) sqrt(0.75 / m) and psi'(t) = -2 t ((3 pi / 4) / m) psi(t): the window of the
// forward transform differentiated analytically, applied to the same deconvolved, FFT'd grid it interpolates from.
// dpos[i, a] = sum_cr G[cr, i, a] (nfft_hip_forward_grad_points: DESIGN.md section "Gradient with respect to the points").
//
// The kernel is interp.hip's one-lane-per-point gather (same plan, same resident-plane sliding window, same aligned
// ds_read_b128 rows and packed FMAs, same point splits; geometry and launch from lane_gather.h) with two dot products per
// row instead of one -- the row with the axis-2 window and with its derivative -- and d partial sums carried through the
// plane and slab loops.  Every G value is written by exactly one lane and the sum over the planes runs in a fixed order
// (grad_reduce_kernel): no atomics, the result is bitwise reproducible.  A second kernel writes the interpolated value
// alongside (the fused gather of the fastsum backward: DESIGN.md section 7a).
#include "kernels.h"
#include "lane_gather.h"

namespace nfft {

namespace {

// part[(cr * n + i) * DIM + u]: the gradient of point i (caller order, user axis u) from real plane cr of its set, already
// multiplied by w[i, cr].  With one real plane per set part is dpos itself.
// VALUE: also y[i * Cr + cr], the plain interpolated value -- what interp_kernel writes for the same grid (same
// normalisation, same layout).  Every row sum V the gradient needs is the value's row sum as well, so the value costs one
// FMA per axis-0 plane and one store.  With VALUE = false, y is unused and the code is the gradient-only kernel's.
template <int DIM, int W, bool WIDE, bool VALUE>
__global__ void __launch_bounds__((GatherCfg<DIM, W, WIDE>::NT))
__attribute__((amdgpu_waves_per_eu(VALUE ? GatherCfg<DIM, W, WIDE>::WPE_VALUE : GatherCfg<DIM, W, WIDE>::WPE)))
interp_grad_kernel(const Geom g, const int *__restrict__ tile_offsets, const int *__restrict__ perm,
                   const float *__restrict__ spos, const float *__restrict__ grid, const int Cr, const int plane0,
                   const float *__restrict__ w, const int64_t n, float *__restrict__ part, float *__restrict__ y)
{
    using C = GatherCfg<DIM, W, WIDE>;
    constexpr int NT = C::NT;
    constexpr int NWAVES = C::NWAVES;
    __shared__ float4 planes4[C::CELLS / 4];
    float *const planes = (float *)planes4;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;

    const int seg = blockIdx.x % g.nseg;
    const int pencil = blockIdx.x / g.nseg;
    const int j2 = pencil % g.nta[2];
    const int j1 = pencil / g.nta[2];
    const int plane_local = blockIdx.y;
    const int plane = plane0 + plane_local;
    const int b = plane / Cr;
    const int cr = plane - b * Cr;

    const int k_begin = seg * kSegChunks;
    const int k_end = min(g.nta[0], k_begin + kSegChunks);
    const int bin0 = b * g.tiles_per_batch + pencil * g.np0;
    {
        int s0, e0, s1, e1;
        chunk_range(g, tile_offsets, bin0, k_begin, s0, e0);
        chunk_range(g, tile_offsets, bin0, k_end - 1, s1, e1);
        if (s0 == e1) return;
    }

    const int m = g.m;
    const int tb1 = j1 * g.Ta[1], tb2 = j2 * g.Ta[2];
    const float sc = win_exp_scale(m);
    // d psi(t) / d pos = M psi'(t) = dk t psi(t)
    const float dk = -(4.71238898038469f / (float)m) * (float)g.M;  // -2 (3 pi / 4) / m * M
    float norm = win_norm(m);
    norm = DIM == 3 ? norm * norm * norm : (DIM == 2 ? norm * norm : norm);
    const float *const gplane = grid + (int64_t)plane_local * g.cells;
    float *const out = part + (int64_t)cr * n * DIM;

    int base_z = 0, have = 0;
    const int nsplit = gridDim.z, split = blockIdx.z;
    for (int k = k_begin; k < k_end; ++k) {
        int s, e;
        chunk_range(g, tile_offsets, bin0, k, s, e);
        if (nsplit > 1) {
            const int span = (e - s + nsplit - 1) / nsplit;
            s = min(e, s + split * span);
            e = min(e, s + span);
        }
        if (e == s) continue;
        const int want_z = k * C::TC - C::M0OFF;
        // resident planes: slide the ones still needed down, fetch the rest (interp.hip)
        const int shift = have > 0 ? min(want_z - base_z, have) : 0;
        const int kept = have - shift;
        __syncthreads();
        if (kept > 0) {
            for (int lo = 0; lo < kept * C::S0; lo += shift * C::S0) {
                const int hi = min(lo + shift * C::S0, kept * C::S0);
                for (int idx = lo + tid; idx < hi; idx += NT) planes[idx] = planes[idx + shift * C::S0];
                __syncthreads();
            }
        }
        for (int row = kept * C::P1 + wave; row < C::NP * C::P1; row += NWAVES) {
            const int p = row / C::P1;
            const int r = row - p * C::P1;
            const int64_t gz = DIM == 3 ? wrap(want_z + p, g.Ma[0]) : 0;
            const int64_t g1 = DIM >= 2 ? wrap(tb1 - m + r, g.Ma[1]) : 0;
            const float *const grow = gplane + (gz * g.Ma[1] + g1) * g.Ma[2];
            for (int c = lane; c < C::S2; c += 64)
                planes[row * C::S2 + c] = c < C::P2 ? grow[wrap_near(tb2 - m + c, g.Ma[2])] : 0.0f;
        }
        base_z = want_z;
        have = C::NP;
        __syncthreads();
        const int tb0 = k * C::TC;

        for (int j0 = s + wave * 64; j0 < e; j0 += NWAVES * 64) {
            const int j = j0 + lane;
            if (j >= e) continue;
            int c0 = 0, c1 = 0, c2 = 0;
            float f0 = 0.f, f1 = 0.f, f2 = 0.f;
            int idx;
            if (DIM == 3) {
                const f32x4 rec = *(const f32x4 *)(spos + (int64_t)j * 4);  // {p0, p1, p2, index}
                split_cell(rec.x, g.M, c0, f0);
                split_cell(rec.y, g.M, c1, f1);
                split_cell(rec.z, g.M, c2, f2);
                idx = __float_as_int(rec.w);
            } else if (DIM == 2) {
                split_cell(spos[(int64_t)j * 2 + 0], g.M, c1, f1);
                split_cell(spos[(int64_t)j * 2 + 1], g.M, c2, f2);
                idx = perm[j];
            } else {
                split_cell(spos[j], g.M, c2, f2);
                idx = perm[j];
            }
            // (the value-writing 2-D kernels from m = 4 on read w[i, cr] after the window loops, where its register is free)
            constexpr bool LATE_W = VALUE && DIM == 2 && W >= 10;
            float wi = 0.0f;
            if (!LATE_W) wi = w[(int64_t)idx * Cr + cr];
            const int col = c2 - tb2;
            const int sh = col & 3;
            // axis-2 window on the aligned positions k = l2 + sh (zero outside the window), as in interp.hip.  Its derivative
            // needs no second set of weights: t = tau2 - k, so sum_k t w2 v = tau2 sum_k w2 v - sum_k k w2 v, and the
            // k-weighted sum falls out of a running suffix sum over the pairs (see the row loop)
            f32x2 w2[2 * C::NR];
#pragma unroll
            for (int q = 0; q < 2 * C::NR; ++q) {
                float pair[2];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int l2 = 2 * q + h - sh;
                    const float t = f2 + (float)(m - l2);
                    const float v = __builtin_amdgcn_exp2f(sc * t * t);
                    pair[h] = (l2 >= 0 && l2 < W) ? v : 0.0f;
                }
                w2[q] = f32x2{pair[0], pair[1]};
            }
            const float tau2 = f2 + (float)(m + sh);  // t of aligned position k: tau2 - k
            const float tau1 = f1 + (float)m;         // t of row l1: tau1 - l1
            const f32x4 *row0 = (const f32x4 *)(planes + (c0 - tb0) * C::S0 + (c1 - tb1) * C::S2 + (col - sh));
            float w1[C::W1];
#pragma unroll
            for (int l1 = 0; l1 < C::W1; ++l1) {
                const float t1 = f1 + (float)(m - l1);
                w1[l1] = DIM >= 2 ? __builtin_amdgcn_exp2f(sc * t1 * t1) : 1.0f;
            }
            float acc0 = 0.0f, acc1 = 0.0f, acc2 = 0.0f;  // d/d internal axis 0, 1, 2 (without dk, norm, w)
            float accv = 0.0f;                            // VALUE: the interpolated value (without norm)
            for (int l0 = 0; l0 < C::W0; ++l0) {
                const f32x4 *rowp = row0 + l0 * (C::S0 / 4);
                // rows from the last down, the same suffix-sum device along axis 1: pv = sum_{l1' >= l1} w1 S, and
                // pu = sum over the rows of pv = sum (l1 + 1) w1 S; pt = sum w1 T
                f32x2 pv = {0.0f, 0.0f}, pu = {0.0f, 0.0f}, pt = {0.0f, 0.0f};
#pragma unroll
                for (int l1 = C::W1 - 1; l1 >= 0; --l1) {
                    f32x4 v[C::NR];
#pragma unroll
                    for (int q = 0; q < C::NR; ++q) v[q] = rowp[l1 * (C::S2 / 4) + q];
                    // pairs P = 2q + hh (aligned positions 2P, 2P + 1) from the last down: S = sum_{P' >= P} w2 v,
                    // T = sum_P S = sum_P (P + 1) w2[P] v[P]
                    f32x2 S = w2[2 * C::NR - 1] * v[C::NR - 1].zw;
                    f32x2 T = S;
                    S = __builtin_elementwise_fma(w2[2 * C::NR - 2], v[C::NR - 1].xy, S);
                    T += S;
#pragma unroll
                    for (int q = C::NR - 2; q >= 0; --q) {
                        S = __builtin_elementwise_fma(w2[2 * q + 1], v[q].zw, S);
                        T += S;
                        S = __builtin_elementwise_fma(w2[2 * q], v[q].xy, S);
                        T += S;
                    }
                    const f32x2 wr = {w1[l1], w1[l1]};
                    pv = __builtin_elementwise_fma(wr, S, pv);
                    pt = __builtin_elementwise_fma(wr, T, pt);
                    if (DIM >= 2) pu += pv;
                }
                // value V = sum w v; sum k w v = 2 sum P X_P + sum of the odd positions = 2 (T - S) summed + S.y
                const float V = pv.x + pv.y;
                const float K = 2.0f * (pt.x + pt.y) - 2.0f * pv.x - pv.y;
                float p0 = 1.0f;
                if (DIM == 3) {
                    const float t0 = f0 + (float)(m - l0);
                    p0 = __builtin_amdgcn_exp2f(sc * t0 * t0);
                    acc0 = fmaf(t0 * p0, V, acc0);
                }
                if (VALUE) accv = fmaf(p0, V, accv);
                // sum l1 w1 S = pu - pv
                if (DIM >= 2) acc1 = fmaf(p0, fmaf(tau1, V, V - (pu.x + pu.y)), acc1);
                acc2 = fmaf(p0, fmaf(tau2, V, -K), acc2);
            }
            if (LATE_W) wi = w[(int64_t)idx * Cr + cr];
            const float f = dk * wi * norm;
            float *const o = out + (int64_t)idx * DIM;
            if (DIM == 3) {
                o[0] = acc0 * f;
                o[1] = acc1 * f;
                o[2] = acc2 * f;
            } else if (DIM == 2) {
                o[0] = acc1 * f;
                o[1] = acc2 * f;
            } else {
                o[0] = acc2 * f;
            }
            if (VALUE) y[(int64_t)idx * Cr + cr] = accv * norm;
        }
    }
}

// dpos[e] = sum_{cr < Cr} part[cr * len + e], planes in order
__global__ void __launch_bounds__(256)
grad_reduce_kernel(const float *__restrict__ part, const int64_t len, const int Cr, float *__restrict__ dpos)
{
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < len; e += (int64_t)gridDim.x * 256) {
        float s = part[e];
        for (int cr = 1; cr < Cr; ++cr) s += part[(int64_t)cr * len + e];
        dpos[e] = s;
    }
}

// Second-order gather (the backward of the weighted gradient gather G above).  For an upstream v
// [n, dim] (user axes), with q = sum_a v[i, a] t_a and the same deconvolved, FFT'd grid:
//     dw[i, cr]               = norm dk sum_l g psi q                                   (sum_a v_a d Fr / d pos_a)
//     part[(cr * n + i) * DIM + b] = w[i, cr] norm (dk^2 T_b + dk M v_b S0)               (the Hessian-vector gather)
// where S0 = sum_l g psi, T_b = sum_l g psi t_b q and psi is the product window: d + 2 accumulators with v folded in.
// Same plan, plane loading and lane-per-point walk as interp_grad_kernel.  Along axis 2 a row gives A = sum psi2 g,
// B = sum psi2 t2 g and C2 = sum psi2 t2^2 g = tau2 B - sum k psi2 t2 g, whose k-weighted sum is the running suffix sum
// of interp_grad_kernel.  dw is written once per (plane, point); the partial
// gradients are summed over the planes by grad_reduce_kernel in a fixed order: bitwise reproducible.  dw or part may be null.
template <int DIM, int W, bool WIDE>
__global__ void __launch_bounds__((GatherCfg<DIM, W, WIDE>::NT))
__attribute__((amdgpu_waves_per_eu(GatherCfg<DIM, W, WIDE>::WPE_HVP)))
interp_hvp_kernel(const Geom g, const int *__restrict__ tile_offsets, const int *__restrict__ perm,
                  const float *__restrict__ spos, const float *__restrict__ grid, const int Cr, const int plane0,
                  const float *__restrict__ w, const float *__restrict__ v, const int64_t n, float *__restrict__ dw,
                  float *__restrict__ part)
{
    using C = GatherCfg<DIM, W, WIDE>;
    constexpr int NT = C::NT;
    constexpr int NWAVES = C::NWAVES;
    __shared__ float4 planes4[C::CELLS / 4];
    float *const planes = (float *)planes4;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;

    const int seg = blockIdx.x % g.nseg;
    const int pencil = blockIdx.x / g.nseg;
    const int j2 = pencil % g.nta[2];
    const int j1 = pencil / g.nta[2];
    const int plane_local = blockIdx.y;
    const int plane = plane0 + plane_local;
    const int b = plane / Cr;
    const int cr = plane - b * Cr;

    const int k_begin = seg * kSegChunks;
    const int k_end = min(g.nta[0], k_begin + kSegChunks);
    const int bin0 = b * g.tiles_per_batch + pencil * g.np0;
    {
        int s0, e0, s1, e1;
        chunk_range(g, tile_offsets, bin0, k_begin, s0, e0);
        chunk_range(g, tile_offsets, bin0, k_end - 1, s1, e1);
        if (s0 == e1) return;
    }

    const int m = g.m;
    const int tb1 = j1 * g.Ta[1], tb2 = j2 * g.Ta[2];
    const float sc = win_exp_scale(m);
    const float dk = -(4.71238898038469f / (float)m) * (float)g.M;  // -2 (3 pi / 4) / m * M
    const float Mf = (float)g.M;
    float norm = win_norm(m);
    norm = DIM == 3 ? norm * norm * norm : (DIM == 2 ? norm * norm : norm);
    const float *const gplane = grid + (int64_t)plane_local * g.cells;
    float *const out = part ? part + (int64_t)cr * n * DIM : nullptr;

    int base_z = 0, have = 0;
    const int nsplit = gridDim.z, split = blockIdx.z;
    for (int k = k_begin; k < k_end; ++k) {
        int s, e;
        chunk_range(g, tile_offsets, bin0, k, s, e);
        if (nsplit > 1) {
            const int span = (e - s + nsplit - 1) / nsplit;
            s = min(e, s + split * span);
            e = min(e, s + span);
        }
        if (e == s) continue;
        const int want_z = k * C::TC - C::M0OFF;
        // resident planes: slide the ones still needed down, fetch the rest (interp.hip)
        const int shift = have > 0 ? min(want_z - base_z, have) : 0;
        const int kept = have - shift;
        __syncthreads();
        if (kept > 0) {
            for (int lo = 0; lo < kept * C::S0; lo += shift * C::S0) {
                const int hi = min(lo + shift * C::S0, kept * C::S0);
                for (int idx = lo + tid; idx < hi; idx += NT) planes[idx] = planes[idx + shift * C::S0];
                __syncthreads();
            }
        }
        for (int row = kept * C::P1 + wave; row < C::NP * C::P1; row += NWAVES) {
            const int p = row / C::P1;
            const int r = row - p * C::P1;
            const int64_t gz = DIM == 3 ? wrap(want_z + p, g.Ma[0]) : 0;
            const int64_t g1 = DIM >= 2 ? wrap(tb1 - m + r, g.Ma[1]) : 0;
            const float *const grow = gplane + (gz * g.Ma[1] + g1) * g.Ma[2];
            for (int c = lane; c < C::S2; c += 64)
                planes[row * C::S2 + c] = c < C::P2 ? grow[wrap_near(tb2 - m + c, g.Ma[2])] : 0.0f;
        }
        base_z = want_z;
        have = C::NP;
        __syncthreads();
        const int tb0 = k * C::TC;

        for (int j0 = s + wave * 64; j0 < e; j0 += NWAVES * 64) {
            const int j = j0 + lane;
            if (j >= e) continue;
            int c0 = 0, c1 = 0, c2 = 0;
            float f0 = 0.f, f1 = 0.f, f2 = 0.f;
            int idx;
            if (DIM == 3) {
                const f32x4 rec = *(const f32x4 *)(spos + (int64_t)j * 4);  // {p0, p1, p2, index}
                split_cell(rec.x, g.M, c0, f0);
                split_cell(rec.y, g.M, c1, f1);
                split_cell(rec.z, g.M, c2, f2);
                idx = __float_as_int(rec.w);
            } else if (DIM == 2) {
                split_cell(spos[(int64_t)j * 2 + 0], g.M, c1, f1);
                split_cell(spos[(int64_t)j * 2 + 1], g.M, c2, f2);
                idx = perm[j];
            } else {
                split_cell(spos[j], g.M, c2, f2);
                idx = perm[j];
            }
            // v on the internal axes (axis 2 is the last user axis)
            float v0 = 0.0f, v1 = 0.0f, v2;
            const float *const vi = v + (int64_t)idx * DIM;
            if (DIM == 3) { v0 = vi[0]; v1 = vi[1]; v2 = vi[2]; }
            else if (DIM == 2) { v1 = vi[0]; v2 = vi[1]; }
            else v2 = vi[0];
            const int col = c2 - tb2;
            const int sh = col & 3;
            const float tau2 = f2 + (float)(m + sh);  // t of aligned position k: tau2 - k
            const float tau1 = f1 + (float)m;         // t of row l1: tau1 - l1
            // axis-2 window on the aligned positions k = l2 + sh (zero outside the window), as in interp_grad_kernel
            f32x2 w2[2 * C::NR];
#pragma unroll
            for (int q = 0; q < 2 * C::NR; ++q) {
                float pair[2];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int l2 = 2 * q + h - sh;
                    const float t = f2 + (float)(m - l2);
                    const float wv = __builtin_amdgcn_exp2f(sc * t * t);
                    pair[h] = (l2 >= 0 && l2 < W) ? wv : 0.0f;
                }
                w2[q] = f32x2{pair[0], pair[1]};
            }
            const f32x4 *row0 = (const f32x4 *)(planes + (c0 - tb0) * C::S0 + (c1 - tb1) * C::S2 + (col - sh));
            float S0 = 0.0f, Q = 0.0f, T0 = 0.0f, T1 = 0.0f, T2 = 0.0f;  // (without norm, dk)
            for (int l0 = 0; l0 < C::W0; ++l0) {
                const f32x4 *rowp = row0 + l0 * (C::S0 / 4);
                float t0 = 0.0f, p0 = 1.0f;
                if (DIM == 3) {
                    t0 = f0 + (float)(m - l0);
                    p0 = __builtin_amdgcn_exp2f(sc * t0 * t0);
                }
                const float a0 = v0 * t0;
                float sA = 0.0f, sE = 0.0f, sE1 = 0.0f, sT2 = 0.0f;
#pragma unroll 1
                for (int l1 = 0; l1 < C::W1; ++l1) {
                    f32x4 vv[C::NR];
#pragma unroll
                    for (int q = 0; q < C::NR; ++q) vv[q] = rowp[l1 * (C::S2 / 4) + q];
                    // pairs from the last down, X = w2 v: SA = sum X, SB = sum t X, TB = sum_P (P + 1) t X.  The t of
                    // the pairs is recomputed per row: a second weight set held across the rows would spill
                    float tau = tau2;
                    asm volatile("" : "+v"(tau));
                    f32x2 tv = f32x2{tau, tau} - f32x2{(float)(4 * C::NR - 2), (float)(4 * C::NR - 1)};
                    f32x2 X = w2[2 * C::NR - 1] * vv[C::NR - 1].zw;
                    f32x2 SA = X;
                    f32x2 SB = X * tv;
                    f32x2 TB = SB;
#pragma unroll
                    for (int P = 2 * C::NR - 2; P >= 0; --P) {
                        tv += f32x2{2.0f, 2.0f};  // (exact: small integers apart)
                        X = w2[P] * ((P & 1) ? vv[P >> 1].zw : vv[P >> 1].xy);
                        SA += X;
                        SB = __builtin_elementwise_fma(X, tv, SB);
                        TB += SB;
                    }
                    const float A = SA.x + SA.y;
                    const float Bm = SB.x + SB.y;
                    const float KB = 2.0f * (TB.x + TB.y) - 2.0f * SB.x - SB.y;  // sum k t X
                    const float C2 = fmaf(tau2, Bm, -KB);                        // sum t2^2 psi2 v
                    float t1 = 0.0f, p1 = 1.0f;
                    if (DIM >= 2) {
                        t1 = tau1 - (float)l1;
                        p1 = __builtin_amdgcn_exp2f(sc * t1 * t1);
                    }
                    const float alpha = fmaf(v1, t1, a0);   // v0 t0 + v1 t1
                    const float E = fmaf(alpha, A, v2 * Bm); // sum psi2 q v
                    sA = fmaf(p1, A, sA);
                    sE = fmaf(p1, E, sE);
                    if (DIM >= 2) sE1 = fmaf(p1 * t1, E, sE1);
                    sT2 = fmaf(p1, fmaf(alpha, Bm, v2 * C2), sT2);
                }
                S0 = fmaf(p0, sA, S0);
                Q = fmaf(p0, sE, Q);
                if (DIM == 3) T0 = fmaf(p0 * t0, sE, T0);
                T1 = fmaf(p0, sE1, T1);
                T2 = fmaf(p0, sT2, T2);
            }
            if (dw) dw[(int64_t)idx * Cr + cr] = Q * (dk * norm);
            if (out) {
                const float wi = w[(int64_t)idx * Cr + cr] * norm;
                const float dd = dk * dk, dm = dk * Mf;
                float *const o = out + (int64_t)idx * DIM;
                if (DIM == 3) {
                    o[0] = wi * fmaf(dd, T0, dm * v0 * S0);
                    o[1] = wi * fmaf(dd, T1, dm * v1 * S0);
                    o[2] = wi * fmaf(dd, T2, dm * v2 * S0);
                } else if (DIM == 2) {
                    o[0] = wi * fmaf(dd, T1, dm * v1 * S0);
                    o[1] = wi * fmaf(dd, T2, dm * v2 * S0);
                } else {
                    o[0] = wi * fmaf(dd, T2, dm * v2 * S0);
                }
            }
        }
    }
}

} // namespace

int launch_interp_grad(const Geom &g, const PlanLayout &L, const void *plan, const float *grid, int64_t n, int64_t Cr,
                       int64_t plane0, int64_t nplanes, const float *w, float *part, hipStream_t stream)
{
    return launch_lane_gather(g, L, plan, n, nplanes, [&](auto cfg, const dim3 &blocks, const LanePlan &p) {
        using C = decltype(cfg);
        hipLaunchKernelGGL((interp_grad_kernel<C::DIM, C::W, C::WIDE, false>), blocks, dim3(C::NT), 0, stream, g,
                           p.tile_offsets, p.perm, p.spos, grid, (int)Cr, (int)plane0, w, n, part, nullptr);
    });
}

int launch_interp_value_grad(const Geom &g, const PlanLayout &L, const void *plan, const float *grid, int64_t n, int64_t Cr,
                             int64_t plane0, int64_t nplanes, const float *w, float *part, float *yr, hipStream_t stream)
{
    if (!yr) { set_error("Input mismatch: y is null"); return 1; }
    return launch_lane_gather(g, L, plan, n, nplanes, [&](auto cfg, const dim3 &blocks, const LanePlan &p) {
        using C = decltype(cfg);
        hipLaunchKernelGGL((interp_grad_kernel<C::DIM, C::W, C::WIDE, true>), blocks, dim3(C::NT), 0, stream, g,
                           p.tile_offsets, p.perm, p.spos, grid, (int)Cr, (int)plane0, w, n, part, yr);
    });
}

int launch_interp_hvp(const Geom &g, const PlanLayout &L, const void *plan, const float *grid, int64_t n, int64_t Cr,
                      int64_t plane0, int64_t nplanes, const float *w, const float *v, float *dw, float *part,
                      hipStream_t stream)
{
    if (!dw && !part) return 0;
    return launch_lane_gather(g, L, plan, n, nplanes, [&](auto cfg, const dim3 &blocks, const LanePlan &p) {
        using C = decltype(cfg);
        hipLaunchKernelGGL((interp_hvp_kernel<C::DIM, C::W, C::WIDE>), blocks, dim3(C::NT), 0, stream, g, p.tile_offsets,
                           p.perm, p.spos, grid, (int)Cr, (int)plane0, w, v, n, dw, part);
    });
}

int launch_grad_reduce(const float *part, int64_t len, int64_t Cr, float *dpos, hipStream_t stream)
{
    if (len <= 0) return 0;
    const int64_t blocks = std::min<int64_t>((len + 255) / 256, 4096);
    hipLaunchKernelGGL(grad_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, part, len, (int)Cr, dpos);
    NFFT_HIP_CHECK(hipGetLastError());
    return 0;
}

} // namespace nfft
