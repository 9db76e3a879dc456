// Virial tensor of the Ewald sum for the periodic 1/r: the two reductions that the potential and
// field kernels do not do.  For the homogeneous strain A -> A (1 + eps) at fixed fractional coordinates,
// W_ab = -dU / d eps_ab is the sum of a pair part, a spectral part and the background term (added by the host side):
//
//     near[b, 0, c]  = 1/2 sum_{i in set b} x_ic sum_{j: 0 < r_ij < r_c} erfc(alpha r_ij) / r_ij  x_jc          (energy)
//     near[b, e, c]  = 1/2 sum_i x_ic sum_j (-g(r_ij^2)) d_ij,a d_ij,b x_jc,   e = 1 .. 6: ab = xx, yy, zz, yz, xz, xy
//     far[b, 0, c]   = 1/2 sum_k b_k |band_k|^2                                                                  (energy)
//     far[b, e, c]   = 1/2 sum_k b_k |band_k|^2 (delta_ab - 2 (1 / |kappa|^2 + pi^2 / alpha^2) kappa_a kappa_b)
//
// with g = K'(r) / r for K = erfc(alpha r) / r, d_ij = (ds - rint(ds)) A and kappa = A^-1 k, as in ewald_near.hip.
//
// ewald_virial_near_kernel  on the frame of pair_frame.h like ewald_near_kernel<CC, true, true> -- the same items, lanes, LDS
//                           tiles, 27-cell walk, image, branch and pair weights -- with seven sums per column in place of
//                           four and no store per point: at the
//                           end a lane multiplies its sums by x_i / 2 of its own target (exactly zero for a lane without
//                           one), in float64 from there on, and the workgroup adds its lanes: a butterfly inside each
//                           wave, then the waves in order.  One partial [7, Cr] float64 per item slot.
// ewald_virial_far_kernel   one thread per grid cell, the columns innermost as stored: kappa from the index, the seven
//                           weights in float64 once per cell, |band|^2 per column, float64 sums per thread, the same
//                           workgroup sum.  One partial [7, C] per workgroup.  Cells with b_k = 0 (k = 0, the zeroed
//                           planes k_a = -N/2) are skipped.
// virial_sum_kernel         second level of both: one workgroup per (point set, column) adds that set's partials, each
//                           thread a fixed stride of them in order, then the workgroup sum.
//
// The second level, the workspaces and their layout also serve the dispersion sum's virial (ewald_disp_virial.hip, section
// 7k) through launch_virial_sum, ewald_virial_near_item_slots / _partials and ewald_virial_far_blocks.
//
// No atomics anywhere and every order of addition is fixed by the launch geometry: two calls give the same bits.
#include "host_util.h"
#include "pair_frame.h"

namespace nfft {

namespace {

constexpr int kVirialTerms = 7;    // energy, xx, yy, zz, yz, xz, xy
constexpr int kVirialBlock = 256;  // lanes of the far kernel and of the second level
constexpr int kVirialFarBlocks = 1024;  // workgroups per point set of the far kernel, at most

template <int CC>
__global__ void __launch_bounds__(kNearBlock) ewald_virial_near_kernel(EwaldPairParams q, const int2 *__restrict__ items,
                                                                       const float *__restrict__ pos,
                                                                       const float *__restrict__ xr,
                                                                       const int *__restrict__ start,
                                                                       double *__restrict__ partial)
{
    __shared__ float4 s_pos[kNearTile];
    __shared__ __attribute__((aligned(16))) float s_x[kNearTile * CC];
    __shared__ double s_red[kNearBlock / 64][kVirialTerms * CC];
    const int2 item = items[blockIdx.x];
    if (item.x < 0) return;  // (uniform: an empty slot; the second level skips it)
    const PairLane lane = pair_lane(item, start);
    const WrappedWalk walk(lane.cell, q.G0, q.G1, q.G2);
    // (a lane without a target sums pairs of the origin; its sums are replaced by zero before the reduction)
    const float4 t = lane_position(lane, pos, 3, 0.f);
    for (int64_t col0 = 0; col0 < q.Cr; col0 += CC) {
        float acc[kVirialTerms][CC];
#pragma unroll
        for (int e = 0; e < kVirialTerms; ++e)
#pragma unroll
            for (int c = 0; c < CC; ++c) acc[e][c] = 0.f;
        const StageColumns<CC> stage = {s_x, xr, q.Cr, col0};
        walk(start, [&](int first, int last) {
            sweep_range<2>(first, last, lane, s_pos, pos, 3, stage, [&](int j) {
                const PairSep d = ewald_image<true>(t, s_pos[j], q);
                // the lanes that fail the test sit the expansion out
                if (!(d.rr > 0.f && d.rr < q.rc2)) return;
                const EwaldPairWeight e(d.rr, q);
                const float w = e.w, mg = e.mg(q);
                const float gx = mg * d.dx, gy = mg * d.dy, gz = mg * d.dz;
                const float pxx = gx * d.dx, pyy = gy * d.dy, pzz = gz * d.dz;
                const float pyz = gy * d.dz, pxz = gx * d.dz, pxy = gx * d.dy;
#pragma unroll
                for (int c = 0; c < CC; ++c) {
                    const float v = s_x[j * CC + c];
                    acc[0][c] += w * v;
                    acc[1][c] += pxx * v;
                    acc[2][c] += pyy * v;
                    acc[3][c] += pzz * v;
                    acc[4][c] += pyz * v;
                    acc[5][c] += pxz * v;
                    acc[6][c] += pxy * v;
                }
            });
        });
        // x_i / 2 of the lane's own target, float64 from here on; a lane without a target adds exactly zero
        double red[kVirialTerms * CC];
#pragma unroll
        for (int c = 0; c < CC; ++c) {
            const bool live = lane.active && col0 + c < q.Cr;
            const double h = live ? 0.5 * (double)xr[(int64_t)lane.ti * q.Cr + col0 + c] : 0.0;
#pragma unroll
            for (int e = 0; e < kVirialTerms; ++e) red[e * CC + c] = live ? h * (double)acc[e][c] : 0.0;
        }
        const double v = block_sum_f64(red, s_red);
        const int tid = threadIdx.x;
        if (tid < kVirialTerms * CC) {
            const int e = tid / CC, c = tid % CC;
            if (col0 + c < q.Cr) partial[((int64_t)blockIdx.x * kVirialTerms + e) * q.Cr + col0 + c] = v;
        }
    }
}

struct VirialFarParams {
    int N, blocks;  // frequencies per axis; workgroups per point set
    int wide;       // band is 16-byte aligned: a cell of two or four columns is read with 16-byte loads
    int64_t C;
    double i00, i10, i11, i20, i21, i22;  // the lower triangle of A^-1
    double p2a2;                          // pi^2 / alpha^2
};

template <int CC>
__global__ void __launch_bounds__(kVirialBlock) ewald_virial_far_kernel(VirialFarParams q, const float2 *__restrict__ band,
                                                                        const float *__restrict__ coeffs,
                                                                        double *__restrict__ partial)
{
    __shared__ double s_red[kVirialBlock / 64][kVirialTerms * CC];
    const int tid = threadIdx.x;
    const int N = q.N, half = q.N / 2;
    const int64_t cells = (int64_t)N * N * N;
    const int set = blockIdx.x / q.blocks, blk = blockIdx.x % q.blocks;  // (point set, workgroup within it)
    const float2 *bb = band + (int64_t)set * cells * q.C;
    for (int64_t col0 = 0; col0 < q.C; col0 += CC) {
        double acc[kVirialTerms * CC];
#pragma unroll
        for (int n = 0; n < kVirialTerms * CC; ++n) acc[n] = 0.0;
        // the cells blk * 256 + tid, + stride, + 2 stride, ...: their index (i0, i1, i2) is kept beside them and advanced
        // by the stride's own digits with carries, so that no division runs per cell
        const int stride = q.blocks * kVirialBlock;
        const unsigned first = (unsigned)blk * kVirialBlock + tid;
        int i2 = (int)(first % (unsigned)N), i1 = (int)((first / (unsigned)N) % (unsigned)N), i0 = (int)(first / ((unsigned)N * N));
        const int s2 = stride % N, s1 = (stride / N) % N, s0 = stride / (N * N);
        for (int64_t cell = first; cell < cells; cell += stride) {
            const float bk = coeffs[cell];
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
            if (bk == 0.f) continue;  // k = 0 and the zeroed planes k_a = -N/2
            // kappa = A^-1 k, A^-1 lower triangular
            const double kx = q.i00 * k0;
            const double ky = q.i10 * k0 + q.i11 * k1;
            const double kz = q.i20 * k0 + q.i21 * k1 + q.i22 * k2;
            const double kk = kx * kx + ky * ky + kz * kz;
            const double b = (double)bk;
            const double t = -2.0 * (1.0 / kk + q.p2a2) * b;
            double wgt[kVirialTerms];
            wgt[0] = b;
            wgt[1] = b + t * kx * kx;
            wgt[2] = b + t * ky * ky;
            wgt[3] = b + t * kz * kz;
            wgt[4] = t * ky * kz;
            wgt[5] = t * kx * kz;
            wgt[6] = t * kx * ky;
            float2 v[CC];
            const float2 *bp = bb + cell * q.C + col0;
            bool loaded = false;
            if constexpr (CC == 2) {
                if (q.C == 2 && q.wide) {  // (16 bytes per cell, aligned: one load)
                    const float4 u = *reinterpret_cast<const float4 *>(bp);
                    v[0] = make_float2(u.x, u.y);
                    v[1] = make_float2(u.z, u.w);
                    loaded = true;
                }
            }
            if constexpr (CC == 4) {
                if (q.C == 4 && q.wide) {  // (32 bytes per cell, aligned: two loads)
                    const float4 u0 = reinterpret_cast<const float4 *>(bp)[0], u1 = reinterpret_cast<const float4 *>(bp)[1];
                    v[0] = make_float2(u0.x, u0.y);
                    v[1] = make_float2(u0.z, u0.w);
                    v[2] = make_float2(u1.x, u1.y);
                    v[3] = make_float2(u1.z, u1.w);
                    loaded = true;
                }
            }
            if (!loaded) {
#pragma unroll
                for (int c = 0; c < CC; ++c) v[c] = col0 + c < q.C ? bp[c] : make_float2(0.f, 0.f);
            }
#pragma unroll
            for (int c = 0; c < CC; ++c) {
                const double p = (double)v[c].x * (double)v[c].x + (double)v[c].y * (double)v[c].y;
#pragma unroll
                for (int e = 0; e < kVirialTerms; ++e) acc[e * CC + c] += wgt[e] * p;
            }
        }
        const double v = block_sum_f64(acc, s_red);
        if (tid < kVirialTerms * CC) {
            const int e = tid / CC, c = tid % CC;
            if (col0 + c < q.C) partial[((int64_t)blockIdx.x * kVirialTerms + e) * q.C + col0 + c] = 0.5 * v;
        }
    }
}

// out[b, e, c] = sum of partial[row, e, c] over the rows of point set b, column c (one workgroup each,
// blockIdx.x = b C + c), e < terms: seven here and in the sums that share this level, eight in ewald_lj_step.hip (section 7r).
// items == nullptr: the rows are b * rows_per_set ... (b + 1) * rows_per_set.  Otherwise the rows are the item slots of the
// set's cells: slot = first point / kNearBlock + cell + piece grows with the cell, so they are the slots from that of the
// set's first cell up to that of the next set's first cell.  The last slot of a cell lies before the first slot of the next
// cell, so that range holds items of set b (item.x / cells_per_set == b) and empty slots (item.x < 0, skipped), no others.
__global__ void __launch_bounds__(kVirialBlock) virial_sum_kernel(const double *__restrict__ partial, int terms, int64_t C,
                                                                  int rows_per_set, const int2 *__restrict__ items,
                                                                  const int *__restrict__ start, int cells_per_set,
                                                                  double *__restrict__ out)
{
    __shared__ double s_red[kVirialBlock / 64][1];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x / C, c = blockIdx.x % C;
    int64_t lo, hi;
    if (items) {
        const int64_t k0 = b * cells_per_set, k1 = (b + 1) * cells_per_set;
        lo = start[k0] / kNearBlock + k0;
        hi = start[k1] / kNearBlock + k1;
    } else {
        lo = b * rows_per_set;
        hi = lo + rows_per_set;
    }
    for (int e = 0; e < terms; ++e) {
        double v = 0.0;
        for (int64_t row = lo + tid; row < hi; row += kVirialBlock) {
            if (items) {
                const int cell = items[row].x;
                if (cell < 0) continue;
            }
            v += partial[(row * terms + e) * C + c];
        }
        const double sum[1] = {v};
        const double r = block_sum_f64(sum, s_red);
        if (tid == 0) out[(b * terms + e) * C + c] = r;
    }
}

int64_t virial_cells(const nfft_hip_ewald_box_problem *p)
{
    return p->batch_size * p->cells[0] * p->cells[1] * p->cells[2];
}

int virial_far_blocks(int64_t N)
{
    const int64_t cells = N * N * N;
    return (int)std::min<int64_t>((cells + kVirialBlock - 1) / kVirialBlock, kVirialFarBlocks);
}

}  // namespace

int ewald_virial_far_blocks(int64_t N) { return virial_far_blocks(N); }

// the second level on `partial` [rows, terms, C]: out [batch_size, terms, C]; the rows of a point set as virial_sum_kernel
// takes them
int launch_virial_sum_terms(const double *partial, int terms, int64_t batch_size, int64_t C, int rows_per_set, const void *items,
                            const int *start, int cells_per_set, double *out, hipStream_t stream)
{
    hipLaunchKernelGGL(virial_sum_kernel, dim3((unsigned)(batch_size * C)), dim3(kVirialBlock), 0, stream, partial, terms, C,
                       rows_per_set, (const int2 *)items, start, cells_per_set, out);
    NFFT_HIP_CHECK(hipGetLastError());
    return 0;
}

// ... with the seven terms of a virial
int launch_virial_sum(const double *partial, int64_t batch_size, int64_t C, int rows_per_set, const void *items, const int *start,
                      int cells_per_set, double *out, hipStream_t stream)
{
    return launch_virial_sum_terms(partial, kVirialTerms, batch_size, C, rows_per_set, items, start, cells_per_set, out, stream);
}

int64_t ewald_virial_near_item_slots(const nfft_hip_ewald_box_problem *p)
{
    return nearfield_item_slots(virial_cells(p), p->num_points);
}

int64_t ewald_virial_near_workspace(const nfft_hip_ewald_box_problem *p)
{
    const int64_t slots = ewald_virial_near_item_slots(p);
    return round256(slots * (int64_t)sizeof(int2)) + slots * kVirialTerms * p->num_columns * (int64_t)sizeof(double);
}

// the near workspace: the work items, then (256-byte aligned) one partial per item slot
double *ewald_virial_near_partials(const nfft_hip_ewald_box_problem *p, void *workspace)
{
    return (double *)((char *)workspace + round256(ewald_virial_near_item_slots(p) * (int64_t)sizeof(int2)));
}

int launch_ewald_virial_near(const nfft_hip_ewald_box_problem *p, const float *pos, const float *xr, const int *start,
                             double *out, void *workspace, hipStream_t stream)
{
    const EwaldPairParams q = ewald_pair_params(p->cells[0], p->cells[1], p->cells[2], p->num_columns, p->alpha, p->r_cut, p->box);
    const int64_t slots = ewald_virial_near_item_slots(p);
    int2 *items = (int2 *)workspace;
    double *partial = ewald_virial_near_partials(p, workspace);
    if (int rc = launch_nearfield_items(virial_cells(p), p->num_points, start, items, stream)) return rc;
    const dim3 grid((unsigned)slots), block(kNearBlock);
    dispatch_columns(q.Cr, [&](auto CC) {
        hipLaunchKernelGGL((ewald_virial_near_kernel<CC()>), grid, block, 0, stream, q, (const int2 *)items, pos, xr, start,
                           partial);
    });
    NFFT_HIP_CHECK(hipGetLastError());
    return launch_virial_sum(partial, p->batch_size, q.Cr, 0, items, start, (int)(p->cells[0] * p->cells[1] * p->cells[2]), out,
                             stream);
}

int64_t ewald_virial_far_workspace(int64_t N, int64_t batch_size, int64_t num_columns)
{
    return batch_size * virial_far_blocks(N) * kVirialTerms * num_columns * (int64_t)sizeof(double);
}

int launch_ewald_virial_far(int64_t N, int64_t batch_size, int64_t num_columns, const void *band, const float *coeffs,
                            const double *box_inverse, double pi2_over_alpha2, double *out, void *workspace,
                            hipStream_t stream)
{
    VirialFarParams q;
    q.N = (int)N;
    q.blocks = virial_far_blocks(N);
    q.C = num_columns;
    q.wide = ((uintptr_t)band & 15) == 0 ? 1 : 0;  // (otherwise 8-byte loads, which complex64 data always allows)
    q.i00 = box_inverse[0];
    q.i10 = box_inverse[1];
    q.i11 = box_inverse[2];
    q.i20 = box_inverse[3];
    q.i21 = box_inverse[4];
    q.i22 = box_inverse[5];
    q.p2a2 = pi2_over_alpha2;
    double *partial = (double *)workspace;
    const dim3 grid((unsigned)(q.blocks * batch_size)), block(kVirialBlock);
    dispatch_columns(q.C, [&](auto CC) {
        hipLaunchKernelGGL((ewald_virial_far_kernel<CC()>), grid, block, 0, stream, q, (const float2 *)band, coeffs, partial);
    });
    NFFT_HIP_CHECK(hipGetLastError());
    return launch_virial_sum(partial, batch_size, q.C, q.blocks, nullptr, nullptr, 0, out, stream);
}

}  // namespace nfft
