// Bonded-pair exclusions of the Coulomb and the dispersion Ewald sums: what the listed pairs {i, j}
// take back out of the periodic sums.  The list comes symmetrised and sorted as a CSR matrix -- row_start [n + 1], col [2 m],
// weight [2 m] = 1 - scale -- over the points in the CALLER's order, and for one point set on both sides
//
//     z[i, c]    = sum_{k in row i} weight[k] K0(r) xr[col[k], c]               K0 = 1 / r    (Coulomb),  1 / r^6    (dispersion)
//     f[i, a, c] = sum_{k in row i} weight[k] K1(r) d[a] xr[col[k], c]          K1 = 1 / r^3  (Coulomb),  6 / r^8    (dispersion)
//
// with d the image of pos_i - pos_col[k] that ewald_image<BOX> of pair_frame.h forms -- the very routine of the pair sweeps,
// on positions reduced to [-1/2, 1/2)^3 by the very expression that their binning uses, so d and r = |d| carry the bits the
// sweep saw and the singular terms cancel to the rounding of the sweep's accumulator.  A listed pair at r = 0 takes the limit
// of the smooth part that the far field has added, K0 = 2 alpha / sqrt(pi) or alpha^6 / 6, and no field.  The caller
// subtracts z and f.
//
// ewald_excl_kernel         one lane per point, a wave owns 64 consecutive rows; the lane reads its two row_start entries once
//                           and walks its row: one col, one weight, one gathered position and CC gathered values per entry,
//                           1 or 4 float32 sums per column in registers, in row order.  No LDS, no atomics: two calls give the
//                           same bits.  Bound by the latency of the gathers, not by the VALU.
// ewald_excl_virial_kernel  the listed pairs' share of the energy and of the virial, each pair once (col > row), seven float64
//                           sums per column: a workgroup takes every blocks-th tile of 256 points of ONE point set in order,
//                           then adds its lanes (block_sum_f64).  One partial [7, Cr] per workgroup; the second level is
//                           launch_virial_sum of ewald_virial.hip.  No atomics, every order fixed by the launch geometry.
//
// Entries whose column lies outside [0, n) and row bounds outside [0, entries] are skipped, not trusted.
#include "pair_frame.h"

namespace nfft {

namespace {

constexpr int kExclBlock = 256;
constexpr int kExclTerms = 7;           // energy, xx, yy, zz, yz, xz, xy
constexpr int kExclVirialBlocks = 1024;  // workgroups per point set of the virial kernel, at most

struct ExclParams {
    int n, entries;  // points; entries of col and weight
    int blocks;      // virial: workgroups per point set
    float zero;      // K0 at r = 0
    double zero64;
};

// (K0, K1) from rr = r^2 of the image
template <int KIND>
__device__ __forceinline__ void excl_weights(float rr, float zero, float &k0, float &k1)
{
    if (!(rr > 0.f)) {
        k0 = zero;
        k1 = 0.f;
    } else if (KIND == NFFT_HIP_EXCL_COULOMB) {
        const float ir = rsqrtf(rr);  // (as EwaldPairWeight)
        k0 = ir;
        k1 = ir * (ir * ir);
    } else {
        const float ir2 = __builtin_amdgcn_rcpf(rr);  // (as DispersionPairWeight)
        k0 = ir2 * ir2 * ir2;
        k1 = 6.f * (k0 * ir2);
    }
}

template <int CC, int KIND, bool FIELD, bool BOX>
__global__ void __launch_bounds__(kExclBlock) ewald_excl_kernel(EwaldPairParams q, ExclParams e, const float *__restrict__ pos,
                                                                const float *__restrict__ xr,
                                                                const int *__restrict__ row_start, const int *__restrict__ col,
                                                                const float *__restrict__ weight, float *__restrict__ z,
                                                                float *__restrict__ f)
{
    const int i = (int)(blockIdx.x * (unsigned)kExclBlock + threadIdx.x);
    if (i >= e.n) return;
    const int first = max(row_start[i], 0), last = min(row_start[i + 1], e.entries);
    const float4 t = load_position(pos, i, 3);
    for (int64_t col0 = 0; col0 < q.Cr; col0 += CC) {
        float acc[CC];
        float fx[FIELD ? CC : 1], fy[FIELD ? CC : 1], fz[FIELD ? CC : 1];
#pragma unroll
        for (int c = 0; c < CC; ++c) acc[c] = 0.f;
#pragma unroll
        for (int c = 0; c < (FIELD ? CC : 1); ++c) fx[c] = fy[c] = fz[c] = 0.f;
        for (int k = first; k < last; ++k) {
            const int j = col[k];
            if ((unsigned)j >= (unsigned)e.n) continue;
            const float w = weight[k];
            const PairSep d = ewald_image<BOX>(t, load_position(pos, j, 3), q);
            float k0, k1;
            excl_weights<KIND>(d.rr, e.zero, k0, k1);
            const float *xp = xr + (int64_t)j * q.Cr + col0;
            float v[CC];
#pragma unroll
            for (int c = 0; c < CC; ++c) v[c] = col0 + c < q.Cr ? xp[c] : 0.f;
            const float w0 = w * k0;
#pragma unroll
            for (int c = 0; c < CC; ++c) acc[c] += w0 * v[c];
            if (FIELD) {
                const float w1 = w * k1;
                const float gx = w1 * d.dx, gy = w1 * d.dy, gz = w1 * d.dz;
#pragma unroll
                for (int c = 0; c < (FIELD ? CC : 1); ++c) {
                    fx[c] += gx * v[c];
                    fy[c] += gy * v[c];
                    fz[c] += gz * v[c];
                }
            }
        }
        float *zp = z + (int64_t)i * q.Cr + col0;
#pragma unroll
        for (int c = 0; c < CC; ++c)
            if (col0 + c < q.Cr) zp[c] = acc[c];
        if (FIELD) {
            float *fp = f + (int64_t)i * 3 * q.Cr + col0;
#pragma unroll
            for (int c = 0; c < (FIELD ? CC : 1); ++c)
                if (col0 + c < q.Cr) {
                    fp[c] = fx[c];
                    fp[q.Cr + c] = fy[c];
                    fp[2 * q.Cr + c] = fz[c];
                }
        }
    }
}

template <int CC, int KIND>
__global__ void __launch_bounds__(kExclBlock) ewald_excl_virial_kernel(EwaldPairParams q, ExclParams e,
                                                                       const float *__restrict__ pos,
                                                                       const float *__restrict__ xr,
                                                                       const int *__restrict__ row_start,
                                                                       const int *__restrict__ col,
                                                                       const float *__restrict__ weight,
                                                                       const int *__restrict__ set_start,
                                                                       double *__restrict__ partial)
{
    __shared__ double s_red[kExclBlock / 64][kExclTerms * CC];
    const int tid = threadIdx.x;
    const int set = blockIdx.x / e.blocks, blk = blockIdx.x % e.blocks;  // (point set, workgroup within it)
    const int lo = set_start ? max(set_start[set], 0) : 0;
    const int hi = set_start ? min(set_start[set + 1], e.n) : e.n;
    for (int64_t col0 = 0; col0 < q.Cr; col0 += CC) {
        double acc[kExclTerms * CC];
#pragma unroll
        for (int m = 0; m < kExclTerms * CC; ++m) acc[m] = 0.0;
        for (int64_t i = (int64_t)lo + blk * kExclBlock + tid; i < hi; i += (int64_t)e.blocks * kExclBlock) {
            const int first = max(row_start[i], 0), last = min(row_start[i + 1], e.entries);
            if (first >= last) continue;
            const float4 t = load_position(pos, i, 3);
            double xi[CC];
#pragma unroll
            for (int c = 0; c < CC; ++c) xi[c] = col0 + c < q.Cr ? (double)xr[i * q.Cr + col0 + c] : 0.0;
            for (int k = first; k < last; ++k) {
                const int j = col[k];
                if (j <= i || j >= e.n) continue;  // each pair once, from its lower end
                const PairSep d = ewald_image<true>(t, load_position(pos, j, 3), q);
                const double w = (double)weight[k];
                double u, g = 0.0;
                if (!(d.rr > 0.f)) {
                    u = w * e.zero64;  // (the smooth part's limit: no strain in it)
                } else if (KIND == NFFT_HIP_EXCL_COULOMB) {
                    const double ir2 = 1.0 / (double)d.rr, ir = sqrt(ir2);
                    u = w * ir;
                    g = u * ir2;
                } else {
                    const double ir2 = 1.0 / (double)d.rr;
                    u = w * (ir2 * ir2 * ir2);
                    g = 6.0 * u * ir2;
                }
                const double dx = d.dx, dy = d.dy, dz = d.dz;
                const double gx = g * dx, gy = g * dy, gz = g * dz;
                const double pxx = gx * dx, pyy = gy * dy, pzz = gz * dz;
                const double pyz = gy * dz, pxz = gx * dz, pxy = gx * dy;
                const float *xp = xr + (int64_t)j * q.Cr + col0;
#pragma unroll
                for (int c = 0; c < CC; ++c) {
                    const double v = col0 + c < q.Cr ? xi[c] * (double)xp[c] : 0.0;
                    acc[0 * CC + c] += u * v;
                    acc[1 * CC + c] += pxx * v;
                    acc[2 * CC + c] += pyy * v;
                    acc[3 * CC + c] += pzz * v;
                    acc[4 * CC + c] += pyz * v;
                    acc[5 * CC + c] += pxz * v;
                    acc[6 * CC + c] += pxy * v;
                }
            }
        }
        const double v = block_sum_f64(acc, s_red);
        if (tid < kExclTerms * CC) {
            const int t7 = tid / CC, c = tid % CC;
            if (col0 + c < q.Cr) partial[((int64_t)blockIdx.x * kExclTerms + t7) * q.Cr + col0 + c] = v;
        }
    }
}

ExclParams excl_params(const nfft_hip_ewald_excl_problem *p, int blocks)
{
    const double pi = 3.14159265358979323846;
    const double a = p->alpha;
    ExclParams e;
    e.n = (int)p->num_points;
    e.entries = (int)p->num_entries;
    e.blocks = blocks;
    e.zero64 = p->kind == NFFT_HIP_EXCL_COULOMB ? 2.0 * a / std::sqrt(pi) : a * a * a * a * a * a / 6.0;
    e.zero = (float)e.zero64;
    return e;
}

template <typename F>
void dispatch_kind(int kind, F &&f)
{
    if (kind == NFFT_HIP_EXCL_COULOMB) f(int_c<NFFT_HIP_EXCL_COULOMB>{});
    else f(int_c<NFFT_HIP_EXCL_DISPERSION>{});
}

template <bool BOX>
int launch_list(const nfft_hip_ewald_excl_problem *p, const float *pos, const float *xr, const int *row_start, const int *col,
                const float *weight, float *z, float *f, hipStream_t stream)
{
    const EwaldPairParams q = ewald_pair_params(3, 3, 3, p->num_columns, p->alpha, 0.0, BOX ? p->box : nullptr);
    const ExclParams e = excl_params(p, 0);
    const dim3 grid((unsigned)((p->num_points + kExclBlock - 1) / kExclBlock)), block(kExclBlock);
    dispatch_kind(p->kind, [&](auto KIND) {
        dispatch_flag(p->with_field != 0, [&](auto FIELD) {
            dispatch_columns(q.Cr, [&](auto CC) {
                hipLaunchKernelGGL((ewald_excl_kernel<CC(), KIND(), FIELD() != 0, BOX>), grid, block, 0, stream, q, e, pos, xr,
                                   row_start, col, weight, z, f);
            });
        });
    });
    NFFT_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace

int launch_ewald_excl(const nfft_hip_ewald_excl_problem *p, const float *pos, const float *xr, const int *row_start,
                      const int *col, const float *weight, float *z, float *f, hipStream_t stream)
{
    return launch_list<false>(p, pos, xr, row_start, col, weight, z, f, stream);
}

int launch_ewald_excl_box(const nfft_hip_ewald_excl_problem *p, const float *pos, const float *xr, const int *row_start,
                          const int *col, const float *weight, float *z, float *f, hipStream_t stream)
{
    return launch_list<true>(p, pos, xr, row_start, col, weight, z, f, stream);
}

// workgroups per point set: one per tile of 256 points of an average set, kExclVirialBlocks at most
static int ewald_excl_virial_blocks(const nfft_hip_ewald_excl_problem *p)
{
    const int64_t per_set = (p->num_points + p->batch_size - 1) / p->batch_size;
    return (int)std::max<int64_t>(1, std::min<int64_t>((per_set + kExclBlock - 1) / kExclBlock, kExclVirialBlocks));
}

int64_t ewald_excl_virial_workspace(const nfft_hip_ewald_excl_problem *p)
{
    return p->batch_size * ewald_excl_virial_blocks(p) * kExclTerms * p->num_columns * (int64_t)sizeof(double);
}

int launch_ewald_excl_virial(const nfft_hip_ewald_excl_problem *p, const float *pos, const float *xr, const int *row_start,
                             const int *col, const float *weight, const int *set_start, double *out, void *workspace,
                             hipStream_t stream)
{
    const EwaldPairParams q = ewald_pair_params(3, 3, 3, p->num_columns, p->alpha, 0.0, p->box);
    const int blocks = ewald_excl_virial_blocks(p);
    const ExclParams e = excl_params(p, blocks);
    double *partial = (double *)workspace;
    const dim3 grid((unsigned)(p->batch_size * blocks)), block(kExclBlock);
    dispatch_kind(p->kind, [&](auto KIND) {
        dispatch_columns(q.Cr, [&](auto CC) {
            hipLaunchKernelGGL((ewald_excl_virial_kernel<CC(), KIND()>), grid, block, 0, stream, q, e, pos, xr, row_start, col,
                               weight, set_start, partial);
        });
    });
    NFFT_HIP_CHECK(hipGetLastError());
    return launch_virial_sum(partial, p->batch_size, q.Cr, blocks, nullptr, nullptr, 0, out, stream);
}

}  // namespace nfft
