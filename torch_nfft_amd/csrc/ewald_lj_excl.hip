// Bonded-pair exclusions of the Lennard-Jones + Coulomb step.  The list is ExclusionList's CSR matrix
// over the points in the CALLER's order -- row_start [n + 1], col [entries] ascending within a row, two weights [entries]
// holding w = 1 - s for the Coulomb scale s^C and the Lennard-Jones scale s^L (both powers).  A listed pair's terms are
// SCALED by s before they reach an accumulator; the bounded smooth share that the far field has added is taken out by the
// list kernel.  Nothing of the size of 1/r, 1/r^6 or 1/r^12 of a bonded pair is formed and cancelled.
//
// The masked pair walk is step_near_kernel<LjProductLaw, true> (step_frame.h, ewald_lj_step.hip).  Here:
//
// lj_excl_list_kernel    ewald_excl_kernel's lane per point in the caller's order on the positions reduced by torus_reduce
//                        (the image carries the sweep's bits, so both kernels agree on which side of r_c a pair lies), in
//                        row order, three float32 force sums per lane; and ewald_excl_virial_kernel's pair-once (col > row)
//                        float64 sums of the eight terms over the workgroup: a workgroup takes every blocks-th tile of 256
//                        points of ONE point set.  Per entry, with rr < rc2 (rr = 0 included) the smooth parts
//                            S_C = erf(alpha r) / r,          T_C = (erf(alpha r) / r - (2 alpha / sqrt(pi)) e^(-alpha^2 r^2)) / r^2,
//                            S_D = alpha^6 h(u),              T_D = -2 alpha^8 h'(u),     u = alpha^2 r^2,
//                            h(u) = (1 - e^-u (1 + u + u^2 / 2)) / u^3
//                        and with rr >= rc2, where the sweep added nothing, the full 1/r, 1/r^3, 1/r^6, 6/r^8.  The weights
//                        are formed in float64; below u = kSeriesSwitch the closed forms cancel and a series of
//                        kSeriesTerms terms takes their place (section 7s has the comparison).  Every value is bounded by
//                        its limit at r = 0: 2 alpha / sqrt(pi), 4 alpha^3 / (3 sqrt(pi)), alpha^6 / 6, alpha^8 / 4.
//                        It writes what to ADD: lf_i = -sum_k (w^C q_i q_j T_C - w^L c_i c_j T_D) d and the eight sums
//                        (-w^C qq S_C, +w^L cc S_D, -g d_a d_b).
//
// Entries whose column lies outside [0, n) and row bounds outside [0, entries] are skipped, not trusted.  The second level
// is launch_virial_sum_terms of ewald_virial.hip with eight terms.  No atomics anywhere: two calls give the same bits.
#include "step_frame.h"

namespace nfft {

namespace {

constexpr int kLjTerms = kStepTerms;
constexpr int kLjValues = 3;  // q, c, a
constexpr int kListBlock = 256;
constexpr int kListBlocks = 1024;          // workgroups per point set of the list kernel, at most
constexpr double kSeriesSwitch = 0.125;    // u = alpha^2 r^2 below which the series run
constexpr int kSeriesTerms = 8;

struct ListParams {
    int blocks;            // workgroups per point set
    double alpha_c, alpha_d;
    double slope_c;        // 2 alpha_C / sqrt(pi)
};

// sum_{k < kSeriesTerms} coef(k) (-u)^k by Horner, coef from a table
__device__ __forceinline__ double series(const double (&coef)[kSeriesTerms], double u)
{
    double t = coef[kSeriesTerms - 1];
#pragma unroll
    for (int k = kSeriesTerms - 2; k >= 0; --k) t = coef[k] - u * t;
    return t;
}

struct ListWeights {
    double SC, TC, SD, TD;
};

// the share of a listed pair that the far field (rr < rc2: the smooth parts) or the definition (rr >= rc2: everything)
// has to lose: S_C, T_C at alpha_C and S_D, T_D at alpha_D, from rr = r^2 >= 0 with the sweep's bits.  A call, not inline,
// with values in and out: inlined into the entry loop the float64 erf and exp take more scalar registers than there are
__device__ __noinline__ ListWeights list_weights(float rrf, float rc2, double alpha_c, double alpha_d, double slope_c)
{
    double SC, TC, SD, TD;
    const double rr = (double)rrf;
    if (!(rrf < rc2)) {  // (beyond the cut: rr > 0)
        const double ir2 = 1.0 / rr, ir = sqrt(ir2);
        SC = ir;
        TC = ir * ir2;
        SD = ir2 * ir2 * ir2;
        TD = 6.0 * SD * ir2;
        return {SC, TC, SD, TD};
    }
    // 1 / (k! (2k + 1)) and (2 (k + 1) / (2 k + 3)) / (k + 1)!: erf(x) / x and (erf(x) / x - e^(-x^2)) / x^2 over 2 / sqrt(pi)
    const double c0[kSeriesTerms] = {1.0, 1.0 / 3, 1.0 / 10, 1.0 / 42, 1.0 / 216, 1.0 / 1320, 1.0 / 9360, 1.0 / 75600};
    const double c1[kSeriesTerms] = {2.0 / 3, 2.0 / 5, 1.0 / 7, 1.0 / 27, 1.0 / 132, 1.0 / 780, 1.0 / 5400, 1.0 / 42840};
    // 1 / (2 k! (k + 3)) and 1 / (2 k! (k + 4)): h(u) and -h'(u)
    const double h0[kSeriesTerms] = {1.0 / 6, 1.0 / 8, 1.0 / 20, 1.0 / 72, 1.0 / 336, 1.0 / 1920, 1.0 / 12960, 1.0 / 100800};
    const double h1[kSeriesTerms] = {1.0 / 8, 1.0 / 10, 1.0 / 24, 1.0 / 84, 1.0 / 384, 1.0 / 2160, 1.0 / 14400, 1.0 / 110880};
    {
        const double a2 = alpha_c * alpha_c, u = a2 * rr;
        if (u < kSeriesSwitch) {
            SC = slope_c * series(c0, u);
            TC = slope_c * a2 * series(c1, u);
        } else {
            const double ir2 = 1.0 / rr, ir = sqrt(ir2);
            SC = erf(alpha_c * (rr * ir)) * ir;
            TC = (SC - slope_c * exp(-u)) * ir2;
        }
    }
    {
        const double a2 = alpha_d * alpha_d, a6 = a2 * a2 * a2, u = a2 * rr;
        if (u < kSeriesSwitch) {
            SD = a6 * series(h0, u);
            TD = 2.0 * a6 * a2 * series(h1, u);
        } else {
            const double e = exp(-u), iu = 1.0 / u;
            const double h = (1.0 - e * (1.0 + u + 0.5 * u * u)) * (iu * iu * iu);
            SD = a6 * h;
            TD = a6 * a2 * (6.0 * h - e) * iu;
        }
    }
    return {SC, TC, SD, TD};
}

__global__ void __launch_bounds__(kListBlock) lj_excl_list_kernel(EwaldPairParams q, ListParams l, ExclList ex,
                                                                  const float *__restrict__ pos, const float *__restrict__ xs,
                                                                  const int *__restrict__ set_start, float *__restrict__ f,
                                                                  double *__restrict__ partial)
{
    __shared__ double s_red[kListBlock / 64][kLjTerms];
    const int tid = threadIdx.x;
    const int set = blockIdx.x / l.blocks, blk = blockIdx.x % l.blocks;  // (point set, workgroup within it)
    const int lo = set_start ? max(set_start[set], 0) : 0;
    const int hi = set_start ? min(set_start[set + 1], ex.n) : ex.n;
    double acc[kLjTerms];
#pragma unroll
    for (int m = 0; m < kLjTerms; ++m) acc[m] = 0.0;
    for (int64_t i = (int64_t)lo + blk * kListBlock + tid; i < hi; i += (int64_t)l.blocks * kListBlock) {
        const int first = max(ex.row_start[i], 0), last = min(ex.row_start[i + 1], ex.entries);
        float fx = 0.f, fy = 0.f, fz = 0.f;
        if (first < last) {
            const float4 t = load_position(pos, i, 3);
            const double qi = (double)xs[i * kLjValues], ci = (double)xs[i * kLjValues + 1];
            for (int k = first; k < last; ++k) {
                const int j = ex.col[k];
                if ((unsigned)j >= (unsigned)ex.n) continue;
                const PairSep d = ewald_image<true>(t, load_position(pos, j, 3), q);
                const ListWeights lw = list_weights(d.rr, q.rc2, l.alpha_c, l.alpha_d, l.slope_c);
                const double SC = lw.SC, TC = lw.TC, SD = lw.SD, TD = lw.TD;
                const double wqq = (double)ex.wc[k] * qi * (double)xs[(int64_t)j * kLjValues];
                const double wcc = (double)ex.wl[k] * ci * (double)xs[(int64_t)j * kLjValues + 1];
                const double g = wcc * TD - wqq * TC;  // what to ADD to the pair's slope
                const double dx = d.dx, dy = d.dy, dz = d.dz;
                const double gx = g * dx, gy = g * dy, gz = g * dz;
                fx += (float)gx;
                fy += (float)gy;
                fz += (float)gz;
                if (j <= i) continue;  // each pair once, from its lower end
                acc[0] -= wqq * SC;
                acc[1] += wcc * SD;
                acc[2] += gx * dx;
                acc[3] += gy * dy;
                acc[4] += gz * dz;
                acc[5] += gy * dz;
                acc[6] += gx * dz;
                acc[7] += gx * dy;
            }
        }
        f[i * 3 + 0] = fx;
        f[i * 3 + 1] = fy;
        f[i * 3 + 2] = fz;
    }
    const double v = block_sum_f64(acc, s_red);
    if (tid < kLjTerms) partial[(int64_t)blockIdx.x * kLjTerms + tid] = v;
}

ExclList excl_list(const nfft_hip_ewald_box_problem *p, int64_t entries, const int *row_start, const int *col, const float *wc,
                   const float *wl)
{
    return {row_start, col, wc, wl, (int)p->num_points, (int)entries};
}

// workgroups per point set: one per tile of 256 points of an average set, kListBlocks at most
int list_blocks(const nfft_hip_ewald_box_problem *p)
{
    const int64_t per_set = (p->num_points + p->batch_size - 1) / p->batch_size;
    return (int)std::max<int64_t>(1, std::min<int64_t>((per_set + kListBlock - 1) / kListBlock, kListBlocks));
}

}  // namespace

int64_t ewald_lj_excl_list_workspace(const nfft_hip_ewald_box_problem *p)
{
    return p->batch_size * list_blocks(p) * kLjTerms * (int64_t)sizeof(double);
}

int launch_ewald_lj_excl_list(const nfft_hip_ewald_box_problem *p, double alpha_dispersion, int64_t num_entries, const float *pos,
                              const float *xs, const int *row_start, const int *col, const float *weight_coulomb,
                              const float *weight_lj, const int *set_start, float *f, double *out, void *workspace,
                              hipStream_t stream)
{
    const EwaldPairParams q = ewald_pair_params(p->cells[0], p->cells[1], p->cells[2], kLjValues, p->alpha, p->r_cut, p->box);
    const ExclList ex = excl_list(p, num_entries, row_start, col, weight_coulomb, weight_lj);
    ListParams l;
    l.blocks = list_blocks(p);
    l.alpha_c = p->alpha;
    l.alpha_d = alpha_dispersion;
    l.slope_c = 2.0 * p->alpha / 1.7724538509055160273;
    double *partial = (double *)workspace;
    hipLaunchKernelGGL(lj_excl_list_kernel, dim3((unsigned)(p->batch_size * l.blocks)), dim3(kListBlock), 0, stream, q, l, ex, pos, xs,
                       set_start, f, partial);
    NFFT_HIP_CHECK(hipGetLastError());
    return launch_virial_sum_terms(partial, kLjTerms, p->batch_size, 1, l.blocks, nullptr, nullptr, 0, out, stream);
}

}  // namespace nfft
