// Virial tensor of the dispersion Ewald sum, the periodic 1/r^6: the two reductions of
// ewald_virial.hip (section 7i) with the weights of the dispersion split (section 7j).  For the homogeneous strain
// A -> A (1 + eps) at fixed fractional coordinates, W_ab = -dU / d eps_ab of U = 1/2 sum_i c_i psi_i is a pair part and a
// spectral part (the self term has no strain in it and there is no background: the host side adds the self term to U):
//
//     near[b, 0, c]  = 1/2 sum_{i in set b} x_ic sum_{j: 0 < r_ij < r_c} w(r_ij) x_jc                            (energy)
//     near[b, e, c]  = 1/2 sum_i x_ic sum_j mg(r_ij) d_ij,a d_ij,b x_jc,   e = 1 .. 6: ab = xx, yy, zz, yz, xz, xy
//     far[b, 0, c]   = 1/2 sum_k b_k |band_k|^2                                                                  (energy)
//     far[b, e, c]   = 1/2 sum_k |band_k|^2 (b_k delta_ab + t_k kappa_a kappa_b)
//
// with w and mg = -w'(r) / r of DispersionPairWeight, d_ij = (ds - rint(ds)) A and kappa = A^-1 k as in ewald_disp.hip, and
// t_k = (d b_k / d |kappa|) / |kappa| <= 0 read from a grid of its own that the host side evaluated in float64 (its two
// terms cancel at large |kappa|; finite at k = 0, where it multiplies kappa kappa = 0).  The k = 0 term of b_k is kept.
//
// Both reductions are the frames' (DESIGN.md section 7w), and nothing but the policies is left here:
// virial_near_kernel<CC, DispersionVirialWeight>  of virial_frame.h (until 7w: ewald_disp_virial_near_kernel<CC>).
// virial_far_kernel<CC, TableStrain>              of spectral_frame.h: one more 4-byte load per cell (t_k) in place of the
//                                                 Coulomb sum's closed form (until 7w: ewald_disp_virial_far_kernel<CC>).
// The second level, the workspaces and their layout are those of ewald_virial.hip.
#include "spectral_frame.h"

namespace nfft {

namespace {

// the pair weight of the dispersion sum (virial_frame.h has what a weight is): DispersionPairWeight, no block of its own
struct DispersionVirialWeight {
    struct Params {};
    static __device__ __forceinline__ void weights(float rr, const EwaldPairParams &q, const Params &, float &w, float &mg)
    {
        const DispersionPairWeight e(rr, q);
        w = e.w;
        mg = e.mg();
    }
};

}  // namespace

int launch_ewald_dispersion_virial_near(const nfft_hip_ewald_box_problem *p, const float *pos, const float *xr, const int *start,
                                        double *out, void *workspace, hipStream_t stream)
{
    return launch_virial_near<DispersionVirialWeight>(p, {}, pos, xr, start, out, workspace, stream);
}

int launch_ewald_dispersion_virial_far(int64_t N, int64_t batch_size, int64_t num_columns, const void *band, const float *coeffs,
                                       const float *strain_coeffs, const double *box_inverse, double *out, void *workspace,
                                       hipStream_t stream)
{
    return launch_virial_far(N, batch_size, num_columns, band, coeffs, box_inverse, TableStrain{strain_coeffs}, out, workspace, stream);
}

}  // namespace nfft
