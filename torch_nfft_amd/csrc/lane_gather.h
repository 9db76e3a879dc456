// What the one-lane-per-point gathers share: interp_kernel (interp.hip), interp_grad_kernel and interp_hvp_kernel
// (interp_grad.hip) run on one tile geometry (GatherCfg) and one launch shape (launch_lane_gather).
#pragma once
#include <type_traits>

#include "common.h"

namespace nfft {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// Geometry of the lane gathers.  They share the point plan (pencils, chunks of TC planes) with the spreading kernel but
// keep 4-byte cells and rows padded to a multiple of 4 floats so that a lane can fetch its 2m+2 taps of a row with
// aligned ds_read_b128.
template <int DIM_, int W_, bool WIDE_>
struct GatherCfg {
    static constexpr int DIM = DIM_, W = W_;
    static constexpr bool WIDE = WIDE_;
    static constexpr TileCfg tc = tile_cfg(DIM, W, WIDE);
    static constexpr int T1 = tc.T1, T2 = tc.T2, TC = tc.TC;
    static constexpr int W0 = DIM == 3 ? W : 1;
    static constexpr int W1 = DIM >= 2 ? W : 1;
    static constexpr int M0OFF = DIM == 3 ? (W / 2 - 1) : 0;
    static constexpr int NP = TC + W0 - 1;
    static constexpr int P1 = T1 + W1 - 1;
    static constexpr int P2 = T2 + W - 1;
    static constexpr int NR = (W + 3 + 3) / 4;            // aligned 16-byte reads covering any 2m+2 window
    static constexpr int S2 = (P2 + 3 + 3) / 4 * 4;       // row stride (floats): room for the aligned over-read
    static constexpr int S0 = P1 * S2;
    static constexpr int CELLS = NP * S0;
    static constexpr int NT = DIM == 3 ? (WIDE ? 1024 : 512) : 256;  // the wide tiling fills the LDS with one workgroup
    static constexpr int NWAVES = NT / 64;
    // waves per SIMD the register allocation must allow: at least what interp_kernel reaches for the same geometry
    // (without the floor the compiler gives the 1-D / 2-D kernels and the narrow 3-D one of m <= 2 up to 16 more VGPRs)
    static constexpr int WPE = DIM == 1 ? 8 : DIM == 2 ? (W <= 6 ? 8 : W == 10 || W == 18 ? 6 : 7) : (!WIDE && W <= 6) ? 6 : 1;
    // the value-writing kernel: the occupancy the gradient-only kernel reaches.  2-D m = 4: 7 (the floor of 6 would let the
    // allocator take the VGPRs the value needs from it); 2-D m = 1: 7, where the floor of 8 caps the SGPRs below what the
    // y pointer needs -- its 62 VGPRs still give 8 waves.  (2-D m = 2 keeps 8: at 7 it takes 65 VGPRs and loses a wave, at
    // 8 six SGPRs live in VGPR lanes -- v_writelane / v_readlane, no scratch.)
    static constexpr int WPE_VALUE = DIM == 2 && (W == 10 || W == 4) ? 7 : WPE;
    // the second-order gather (interp_hvp_kernel): the gradient kernel's occupancy, except three kernels one wave lower,
    // where its two more moments would otherwise spill VGPRs to scratch (1-D and 2-D m = 8, narrow 3-D m = 2)
    static constexpr int WPE_HVP = DIM == 2 && W == 10 ? 7 : (DIM <= 2 && W == 18) || (DIM == 3 && !WIDE && W == 6) ? WPE - 1 : WPE;
    static_assert(CELLS * 4 <= 160 * 1024, "LDS budget");
};

// The plan arrays a lane gather reads
struct LanePlan {
    const int *tile_offsets;
    const int *perm;
    const float *spos;
};

// Host side of the lane gathers: nothing to do for an empty call; else launch(C{}, blocks, plan) with the configuration
// C = GatherCfg<DIM, W, WIDE> of g (dim, cutoff, tiling) and the grid blocks = (pencil x segment, local plane, point
// split) the kernels decode from blockIdx.
template <class F>
int launch_lane_gather(const Geom &g, const PlanLayout &L, const void *plan, int64_t n, int64_t nplanes, F &&launch)
{
    const char *base = (const char *)plan;
    const LanePlan p{(const int *)(base + L.off_offsets), (const int *)(base + L.off_perm),
                     (const float *)(base + L.off_spos)};
    if (nplanes <= 0 || n <= 0) return 0;
    const int splits = point_splits(g, L, n, nplanes);
    const dim3 blocks((unsigned)(g.nta[1] * g.nta[2] * g.nseg), (unsigned)nplanes, (unsigned)splits);
    const auto for_dim = [&](auto dim) {
        return with_window<8>(g.m, "cutoff m must be in 1..8", [&](auto w) {
            constexpr int DIM = decltype(dim)::value, W = decltype(w)::value;
            if constexpr (DIM == 3) {
                if (g.wide) launch(GatherCfg<DIM, W, true>{}, blocks, p);
                else launch(GatherCfg<DIM, W, false>{}, blocks, p);
            } else {
                launch(GatherCfg<DIM, W, false>{}, blocks, p);
            }
            NFFT_HIP_CHECK(hipGetLastError());
            return 0;
        });
    };
    switch (g.dim) {
    case 1: return for_dim(std::integral_constant<int, 1>{});
    case 2: return for_dim(std::integral_constant<int, 2>{});
    case 3: return for_dim(std::integral_constant<int, 3>{});
    }
    set_error("dim must be 1, 2 or 3");
    return 1;
}

} // namespace nfft
