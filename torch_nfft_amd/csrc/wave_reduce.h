// Reductions over the 64 lanes of a wave that stay in the vector registers.
//
// `for (off = 32; off >= 1; off >>= 1) v = op(v, __shfl_xor(v, off))` compiles on gfx950 to six ds_bpermute_b32, each
// followed by s_waitcnt lgkmcnt(0): six dependent round trips through the LDS pipe, which in the matrix-core gathers is
// the pipe the consumer waves keep busiest.  Here the same reduction is a scan inside each row of 16 lanes (DPP
// row_shr 1, 2, 4, 8), two row broadcasts (row_bcast 15 into rows 1 and 3, row_bcast 31 into rows 2 and 3) and one
// v_readlane of lane 63: six DPP moves, no LDS instruction, and the result is wave-uniform (a scalar register).
//
// Same value as the butterfly, bit for bit: max and min are associative and commutative on everything but the choice of
// a NaN payload -- fmaxf ignores a NaN operand (IEEE maxNum; +0 counts as larger than -0), so a NaN comes out only when
// every lane holds one.  Pinned by tests/test_gpu_wave_reduce.py through nfft_dbg_wave_reduce (selftest.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace nfft {

namespace wave_reduce_detail {
// DPP controls (the instruction's dpp_ctrl field)
constexpr int kRowShr1 = 0x111, kRowShr2 = 0x112, kRowShr4 = 0x114, kRowShr8 = 0x118, kRowBcast15 = 0x142, kRowBcast31 = 0x143;

// v = op(v, the value of the lane CTRL names); lanes CTRL leaves out (no source inside the row, row not in ROW_MASK)
// combine with their own value, which changes nothing
template <int CTRL, int ROW_MASK, typename T, typename Op>
__device__ __forceinline__ T dpp_step(T v, Op op)
{
    static_assert(sizeof(T) == 4, "one dword per lane");
    const int bits = __builtin_bit_cast(int, v);
    return op(v, __builtin_bit_cast(T, __builtin_amdgcn_update_dpp(bits, bits, CTRL, ROW_MASK, 0xf, false)));
}

template <typename T, typename Op>
__device__ __forceinline__ T reduce_to_lane63(T v, Op op)
{
    v = dpp_step<kRowShr1, 0xf>(v, op);
    v = dpp_step<kRowShr2, 0xf>(v, op);
    v = dpp_step<kRowShr4, 0xf>(v, op);
    v = dpp_step<kRowShr8, 0xf>(v, op);     // lane 15 of every row: the row
    v = dpp_step<kRowBcast15, 0xa>(v, op);  // lanes 31 and 63: two rows
    v = dpp_step<kRowBcast31, 0xc>(v, op);  // lane 63: the wave
    return __builtin_bit_cast(T, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
} // namespace wave_reduce_detail

// fmaxf over the wave's 64 lanes (every lane must be active); the same value in every lane
__device__ __forceinline__ float wave_max_f32(float v)
{
    return wave_reduce_detail::reduce_to_lane63(v, [](float a, float b) { return fmaxf(a, b); });
}

// min over the wave's 64 lanes (every lane must be active); the same value in every lane
__device__ __forceinline__ int wave_min_i32(int v)
{
    return wave_reduce_detail::reduce_to_lane63(v, [](int a, int b) { return a < b ? a : b; });
}

} // namespace nfft
