// Spectral side of the second-order backward of the point gradient.
//
// The coefficient gradient of G(pos, xhat, w)[i, a] = sum_cr w[i, cr] d Fr[i, cr] / d pos[i, a] for an upstream v is
//     dxhat[k, c] = sum_a 2 pi i k_a adjoint(pos, omega v_a)[k, c],     omega = w_re + i w_im (or w with real_output),
// d adjoints of the point-side products u_a = omega v_a, each multiplied by its axis' wave number and summed in axis order.
// stage: u_a from the real view of w (the scaling of interleaved re / im pairs by a real v is the same as of real columns);
// combine: one elementwise pass per axis over the adjoint's complex output.
#include "common.h"
#include "kernels.h"

namespace nfft {

namespace {

__global__ void __launch_bounds__(256)
hvp_stage_kernel(const float *__restrict__ w, const float *__restrict__ v, const int64_t n, const int64_t Cr, const int dim,
                 const int a, float *__restrict__ u)
{
    const int64_t len = n * Cr;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < len; e += (int64_t)gridDim.x * 256) {
        const int64_t i = e / Cr;
        u[e] = w[e] * v[i * dim + a];
    }
}

// y, dxhat: [B, N^dim, C]; k_a = (index along spectral axis a) - N / 2
__global__ void __launch_bounds__(256)
hvp_combine_kernel(const float2 *__restrict__ y, const int64_t total, const int64_t N, const int dim, const int64_t C,
                   const int a, const int accumulate, const int out_complex, void *__restrict__ dxhat)
{
    int64_t stride = C;  // elements between neighbours along spectral axis a
    for (int b = a + 1; b < dim; ++b) stride *= N;
    const float twopi = 6.283185307179586f;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const float ka = twopi * (float)((e / stride) % N - N / 2);
        const float2 z = y[e];
        // 2 pi i k_a (z.x + i z.y) = 2 pi k_a (-z.y + i z.x)
        const float re = -ka * z.y, im = ka * z.x;
        if (out_complex) {
            float2 *const o = (float2 *)dxhat + e;
            if (accumulate) *o = float2{o->x + re, o->y + im};
            else *o = float2{re, im};
        } else {
            float *const o = (float *)dxhat + e;
            *o = accumulate ? *o + re : re;
        }
    }
}

unsigned grid_blocks(int64_t len) { return (unsigned)std::min<int64_t>((len + 255) / 256, 4096); }

} // namespace

int launch_hvp_stage(const float *w, const float *v, int64_t n, int64_t Cr, int dim, int a, float *u, hipStream_t stream)
{
    if (n * Cr <= 0) return 0;
    hipLaunchKernelGGL(hvp_stage_kernel, dim3(grid_blocks(n * Cr)), dim3(256), 0, stream, w, v, n, Cr, dim, a, u);
    NFFT_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_hvp_combine(const void *y, int64_t B, int64_t N, int dim, int64_t C, int a, int accumulate, int out_complex,
                       void *dxhat, hipStream_t stream)
{
    int64_t total = B * C;
    for (int b = 0; b < dim; ++b) total *= N;
    if (total <= 0) return 0;
    hipLaunchKernelGGL(hvp_combine_kernel, dim3(grid_blocks(total)), dim3(256), 0, stream, (const float2 *)y, total, N, dim,
                       C, a, accumulate, out_complex, dxhat);
    NFFT_HIP_CHECK(hipGetLastError());
    return 0;
}

} // namespace nfft
