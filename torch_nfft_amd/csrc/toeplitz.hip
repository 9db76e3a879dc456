// Toeplitz normal operator A^H W A: the two kernels of its own.
//
//   (A^H W A)[k, k'] = sum_i w_i e^{2 pi i (k - k').p_i} = t[k - k']  is a d-level Toeplitz matrix; embedded in a
//   circulant of size M = 2N per axis -- the oversampled grid of the transforms -- one application is
//       forward FFT stage (band -> grid, no roll-off)  ->  grid *= K  ->  adjoint FFT stage (grid -> band, no roll-off)
//   with the real grid K[j] = M^-d sum_n t[n] e^{-2 pi i n.j / M}.
//
// toeplitz_spectrum_kernel   set-up: t (the bandwidth-2N adjoint of the weights, centred: lag n at index n + N) -> the
//                            Hermitian half spectrum of K in the order the C2R transform of fft.cpp reads
// toeplitz_multiply_kernel   hot path: grid plane p *= K[set of p]; bound by HBM (read grid, read K, write grid)
// No reference counterpart: the reference has no normal operator.
#include "common.h"
#include "kernels.h"

namespace nfft {

namespace {

struct LagGeom {
    int dim, M, Mh;  // Mh = M/2 + 1
    int Ma[3];       // extent per internal axis (1 when degenerate)
    int64_t half_cells, cells;
    float scale;     // M^-dim
};

__device__ __forceinline__ float2 load_lag(const LagGeom &s, const float2 *__restrict__ t, int n0, int n1, int n2)
{
    // index n + N on every live axis (N = M/2)
    const int h = s.M / 2;
    const int i2 = n2 + h;
    const int i1 = s.Ma[1] > 1 ? n1 + h : 0;
    const int i0 = s.Ma[0] > 1 ? n0 + h : 0;
    return t[((int64_t)i0 * s.Ma[1] + i1) * s.Ma[2] + i2];
}

// One thread per element of the half spectrum of every point set.  The C2R transform evaluates
// sum_kappa S[kappa] e^{+2 pi i kappa.j / M}, so S[kappa] = M^-d t[-kappa]; t is Hermitian up to the rounding of the
// adjoint that made it, and S takes its Hermitian part (t[-kappa] + conj(t[kappa])) / 2 -- the part a real K keeps.
// Lags with a component -N (kappa = M/2 on an axis) never occur in k - k' and are set to zero.
__global__ void __launch_bounds__(256) toeplitz_spectrum_kernel(LagGeom s, const float2 *__restrict__ t, int64_t B,
                                                               float2 *__restrict__ spec)
{
    const int64_t total = B * s.half_cells;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = e / s.half_cells;
        int64_t r = e - b * s.half_cells;
        const int k2 = (int)(r % s.Mh); r /= s.Mh;
        const int k1 = (int)(r % s.Ma[1]); r /= s.Ma[1];
        const int k0 = (int)r;
        const int half = s.M / 2;
        float2 out = make_float2(0.f, 0.f);
        const bool edge = k2 == half || (s.Ma[1] > 1 && k1 == half) || (s.Ma[0] > 1 && k0 == half);
        if (!edge) {
            const int n2 = k2;  // 0 .. N-1
            const int n1 = k1 < half ? k1 : k1 - s.M;
            const int n0 = k0 < half ? k0 : k0 - s.M;
            const float2 *tb = t + b * s.cells;
            const float2 tp = load_lag(s, tb, n0, n1, n2);
            const float2 tm = load_lag(s, tb, -n0, -n1, -n2);
            out.x = 0.5f * s.scale * (tm.x + tp.x);
            out.y = 0.5f * s.scale * (tm.y - tp.y);
        }
        spec[e] = out;
    }
}

// grid[p, :] *= K[set of p, :] for the planes [plane0, plane0 + nplanes) of a chunk; plane = set * Cr + real plane.
// A work item is four consecutive cells of one point set: one 16-byte load of K serves every plane of the set that the
// chunk holds (the 2 C real planes of a set; at C > 1 re-reading K per plane would be most of the traffic), each plane
// is one 16-byte load and one 16-byte store.  Grid-stride over a launch sized to the CUs; no atomics, every cell is
// written by exactly one thread: bitwise reproducible.
__global__ void __launch_bounds__(256) toeplitz_multiply_kernel(float4 *__restrict__ grid, const float4 *__restrict__ K,
                                                               int64_t cells4, int64_t Cr, int64_t plane0,
                                                               int64_t nplanes, int64_t set0, int64_t nsets)
{
    const int64_t total = nsets * cells4;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t sl = e / cells4;
        const int64_t v = e - sl * cells4;
        const int64_t set = set0 + sl;
        const float4 k = K[set * cells4 + v];
        // planes of this set inside the chunk, as local plane indices
        const int64_t lo = max(set * Cr, plane0) - plane0;
        const int64_t hi = min((set + 1) * Cr, plane0 + nplanes) - plane0;
        float4 *g = grid + lo * cells4 + v;
        int64_t p = lo;
        for (; p + 2 <= hi; p += 2, g += 2 * cells4) {  // (two planes in flight: the (re, im) pair of a column)
            float4 a = g[0], b = g[cells4];
            a.x *= k.x; a.y *= k.y; a.z *= k.z; a.w *= k.w;
            b.x *= k.x; b.y *= k.y; b.z *= k.z; b.w *= k.w;
            g[0] = a;
            g[cells4] = b;
        }
        if (p < hi) {
            float4 a = g[0];
            a.x *= k.x; a.y *= k.y; a.z *= k.z; a.w *= k.w;
            g[0] = a;
        }
    }
}

}  // namespace

int launch_toeplitz_spectrum(const Geom &g, const float2 *t, int64_t B, float2 *spec, hipStream_t stream)
{
    LagGeom s;
    s.dim = g.dim;
    s.M = g.M;
    s.Mh = g.M / 2 + 1;
    s.half_cells = s.Mh;
    s.scale = 1.0f;
    for (int a = 0; a < 3; ++a) {
        s.Ma[a] = g.Ma[a];
        if (a < 2) s.half_cells *= g.Ma[a];
        if (g.Ma[a] > 1) s.scale /= (float)g.M;
    }
    s.cells = g.cells;
    const int64_t total = B * s.half_cells;
    if (total <= 0) return 0;
    int64_t blocks = (total + 255) / 256;
    if (blocks > 256 * 64) blocks = 256 * 64;
    hipLaunchKernelGGL(toeplitz_spectrum_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, s, t, B, spec);
    NFFT_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_toeplitz_multiply(const Geom &g, float *grid, const float *K, int64_t Cr, int64_t plane0, int64_t nplanes,
                             hipStream_t stream)
{
    if (nplanes <= 0 || Cr <= 0) return 0;
    // (M = 2N with N even: a plane is a whole number of 16-byte vectors)
    const int64_t cells4 = g.cells / 4;
    const int64_t set0 = plane0 / Cr;
    const int64_t nsets = (plane0 + nplanes - 1) / Cr - set0 + 1;
    const int64_t total = nsets * cells4;
    // eight workgroups of 256 per CU keep enough 16-byte loads in flight to cover the HBM latency
    int64_t blocks = (total + 255) / 256;
    const int64_t most = (int64_t)device_cu_count() * 8;
    if (blocks > most) blocks = most;
    hipLaunchKernelGGL(toeplitz_multiply_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, (float4 *)grid,
                       (const float4 *)K, cells4, Cr, plane0, nplanes, set0, nsets);
    NFFT_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace nfft
