// Host-side conventions of the C-ABI layer (api.hip, api_pair.hip): how a workspace is carved and its base checked.
#pragma once
#include "common.h"

namespace nfft {

// where a workspace's next block begins: blocks inside an aligned workspace sit on 256-byte boundaries
inline int64_t round256(int64_t bytes) { return (bytes + 255) & ~int64_t(255); }

// Offsets of a workspace's blocks, each on a 256-byte boundary.  The entry points align the caller's pointer up to 256
// themselves (workspace_base), which may skip up to 255 bytes: total() is the aligned end + 256 bytes of slack for that.
// Carve(end) continues an earlier carve from its end().
struct Carve {
    int64_t o;
    explicit Carve(int64_t end = 0) : o(end) {}
    int64_t take(int64_t bytes) { const int64_t at = o; o = align_up(o + bytes, 256); return at; }
    int64_t end() const { return o; }
    int64_t total() const { return o + 256; }
};

// the 256-aligned base of a workspace of `have` bytes that must hold `need`; nullptr (NFFT_HIP_EWORKSPACE) if it does not
inline char *workspace_base(void *workspace, int64_t have, int64_t need)
{
    if (!workspace || have < need) { set_error("workspace too small"); return nullptr; }
    return (char *)(((uintptr_t)workspace + 255) & ~uintptr_t(255));
}

// every entry a number of magnitude <= limit
inline bool all_finite(const double *v, int n, double limit)
{
    for (int e = 0; e < n; ++e)
        if (!(v[e] == v[e]) || v[e] > limit || v[e] < -limit) return false;
    return true;
}

// cells of the half spectrum of one real grid plane: M / 2 + 1 along the last axis
inline int64_t half_cells_of(const Geom &g) { return (int64_t)(g.M / 2 + 1) * g.Ma[0] * g.Ma[1]; }

} // namespace nfft
