// What the matrix-core kernels of the wide tiling share: spread_mfma_kernel (spread_mfma.hip), interp_mfma_kernel
// (interp_mfma.hip), interp_cols_kernel (interp_cols.hip) and interp_stream_kernel (interp_stream.hip) sweep work items
// -- ranges of slabs of a pencil -- that they all take from ONE place, the plan's work list in launch order (common.h,
// plan layout; binning.hip segment_split_kernel / work_order_kernel), from one pair of launches (launch_range_kernels),
// through one work-item frame on the device (plan_launch, work_items).
//
// The two launches.  A balanced plan runs one workgroup per list entry: workgroup blockIdx.x takes entry blockIdx.x of
// its point set's part of the list, straight-line code without an item loop.  The dispatcher starts workgroups in grid
// order as CUs fall free, so the list's order is the launch order: the grid order of the equal cut, or biggest first
// (longest-first scheduling for free).  Any other plan walks the same list with ONE persistent launch per plane.  Both
// launches are always enqueued, the per-entry one first, on the same stream with the same gridDim.y; the one that is
// not the plan's returns at once (work[0].z says which).  Each kernel is instantiated for both (template flag OVERFLOW:
// the persistent form), because the item loop costs registers.
#pragma once
#include <cassert>

#include "common.h"

namespace nfft {

// What the host knows of a call's work items without reading the plan: the items of an average pencil (seg_base_runs),
// from which the plan's list is cut (binning.hip launch_segment_split) and the launches are sized.  The ranges
// themselves exist in the plan's list only.
struct RangeSplit {
    int64_t pencils;  // pencils per point set
    int64_t nsets;    // point sets (>= 1)
    int runs;         // items of an average pencil
};
inline RangeSplit range_split(const Geom &g, int64_t n, int64_t B)
{
    const int64_t pencils = (int64_t)g.nta[1] * g.nta[2], nsets = B > 0 ? B : 1;
    return RangeSplit{pencils, nsets, seg_base_runs(n, nsets, pencils, g.M, device_cu_count())};
}
// ... at launch time, for the plan L of n points: its point-set count is ntiles / tiles_per_batch, because a plan of the
// wide tiling has no sub-blocks (common.h make_geom: they exist for the register-tile spreading mode only, the wide
// tiling for the matrix-core one).
inline RangeSplit range_split(const Geom &g, const PlanLayout &L, int64_t n)
{
    assert(g.SB == 1);
    return range_split(g, n, g.tiles_per_batch > 0 ? L.ntiles / g.tiles_per_batch : 1);
}

// What the launcher hands to a range kernel's launch: the plan arrays and the work list
struct RangeArgs {
    const int *tile_offsets;
    const float *spos;
    const int4 *work, *sorted;  // the plan's work list (header) and its entries in launch order
    int *tickets;               // counters of the persistent launch (next_work_item), or nullptr: round robin
};

// Host side of the range kernels: launch(kernel, blocks, args) enqueues `kernel` (BALANCED: one workgroup per list entry;
// LISTED: the persistent form) with the grid `blocks`.  ny = gridDim.y: planes, pair slots or column groups.  The
// kernels take up to `lds` bytes of dynamic LDS (one workgroup per CU: raised once per device).  `tickets`: kTicketPlanes
// ints of the caller's workspace; the persistent launch hands its entries out by tickets when its planes fit them, else
// round robin; the launch before it zeroes the counters.
template <auto BALANCED, auto LISTED, class F>
int launch_range_kernels(const Geom &g, const PlanLayout &L, const void *plan, int64_t n, int64_t ny, size_t lds,
                         int *tickets, F &&launch)
{
    const RangeSplit s = range_split(g, L, n);
    static DeviceOnce attr_done;
    if (attr_done.first_use()) {
        NFFT_HIP_CHECK(hipFuncSetAttribute((const void *)BALANCED, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        NFFT_HIP_CHECK(hipFuncSetAttribute((const void *)LISTED, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr_done.mark();
    }
    const char *base = (const char *)plan;
    const int4 *work = (const int4 *)(base + L.off_work);
    const RangeArgs a{(const int *)(base + L.off_offsets), (const float *)(base + L.off_spos), work,
                      work + L.work_head + L.work_cap, ny > kTicketPlanes ? nullptr : tickets};
    const int64_t per_entry = std::min<int64_t>(per_entry_workgroups(n, s.nsets, s.pencils, s.runs, g.M, device_cu_count()), L.work_cap);
    launch(BALANCED, dim3((unsigned)per_entry, (unsigned)ny), a);
    launch(LISTED, dim3(work_list_workgroups(n, s.nsets, s.pencils, s.runs, device_cu_count()), (unsigned)ny), a);
    NFFT_HIP_CHECK(hipGetLastError());
    return 0;
}

#if defined(__HIPCC__)

// Dynamic hand-out of the sorted work list to the workgroups of a persistent launch: a workgroup starts with entry
// blockIdx.x and then takes the next free entry whenever it is done (the list is sorted biggest first: longest-processing-
// time-first scheduling).  A ticket is one atomic add on the counter of the workgroup's plane, tickets[blockIdx.y]: the
// launch's kTicketPlanes ints in the workspace of the call, so the plan stays read-only (it may be in use on several
// streams).  nullptr: the static round robin of listed_item.  The one-workgroup-per-range launch, always enqueued just
// before the persistent one on the same stream with the same gridDim.y, zeroes the counters as its first statement
// (before any early return).  The zero is an atomic exchange: every access to a counter is a device-scope atomic,
// performed where the adds are, and none depends on the end-of-kernel write-back of one XCD's L2.
__device__ __forceinline__ void reset_tickets(int *tickets)
{
    if (tickets && blockIdx.x == 0 && threadIdx.x == 0) (void)atomicExch(&tickets[blockIdx.y], 0);
}

// Next entry of the work list for this workgroup of a persistent launch (n_items or more: none left): its own index
// first, then tickets -- or the static round robin.  Called by all threads of the workgroup together; `word` is an LDS
// int of the workgroup.
__device__ __forceinline__ int next_work_item(int *tickets, int *word, const int prev /* < 0: first call */)
{
    if (prev < 0) return (int)blockIdx.x;
    if (!tickets) return prev + (int)gridDim.x;
    __syncthreads();  // every wave is done with the previous item (and has read the previous ticket)
    if (threadIdx.x == 0) *word = (int)gridDim.x + atomicAdd(&tickets[blockIdx.y], 1);
    __syncthreads();
    return *word;
}

// Entry `item` (= round * gridDim.x + blockIdx.x) of a persistent launch over the plan's sorted work list: a static
// round robin, every other round in reverse -- the workgroup that took the biggest item of one round takes the
// smallest of the next.  (A partial last round stays in order.)
__device__ __forceinline__ int4 listed_item(const int4 *__restrict__ sorted, const int item, const int n_items)
{
    const int G = (int)gridDim.x, round = item / G;
    const bool reverse = (round & 1) && (round + 1) * G <= n_items;
    return sorted[reverse ? (round + 1) * G - 1 - (int)blockIdx.x : item];
}

// Whether this launch is the plan's (work[0].z: the plan walks its list); the other one returns at once.
template <bool OVERFLOW>
__device__ __forceinline__ bool plan_launch(const int4 *work)
{
    const int listed = work[0].z;
    return OVERFLOW ? listed : !listed;
}

// The items of the launch for point set b: its part of the sorted list, n entries from `entries` (set header b =
// {entries, first entry}).  The persistent form walks them (next_work_item); workgroup blockIdx.x of the per-entry form
// has one, entry blockIdx.x, and none if the set has fewer entries (it returns before it touches its LDS).  (The decode of
// an entry {point set * pencils + pencil, sb, se, points} is written out in the kernels: as a helper it changed their code.)
struct WorkItems {
    int n;
    const int4 *entries;
};
__device__ __forceinline__ WorkItems work_items(const int4 *work, const int4 *sorted, const int b)
{
    // (the same for every lane: say so -- a load the compiler cannot prove unclobbered lands in vector registers)
    const int2 set_hdr = ((const int2 *)(work + 1))[b];
    return WorkItems{__builtin_amdgcn_readfirstlane(set_hdr.x), sorted + __builtin_amdgcn_readfirstlane(set_hdr.y)};
}

#endif // __HIPCC__

} // namespace nfft
