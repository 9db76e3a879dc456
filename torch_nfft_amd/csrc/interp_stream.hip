// Interpolation (forward gather) on the matrix cores, streamed: producer waves feed a ring of grid planes,
// consumer waves take blocks of points from a queue -- no workgroup barrier inside a work item.
//
// Same arithmetic as interp_mfma.hip (reference: csrc/cuda/spatial_window_operations.cu:214-332): per plane z of a
// pencil and block of 32 points  T_z = G_z Psi2  (MFMAs on f16-split operands), t = sum_u1 psi1[u1] T_z[u1, i],
// y_i += psi0_i[z] t.  What changes is the schedule.  interp_mfma.hip advances in lock step: stage the planes of a
// chunk (all waves wait for the loads), barrier, every wave takes one block, barrier ... -- measured at config C3:
// staging alone 0.44 ms, compute alone 1.30 ms, nothing overlaps (profiles/r02_experiments.md).  Here
//   * 4 producer waves stage planes continuously: wave p takes the ring slots s = p (mod 4) of the item's sweep,
//     loads the padded 32 x 64 tile, scales it by its own power of two, f16-splits it into the ring slot z & 15 and
//     publishes ready[slot] = z.  A producer's per-plane chain holds ONE LDS round trip besides the eight fragment
//     writes, and that one only when it has to wait: which planes it stages is a bit mask built at the item's set-up,
//     the tile's maximum is reduced in registers (wave_reduce.h), the slowest consumer's progress is cached and read
//     again (one read: the twelve progress words and the abort flag, reduced in registers) only when the cached value
//     does not allow the slot, every address of a plane is formed at set-up, and two register tiles take turns so
//     that the next plane's loads are in flight for the whole conversion of the current one (profiles/
//     r11_gather_staging.md);
//   * 12 consumer waves pull blocks from an LDS counter.  A block is 32 points of ONE chunk (17 - (2m+2) slabs, so its
//     window is at most the 16 planes of the ring) and, when the plan is ordered by column group (common.h), of ONE
//     group: its windows then lie inside two of the tile's four 16-column k-steps, which halves the MFMAs, the B
//     fragments and the A-fragment reads (measured: 1.43 -> 1.05 ms at C3 for half the k-steps).  The points of a
//     (chunk, group) are the group's runs of the chunk's slabs, concatenated; blocks are handed out in the order of the
//     run their first point lies in, i.e. by first slab, whatever the group -- so a wave's first plane never moves
//     backwards.  A wave publishes that plane (progress[wave]), waits until all planes of the block are staged (one
//     poll reads all 16 flags), builds its B fragments / psi1 weights and walks the planes without further checks; the
//     A fragments of the next plane are requested as soon as the MFMAs that read a buffer are issued;
//   * a wave claims its next block and fetches that block's points while it works on the current one;
//   * a producer may overwrite slot z & 15 once every consumer's progress is beyond z - 16.  The slowest consumer
//     needs planes below progress + 16 only, so the producers can always serve it: no cycle of waits.  The producers
//     judge this by a cached minimum of progress[]; progress only grows within an item, so a stale minimum only ever
//     under-estimates it: it can send a producer to read the words again, never past a consumer.
// Every spin loop is bounded (kSpinLimit): a logic error never hangs the GPU; the wave that runs out raises the
// device's fault flag (common.h report_fault), everybody leaves the item, and the next entry point of the C ABI
// returns NFFT_HIP_EKERNEL instead of handing out the unfinished rows as a result.
#include <algorithm>
#include <climits>
#include <type_traits>

#include "common.h"
#include "kernels.h"
#include "mfma_split.h"
#include "range_items.h"
#include "wave_reduce.h"

namespace nfft {

#ifdef NFFT_HIP_TRACE
// Developer instrumentation (variant builds only, scripts/exp_build.sh -DNFFT_HIP_TRACE), in the layout of the spreading
// kernel's (spread_mfma.hip, scripts/spread_trace.py): eight 64-bit words per workgroup of the per-entry launch -- 100 MHz
// real-time stamps at entry [0, 1], after the item's set-up [2], when the last wave is done [3, 6], the hardware id of the
// CU [4], the item's block and point counts [5].
__device__ unsigned long long *g_stream_trace = nullptr;
#define NFFT_GTRACE_AT(slot) (&g_stream_trace[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 8 + (slot)])
#define NFFT_GTRACE(slot, value)                                                                                  \
    do {                                                                                                          \
        if (!OVERFLOW && threadIdx.x == 0 && g_stream_trace) *NFFT_GTRACE_AT(slot) = (value);                     \
    } while (0)
#define NFFT_GTRACE_END()                                                                                         \
    do {                                                                                                          \
        if (!OVERFLOW && lane == 0 && g_stream_trace) {                                                           \
            const unsigned long long now_ = __builtin_amdgcn_s_memrealtime();                                     \
            atomicMax(NFFT_GTRACE_AT(3), now_);                                                                   \
            atomicMax(NFFT_GTRACE_AT(6), now_);                                                                   \
        }                                                                                                         \
    } while (0)
// Second buffer, sixteen words per workgroup (nfft_dbg_set_stream_phase): where the first producer wave and the first
// consumer wave of an item spend their time, as sums of shader-clock ticks (s_memtime).  Producer, per staged plane: [0]
// waiting for the plane's loads, [1] the tile's maximum, [2] waiting for the ring (progress), [3] conversion, fragment
// writes and publishing, [4] bookkeeping: the next plane and issuing its loads; [5] planes staged, [6] 1 in an edge column
// pencil.  Consumer: [8] waiting for ready, [9] everything else, [10] blocks.  (The stamps wait for the scalar cache, which
// also drains the wave's LDS queue: the split is a guide to the order of magnitude of each part, not a cycle count.)
__device__ unsigned long long *g_stream_phase = nullptr;
#define NFFT_PHASE_AT(slot) (&g_stream_phase[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 16 + (slot)])
#define NFFT_PHASE(k)                                                                                             \
    do {                                                                                                          \
        if (phase_on) {                                                                                           \
            const unsigned long long now_ = __builtin_amdgcn_s_memtime();                                         \
            ph[k] += now_ - ph_t;                                                                                 \
            ph_t = now_;                                                                                          \
        }                                                                                                         \
    } while (0)
#define NFFT_PHASE_WAIT_LOADS(n) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(n) : "memory")
#else
#define NFFT_GTRACE(slot, value) do { } while (0)
#define NFFT_GTRACE_END() do { } while (0)
#define NFFT_PHASE(k) do { } while (0)
#define NFFT_PHASE_WAIT_LOADS(n) do { } while (0)
#endif

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int kIsThreads = 1024;
constexpr int kIsWaves = kIsThreads / 64;
#ifndef NFFT_STREAM_PRODUCERS
#define NFFT_STREAM_PRODUCERS 4
#endif
constexpr int kIsProducers = NFFT_STREAM_PRODUCERS;  // measured at C3: 3 producers 1.50 ms, 4: 1.41, 5: 1.50 (each owns 16 / 4 ring slots)
static_assert(16 % kIsProducers == 0, "a ring slot has one owner: the producer count divides the ring");
constexpr int kIsConsumers = kIsWaves - kIsProducers;
constexpr int kIsRing = 16;          // resident planes: TC + 2m+1 = 16 for every cutoff of the wide tiling
constexpr int kIsMaxSlabs = 160;     // slabs the chunks of one work item cover (<= kItemMaxSlabs + 2 TC)
constexpr int kIsMaxRuns = 3 * kIsMaxSlabs;
#ifndef NFFT_HIP_SPIN_LIMIT
#define NFFT_HIP_SPIN_LIMIT (1 << 22)
#endif
constexpr int kSpinLimit = NFFT_HIP_SPIN_LIMIT;  // (the fault-report test builds a variant library with a limit of 0)

struct __align__(16) StreamLds {
    f16x8 frag[kIsRing][4][2][64];   // [plane slot][k-step][hi/lo][lane = 32 (column half) + row]   128 KB
    float pinv[kIsRing];             // what one unit of the scaled plane is worth, times the B operand scale
    int ready[kIsRing];              // plane number held by the slot (published after the fragments)
    int progress[kIsConsumers];      // first plane a consumer still needs
    int next_block;                  // block queue (counts in units of 64: every lane adds 1)
    int abort;                       // set when a spin loop ran out: everybody leaves
    int ticket;                      // work-list entry of the workgroup (persistent launch: next_work_item)
    // runs of the item: run e = (slab - first slab) * NG + group
    int run_start[kIsMaxRuns + 4];   // first point of run e; [runs] = end of the last one
    int run_cum[kIsMaxRuns + 4];     // points of the same chunk and group in front of run e
    int run_blk[kIsMaxRuns + 4];     // blocks whose first point lies in a run before e (prefix sums); [runs] = all blocks
};

// Ordering of the LDS hand-overs between producer and consumer waves.  The LDS unit serves the requests of ONE wave in
// the order they were issued: "data, then flag" on the producer side and "flag, then data" on the consumer side need no
// wait, only the compiler must keep the program order.  The workgroup-scope fences that stood here until round 4 compile
// to s_waitcnt vmcnt(0) as well: a consumer then waited at every block for the acknowledgement of its scattered result
// stores and for the point records of the NEXT block it had just requested (profiles/r04_experiments.md).
#ifndef NFFT_STREAM_LDS_ORDER
#define NFFT_STREAM_LDS_ORDER 1
#endif
__device__ __forceinline__ void lds_release()
{
    if (NFFT_STREAM_LDS_ORDER) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    else __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
}
__device__ __forceinline__ void lds_acquire()
{
    if (NFFT_STREAM_LDS_ORDER) asm volatile("" ::: "memory");
    else __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
__device__ __forceinline__ int lds_load(const int *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void lds_store(int *p, int v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// bit c of the 192-bit mask {w0, w1, w2} (arguments by value: a choice between captured words becomes one between their
// addresses, and the words then live in scratch memory)
__device__ __forceinline__ bool bit192(unsigned long long w0, unsigned long long w1, unsigned long long w2, int c)
{
    const unsigned long long w = c < 64 ? w0 : c < 128 ? w1 : w2;
    return (w >> (c & 63)) & 1;
}

// NG: column groups of the plan (3, or 1 for plans without the group order: every block then spans all four k-steps)
template <int W, bool OVERFLOW, int NG>
__global__ void __launch_bounds__(kIsThreads) __attribute__((amdgpu_waves_per_eu(4, 4)))
interp_stream_kernel(const Geom g, const int *__restrict__ tile_offsets, const int *__restrict__ group_starts,
                     const float *__restrict__ spos, const float *__restrict__ grid,
                     const int Cr, const int plane0, float *__restrict__ yr,
                     const int4 *__restrict__ work, const int4 *__restrict__ sorted, int *tickets, int *__restrict__ status)
{
    constexpr int m = W / 2 - 1;
    if constexpr (!OVERFLOW) reset_tickets(tickets);
    constexpr int TC = 17 - W;                                   // slabs per chunk
    constexpr int SPAN = TC + W - 1;                             // planes a chunk's blocks may touch
    constexpr int NKS = NG == 3 ? 2 : 4;  // k-steps of a block
    static_assert(TC >= 1 && SPAN <= kIsRing, "the ring holds a chunk's planes");
    static_assert(kItemMaxSlabs + 2 * TC <= kIsMaxSlabs, "run tables");
    extern __shared__ __align__(16) unsigned char smem_raw[];
    StreamLds &L = *reinterpret_cast<StreamLds *>(smem_raw);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r32 = lane & 31, h = lane >> 5;
    NFFT_GTRACE(0, __builtin_amdgcn_s_memrealtime());
    NFFT_GTRACE(1, __builtin_amdgcn_s_memrealtime());
    NFFT_GTRACE(4, (unsigned long long)__builtin_amdgcn_s_getreg(63492) | ((unsigned long long)__builtin_amdgcn_s_getreg(63508) << 32));

    const int plane_local = blockIdx.y;
    const int plane = plane0 + plane_local;
    const int b = plane / Cr;
    const int cr = plane - b * Cr;
    const int pencils = g.nta[1] * g.nta[2];
    const int M = g.M;

    // work items (range_items.h)
    if (!plan_launch<OVERFLOW>(work)) return;
    const WorkItems items = work_items(work, sorted, b);
    const int n_items = items.n;
    const int4 *const entries = items.entries;
    for (int item = OVERFLOW ? next_work_item(tickets, &L.ticket, -1) : (int)blockIdx.x; item < n_items;
         item = OVERFLOW ? next_work_item(tickets, &L.ticket, item) : n_items) {
    const int4 it = OVERFLOW && !tickets ? listed_item(entries, item, n_items) : entries[item];
    // (the entry is the same for every lane: say so -- a load the compiler cannot prove unclobbered lands in vector registers)
    const int pencil = __builtin_amdgcn_readfirstlane(it.x) - b * pencils, sb = __builtin_amdgcn_readfirstlane(it.y),
              se = __builtin_amdgcn_readfirstlane(it.z);
    // an item owns the chunks whose first slab lies in its range (as in interp_mfma.hip)
    const int k_begin = (sb + TC - 1) / TC;
    const int k_end = min((M + TC - 1) / TC, (se + TC - 1) / TC);
    if (k_begin >= k_end) continue;
    const int bin0 = b * g.tiles_per_batch + pencil * g.np0;
    const int s0 = k_begin * TC;                    // first slab of the item's chunks
    const int nsl = min(k_end * TC, M) - s0;        // slabs they cover (<= kIsMaxSlabs: a range holds <= 128 slabs)
    const int nruns = nsl * NG;
    if (tile_offsets[bin0 + s0] == tile_offsets[bin0 + s0 + nsl]) continue;  // no points in these chunks
    const int j2 = pencil % g.nta[2], j1 = pencil / g.nta[2];
    const int tb1 = j1 * g.Ta[1], tb2 = j2 * g.Ta[2];
    const float sc = win_exp_scale(m);
    float norm = win_norm(m);
    norm = norm * norm * norm;
    const float *const gplane = grid + (int64_t)plane_local * g.cells;

    // ---- item set-up: run tables, flags -----------------------------------------------------------------------
    __syncthreads();  // the previous item is done with the LDS
    for (int e = tid; e <= nruns; e += kIsThreads) {
        const int s = e / NG, q = e - s * NG;
        const int bin = bin0 + s0 + s;
        L.run_start[e] = q == 0 ? tile_offsets[bin] : group_starts[2 * (int64_t)bin + q - 1];
    }
    if (wave == 0) {
        if (lane < kIsRing) L.ready[lane] = INT_MIN;
        if (lane < kIsConsumers) L.progress[lane] = s0 - m;
        if (lane == 0) { L.next_block = 0; L.abort = 0; }
    }
    __syncthreads();
    for (int e = tid; e < nruns; e += kIsThreads) {
        // blocks of a (chunk, group) are cut from the concatenation of the group's runs over the chunk's slabs
        const int s = e / NG;
        const int t = s % TC;
        int cum = 0;
        for (int k = 1; k <= t; ++k) cum += L.run_start[e - k * NG + 1] - L.run_start[e - k * NG];
        const int len = L.run_start[e + 1] - L.run_start[e];
        L.run_cum[e] = cum;
        L.run_blk[e] = ((cum + len + 31) >> 5) - ((cum + 31) >> 5);  // blocks whose first point lies in this run
    }
    __syncthreads();
    if (wave == 0) {
        int carry = 0;
        for (int base = 0; base <= nruns; base += 64) {
            const int e = base + lane;
            const int nb = e < nruns ? L.run_blk[e] : 0;
            int incl = nb;
            for (int off = 1; off < 64; off <<= 1) {
                const int t = __shfl_up(incl, off);
                if (lane >= off) incl += t;
            }
            if (e <= nruns) L.run_blk[e] = carry + incl - nb;
            carry += __shfl(incl, 63);
        }
    }
    __syncthreads();
    const int total_blocks = L.run_blk[nruns];
    NFFT_GTRACE(2, __builtin_amdgcn_s_memrealtime());
    NFFT_GTRACE(5, (unsigned long long)(unsigned)total_blocks | ((unsigned long long)(unsigned)(L.run_start[nruns] - L.run_start[0]) << 32));

    if (wave >= kIsConsumers) {
        // ================================ producer: planes z = z_begin + p, + 4, ... ================================
        const int p = wave - kIsConsumers;
        const int z_begin = k_begin * TC - m, z_end = (k_end - 1) * TC + SPAN - m;  // planes any chunk of the item needs
        // ---- set-up of the sweep, once per item: everything below stays in registers ------------------------------
        // (1) Which planes are mine to stage.  Chunk c of the item (slabs c TC ... c TC + TC - 1 of its range) uses the
        // planes c TC ... c TC + SPAN - 1 of the sweep (counted from z_begin) iff it holds points; a ring slot belongs
        // to ONE producer (slot mod kIsProducers): planes z and z + 16 share a slot, and only one wave staging them in
        // order keeps a late plane z from overwriting (and un-publishing) plane z + 16.  Both go into one bit mask over
        // the sweep's <= kIsMaxSlabs + 16 planes, which the loop walks with scalar bit scans: no LDS look-up per plane.
        static_assert(kIsMaxSlabs + kIsRing <= 192, "three 64-bit words hold the sweep");
        const int nchunks = k_end - k_begin;
        const auto chunk_live = [&](const int c) {
            if (c >= nchunks) return false;
            const int lo = c * TC, hi = min(lo + TC, nsl);
            return L.run_start[hi * NG] > L.run_start[lo * NG];
        };
        const unsigned long long cm0 = __builtin_amdgcn_ballot_w64(chunk_live(lane)), cm1 = __builtin_amdgcn_ballot_w64(chunk_live(64 + lane)),
                                 cm2 = __builtin_amdgcn_ballot_w64(chunk_live(128 + lane));
        const auto plane_mine = [&](const int r) {
            const int z = z_begin + r;
            if (z >= z_end || ((z & (kIsRing - 1)) % kIsProducers) != p) return false;
            const int c_hi = min(nchunks - 1, r / TC), c_lo = max(0, (r - SPAN + TC) / TC);
            bool any = false;
            for (int c = c_lo; c <= c_hi; ++c) any |= bit192(cm0, cm1, cm2, c);
            return any;
        };
        const unsigned long long pm0 = __builtin_amdgcn_ballot_w64(plane_mine(lane)), pm1 = __builtin_amdgcn_ballot_w64(plane_mine(64 + lane)),
                                 pm2 = __builtin_amdgcn_ballot_w64(plane_mine(128 + lane));
        // first plane >= z (z >= z_begin) of this producer's sequence that some chunk needs; z_end: none
        const auto next_needed = [&](const int z) {
            const int r = z - z_begin;
            unsigned long long w = r < 64 ? pm0 & (~0ull << r) : 0ull;
            if (w) return z_begin + __builtin_ctzll(w);
            w = r < 128 ? (r > 64 ? pm1 & (~0ull << (r - 64)) : pm1) : 0ull;
            if (w) return z_begin + 64 + __builtin_ctzll(w);
            w = r < 192 ? (r > 128 ? pm2 & (~0ull << (r - 128)) : pm2) : 0ull;
            if (w) return z_begin + 128 + __builtin_ctzll(w);
            return z_end;
        };
        // (2) Where a plane's values come from.  A lane's 4 tasks of a plane: (row, group of 8 columns); 16 consecutive
        // lanes = 16 consecutive rows of one column group -> consecutive 16-byte LDS slots on the way out, half rows of
        // 128 contiguous bytes on the way in.  Each task is two 16-byte halves; off[] is the half's offset inside a
        // plane, rows and columns wrapped.  In the first and last column pencil a half may begin beyond column M - 1:
        // it is still ONE vector load, at the wrapped address.  Only a half that straddles columns M - 1 | 0 is not
        // contiguous -- at most one (column group, half) per lane, because a lane's halves are 4 ... 36 columns apart
        // and M >= 64, so it is the same half of both tasks of that column group (rows r and r + 16).  Such a half is
        // loaded as the row's last four columns, the lane loads the first four columns of its two rows on top (xoff[],
        // two more vector loads in an edge pencil), and the half is put together in registers when the plane is
        // converted: `before` = its columns in front of the wrap (1 ... 3).  Every load of a plane is a vector load
        // into registers of its own from an address formed here: nothing between them to wait for.
        int off[8], xoff[2] = {0, 0};
        unsigned straddle = 0;
        int before = 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int t = lane + 64 * i;
            const int cg = ((t >> 4) & 3) + 4 * ((t >> 7) & 1), row = (t & 15) + 16 * ((t >> 6) & 1);
            const int g1 = wrap_near(tb1 - m + row, M);
            if (i < 2) xoff[i] = g1 * M;  // (the row of task i is the row of task i + 2)
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                const int w = wrap_near(tb2 - m + 8 * cg + 4 * hf, M);
                off[2 * i + hf] = g1 * M + min(w, M - 4);
                if (w + 4 > M) {
                    straddle |= 1u << (2 * i + hf);
                    before = M - w;
                }
            }
        }
        struct Tile {
            f32x4 v[8];  // the 8 halves
            f32x4 x[2];  // edge pencils: columns 0 ... 3 of the lane's two rows
        };
        // (3) The slowest consumer, as last seen.  progress[] only grows within an item (s0 - m at set-up, INT_MAX when
        // a consumer is done), so a value read earlier is a lower bound of the present one: if IT already allows a slot
        // the producer goes ahead without reading, and it reads again only when it would have to wait.  A stale value
        // under-estimates progress -- it can make the producer read, never proceed early -- and a producer that reads
        // sees what the per-plane poll saw before: the no-cycle argument of the header is unchanged.  One read serves
        // everything: lanes 0 ... 11 take progress[lane], the others the abort flag as INT_MIN (raised) or INT_MAX, and
        // the minimum is formed in registers (wave_reduce.h): INT_MIN = abort, INT_MAX = every consumer gone.
        int lo_seen = z_begin;
#ifdef NFFT_HIP_TRACE
        const bool phase_on = !OVERFLOW && p == 0 && g_stream_phase;
        unsigned long long ph[6] = {0, 0, 0, 0, 0, 0}, ph_t = __builtin_amdgcn_s_memtime();
#endif
        // The sweep, for interior (EDGE = false) and edge column pencils.  Two tiles take turns: while one is converted
        // the loads of the next needed plane fill the other, and no value is copied between them.  Every path through
        // the loop issues the same number of loads per plane (past the end of the sweep the current plane is requested
        // again and dropped), so the wait in front of a tile's first use is "all but the loads issued after its own":
        // a count the compiler can state.  (With loads under a condition, or a copy `cur = nxt` at the loop's end, every
        // plane was waited for right after its loads were issued.)
        const auto sweep = [&](auto edge_tag) {
            constexpr bool EDGE = decltype(edge_tag)::value;
            const auto load_plane = [&](const int z, Tile &t) {
                const float *const base = gplane + (int64_t)wrap(z, M) * M * M;
#pragma unroll
                for (int k = 0; k < 8; ++k) t.v[k] = *(const f32x4_dw *)(base + off[k]);
                if constexpr (EDGE) {
                    t.x[0] = *(const f32x4_dw *)(base + xoff[0]);
                    t.x[1] = *(const f32x4_dw *)(base + xoff[1]);
                }
            };
            // converts plane z from tile t into its ring slot and publishes it; false: leave the sweep
            const auto stage = [&](const int z, Tile &t) {
                NFFT_PHASE(4);
                NFFT_PHASE_WAIT_LOADS(EDGE ? 10 : 8);  // (this tile's loads: all but the other tile's, issued after them)
                NFFT_PHASE(0);
                if constexpr (EDGE) {
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        if ((straddle >> k) & 1) {  // columns M - before ... M - 1 from v, then 0 ... from x
                            const f32x4 a = t.v[k], c = t.x[(k >> 1) & 1];
                            f32x4 r;
                            r.x = before == 1 ? a.w : before == 2 ? a.z : a.y;
                            r.y = before == 1 ? c.x : before == 2 ? a.w : a.z;
                            r.z = before == 1 ? c.y : before == 2 ? c.x : a.w;
                            r.w = before == 1 ? c.z : before == 2 ? c.y : c.x;
                            t.v[k] = r;
                        }
                    }
                }
                // power-of-two scale of the tile; odd planes are stored negated (un-negated through pinv): the MFMA
                // accumulation truncates with a small sign-independent bias that cancels over alternating planes
                float mx = 0.0f;
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    mx = fmaxf(fmaxf(fmaxf(mx, fabsf(t.v[e].x)), fabsf(t.v[e].y)), fmaxf(fabsf(t.v[e].z), fabsf(t.v[e].w)));
                mx = wave_max_f32(mx);
                NFFT_PHASE(1);
                float scale = 1.0f, inv = 1.0f;
                if (mx > 1.0e-30f && mx < 3.0e38f) {
                    int ex;
                    frexpf(mx, &ex);
                    scale = ldexpf(1.0f, 11 - ex);
                    inv = ldexpf(1.0f, ex - 11);
                }
                const int slot = z & (kIsRing - 1);
                if (slot & 1) { scale = -scale; inv = -inv; }
                // the slot's previous plane, z - 16, must be behind every consumer
                if (lo_seen <= z - kIsRing) {
                    int spins = 0;
                    while (true) {
                        const int word = lds_load(lane < kIsConsumers ? &L.progress[lane] : &L.abort);
                        lo_seen = wave_min_i32(lane < kIsConsumers ? word : word ? INT_MIN : INT_MAX);
                        if (lo_seen > z - kIsRing || lo_seen == INT_MIN) break;
                        if (++spins > kSpinLimit) {
                            lds_store(&L.abort, 1);
                            if (lane == 0) report_fault(status, kFaultStreamStall);
                            lo_seen = INT_MIN;
                            break;
                        }
                        __builtin_amdgcn_s_sleep(4);
                    }
                }
                NFFT_PHASE(2);
                // (abort: everybody leaves; every consumer gone: nobody reads what is left of the sweep)
                if (lo_seen == INT_MIN || lo_seen == INT_MAX) return false;
                lds_acquire();
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int tk = lane + 64 * i;
                    const int cg = ((tk >> 4) & 3) + 4 * ((tk >> 7) & 1), row = (tk & 15) + 16 * ((tk >> 6) & 1);
                    const f32x4 a = t.v[2 * i], c = t.v[2 * i + 1];
                    unsigned h0, h1, h2, h3, q0, q1, q2, q3;
                    split_pair(a.x * scale, a.y * scale, h0, q0);
                    split_pair(a.z * scale, a.w * scale, h1, q1);
                    split_pair(c.x * scale, c.y * scale, h2, q2);
                    split_pair(c.z * scale, c.w * scale, h3, q3);
                    const int ln = 32 * (cg & 1) + row;
                    L.frag[slot][cg >> 1][0][ln] = __builtin_bit_cast(f16x8, u32x4{h0, h1, h2, h3});
                    L.frag[slot][cg >> 1][1][ln] = __builtin_bit_cast(f16x8, u32x4{q0, q1, q2, q3});
                }
                if (lane == 0) L.pinv[slot] = inv * (1.0f / kOpScale);
                lds_release();
                if (lane == 0) lds_store(&L.ready[slot], z);
                NFFT_PHASE(3);
#ifdef NFFT_HIP_TRACE
                ph[5] += 1;
#endif
                return true;
            };
            int z = next_needed(z_begin);
            if (z >= z_end) return;
            Tile ta, tb;
            load_plane(z, ta);
            while (true) {
                int zn = next_needed(z + 1);
                load_plane(zn < z_end ? zn : z, tb);
                if (!stage(z, ta) || zn >= z_end) break;
                z = zn;
                zn = next_needed(z + 1);
                load_plane(zn < z_end ? zn : z, ta);
                if (!stage(z, tb) || zn >= z_end) break;
                z = zn;
            }
        };
        const bool edge_pencil = __builtin_amdgcn_ballot_w64(straddle != 0) != 0ull;  // (wave-uniform)
        if (edge_pencil) sweep(std::true_type{});
        else sweep(std::false_type{});
#ifdef NFFT_HIP_TRACE
        if (phase_on && lane == 0) {
            for (int k = 0; k < 6; ++k) *NFFT_PHASE_AT(k) = ph[k];
            *NFFT_PHASE_AT(6) = edge_pencil;
        }
#endif
    } else {
        // ================================ consumer: blocks from the queue ===========================================
        // A wave claims its next block while it still works on the current one and fetches that block's points (sorted
        // position, output index) early.  Near the end of the queue blocks are claimed only when the wave is ready
        // for them, so that no wave sits on a block while others run dry.
        int run = 0;  // run of the last claimed block's first point: only moves forward
#ifdef NFFT_HIP_TRACE
        const bool phase_on = !OVERFLOW && wave == 0 && g_stream_phase;
        unsigned long long ph[3] = {0, 0, 0}, ph_t = __builtin_amdgcn_s_memtime();
#endif
        auto claim = [&]() {
            // all 64 lanes add 1 (one ds_add of 64 per wave): the counter runs in units of 64
            return __builtin_amdgcn_readfirstlane(atomicAdd(&L.next_block, 1)) >> 6;
        };
        // my point of block `blk` (index into the plan, -1: none), the block's group
        auto fetch = [&](const int blk, int &idx, int &grp, float &a0, float &a1, float &a2, int &pm) {
            while (L.run_blk[run + 1] <= blk) ++run;
            const int s = run / NG;
            grp = run - s * NG;
            const int t = s % TC;
            const int cum = L.run_cum[run];
            // position of the block's first point inside its run, then mine: walk the group's runs of the chunk
            int x = 32 * (((cum + 31) >> 5) + blk - L.run_blk[run]) - cum + r32;
            idx = -1;
#pragma unroll
            for (int k = 0; k < TC; ++k) {
                if (t + k < TC && s + k < nsl) {  // wave-uniform
                    const int e = run + k * NG;
                    const int st = L.run_start[e], len = L.run_start[e + 1] - st;
                    if (idx < 0 && x >= 0) {
                        if (x < len) idx = st + x;
                        x -= len;  // (negative once found)
                    }
                }
            }
            a0 = a1 = a2 = 0.0f;
            pm = 0;
            if (idx >= 0) {
                const f32x4 v = *(const f32x4 *)(spos + (int64_t)idx * 4);  // plan record {p0, p1, p2, x}: one aligned load
                a0 = v.x; a1 = v.y; a2 = v.z;
                pm = __float_as_int(v.w);  // index of the point in the caller's arrays
            }
        };
        int blk = claim();
        int idx = -1, grp = 0, pj = 0;
        float q0 = 0.0f, q1 = 0.0f, q2 = 0.0f;
        if (blk < total_blocks) fetch(blk, idx, grp, q0, q1, q2, pj);
        while (blk < total_blocks && !lds_load(&L.abort)) {
            const bool ahead = blk + 2 * kIsConsumers <= total_blocks;
            int nblk = total_blocks, nidx = -1, ngrp = 0, npj = 0;
            float n0 = 0.0f, n1 = 0.0f, n2 = 0.0f;
            if (ahead) {
                nblk = claim();
                if (nblk < total_blocks) fetch(nblk, nidx, ngrp, n0, n1, n2, npj);
            }
            const bool valid = idx >= 0;
            int c0 = 0, c1 = 0, c2 = 0;
            float f0 = 0.f, f1 = 0.f, f2 = 0.f;
            if (valid) {
                split_cell(q0, M, c0, f0);
                split_cell(q1, M, c1, f1);
                split_cell(q2, M, c2, f2);
            }
            // the points of a block are ordered by slab: its planes run from the first point's window to the last one's
            const int nvalid = __builtin_popcountll(__builtin_amdgcn_ballot_w64(valid && h == 0));
            const int z_first = __builtin_amdgcn_readlane(c0, 0) - m;
            const int z_last = __builtin_amdgcn_readlane(c0, nvalid - 1) + m + 1;
            // planes below z_first are no longer mine: the fragment reads of the previous block must have completed
            // before a producer sees this and overwrites their slots
            lds_release();
            if (lane == 0) lds_store(&L.progress[wave], z_first);
            const int ks0 = NG == 3 ? grp : 0;  // first k-step of the block's group

            // B fragments: psi2 of my point on the padded columns 16 (ks0 + ks) + 8 h + jj (zero outside the window).
            // d = f2 + k with the integer k = m - l2, l2 = column - o2: k is the exact difference of a per-lane base and the
            // column, and the exponent sc d^2 + 11 is evaluated as k (sc k + 2 sc f2) + (sc f2^2 + 11) -- the same three
            // packed instructions per pair of taps as forming d = (f2 + base) - column and squaring it, which rounded the
            // fraction to the ulp of the base (up to 60 columns into the tile: 2^-18 from column 32 on), an error of up to
            // 2e-5 in the taps of the points at the far end of a pencil and 2.3e-6 in their outputs at m = 1
            // (profiles/r14_value_widths.md).  The scale 2^11 of the operand rides in the exponent; padding lanes get a
            // base far outside every window.
            u32x4 bh[NKS], bl[NKS];
            const int o2h = c2 - tb2 - 8 * h - 16 * ks0;  // padded column of tap 0, minus this lane's column offset
            const float kbase2 = valid ? (float)(m + o2h) : 1.0e4f;
            const float lin2 = 2.0f * sc * f2, con2 = fmaf(sc * f2, f2, 11.0f);
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) {
                // (packed fp32 math: two values per VALU instruction for the three arithmetic steps)
                float w[8];
#pragma unroll
                for (int jj = 0; jj < 8; jj += 2) {
                    const f32x2 k = f32x2{kbase2, kbase2} - f32x2{(float)(16 * ks + jj), (float)(16 * ks + jj + 1)};
                    const f32x2 arg = __builtin_elementwise_fma(k, __builtin_elementwise_fma(k, f32x2{sc, sc}, f32x2{lin2, lin2}),
                                                                f32x2{con2, con2});
                    const float e0 = __builtin_amdgcn_exp2f(arg.x), e1 = __builtin_amdgcn_exp2f(arg.y);  // exp2(sc d^2) * kOpScale
                    w[jj] = (unsigned)(16 * ks + jj - o2h) < (unsigned)W ? e0 : 0.0f;
                    w[jj + 1] = (unsigned)(16 * ks + jj + 1 - o2h) < (unsigned)W ? e1 : 0.0f;
                }
                unsigned h0, h1, h2, h3, p0, p1, p2, p3;
                split_pair(w[0], w[1], h0, p0);
                split_pair(w[2], w[3], h1, p1);
                split_pair(w[4], w[5], h2, p2);
                split_pair(w[6], w[7], h3, p3);
                bh[ks] = u32x4{h0, h1, h2, h3};
                bl[ks] = u32x4{p0, p1, p2, p3};
            }
            // psi1 of my point on the 16 rows this lane holds of every T_z (MFMA result layout): row = r + 8 q + 4 h;
            // kept as pairs (registers 2 p, 2 p + 1) for the packed FMAs of the reduction
            f32x2 w1[8];
            const int o1h = c1 - tb1 - 4 * h;
            const float kbase1 = (float)(m + o1h);  // (the integer part first, as above)
            const float lin1 = 2.0f * sc * f1, con1 = sc * f1 * f1;
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                const int rq0 = ((2 * p) & 3) + 8 * ((2 * p) >> 2), rq1 = rq0 + 1;
                const f32x2 k = f32x2{kbase1, kbase1} - f32x2{(float)rq0, (float)rq1};
                const f32x2 arg = __builtin_elementwise_fma(k, __builtin_elementwise_fma(k, f32x2{sc, sc}, f32x2{lin1, lin1}),
                                                            f32x2{con1, con1});
                const float e0 = __builtin_amdgcn_exp2f(arg.x), e1 = __builtin_amdgcn_exp2f(arg.y);
                w1[p].x = (unsigned)(rq0 - o1h) < (unsigned)W ? e0 : 0.0f;
                w1[p].y = (unsigned)(rq1 - o1h) < (unsigned)W ? e1 : 0.0f;
            }

            float y = 0.0f;
            bool bail = false;
            // All planes of the block first (one poll reads the 16 flags: lane s looks at slot s), then a loop without
            // flag round trips.  One A-fragment buffer per k-step: as soon as the MFMAs of (z, ks) are issued the
            // fragments of (z + 1, ks) are requested into the same registers -- the other k-steps' MFMAs and the
            // reduction cover the LDS latency, which under this load is several hundred cycles.
            {
                const int zs = z_first + ((lane - z_first) & (kIsRing - 1));  // the plane of my window that lives in slot `lane`
                const bool need = lane < kIsRing && zs <= z_last;
                int spins = 0;
                NFFT_PHASE(1);
                while (true) {
                    const int v = need ? lds_load(&L.ready[lane]) : zs;
                    if (__builtin_amdgcn_ballot_w64(v != zs) == 0ull) break;
                    if (lds_load(&L.abort) || ++spins > kSpinLimit) { bail = true; break; }
                    __builtin_amdgcn_s_sleep(2);
                }
                NFFT_PHASE(0);
#ifdef NFFT_HIP_TRACE
                ph[2] += 1;
#endif
                lds_acquire();
            }
            if (bail) {
                // the host learns of it (nfft_hip_check_status): the rows this item has not written stay undefined
                lds_store(&L.abort, 1);
                if (lane == 0) report_fault(status, kFaultStreamStall);
                break;
            }
            {
                f16x8 A[NKS][2];
                const float pinv_first = L.pinv[z_first & (kIsRing - 1)];
                {
                    // same request order as in the loop (the compiler's wait counts merge both paths into the loop head)
                    const int slot = z_first & (kIsRing - 1);
#pragma unroll
                    for (int ks = 0; ks < NKS; ++ks) {
                        __builtin_amdgcn_sched_barrier(0);
                        A[ks][0] = L.frag[slot][ks0 + ks][0][lane];
                        A[ks][1] = L.frag[slot][ks0 + ks][1][lane];
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                auto plane_weight = [&](const int z, const float pinv) {
                    // axis-0 weight of plane z for my point (zero outside its window), times the plane's scale
                    const int l0 = z - (c0 - m);
                    const float d0 = f0 + (float)(m - l0);
                    const float p0 = __builtin_amdgcn_exp2f(sc * d0 * d0) * pinv;
                    return (unsigned)l0 < (unsigned)W ? p0 : 0.0f;
                };
                float pw = plane_weight(z_first, pinv_first);
                for (int z = z_first; z <= z_last; ++z) {
                    const int nz = min(z + 1, z_last);  // (the last plane re-reads itself: no branch in the loop body)
                    const int nslot = nz & (kIsRing - 1);
                    // requested before the fragments: LDS answers in order, waiting for it must not wait for them
                    const float pinv_next = L.pinv[nslot];
                    __builtin_amdgcn_sched_barrier(0);
                    f32x16 acc = 0.0f;
#pragma unroll
                    for (int ks = 0; ks < NKS; ++ks) {
                        const f16x8 bhk = __builtin_bit_cast(f16x8, bh[ks]), blk2 = __builtin_bit_cast(f16x8, bl[ks]);
                        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[ks][0], bhk, acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[ks][0], blk2, acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[ks][1], bhk, acc, 0, 0, 0);
                        __builtin_amdgcn_sched_barrier(0);
                        A[ks][0] = L.frag[nslot][ks0 + ks][0][lane];
                        A[ks][1] = L.frag[nslot][ks0 + ks][1][lane];
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    const float pw_next = plane_weight(nz, pinv_next);
                    f32x2 t = {0.0f, 0.0f};
#pragma unroll
                    for (int p = 0; p < 8; ++p)
                        t = __builtin_elementwise_fma(w1[p], f32x2{acc[2 * p], acc[2 * p + 1]}, t);  // v_pk_fma_f32
                    y = fmaf(pw, t.x + t.y, y);
                    pw = pw_next;
                }
            }
            y += __shfl_xor(y, 32);  // the two row halves of the point
            if (valid && h == 0) yr[(int64_t)pj * Cr + cr] = y * norm;
            if (!ahead) {
                nblk = claim();
                if (nblk < total_blocks) fetch(nblk, nidx, ngrp, n0, n1, n2, npj);
            }
            blk = nblk; idx = nidx; grp = ngrp; pj = npj;
            q0 = n0; q1 = n1; q2 = n2;
        }
#ifdef NFFT_HIP_TRACE
        NFFT_PHASE(1);
        if (phase_on && lane == 0) {
            *NFFT_PHASE_AT(8) = ph[0];
            *NFFT_PHASE_AT(9) = ph[1];
            *NFFT_PHASE_AT(10) = ph[2];
        }
#endif
        // nothing of the ring is mine any more: the producers may run to the end of their sweep
        lds_release();
        if (lane == 0) lds_store(&L.progress[wave], INT_MAX);
    }
    NFFT_GTRACE_END();
    }  // work items
}

} // namespace

#ifdef NFFT_HIP_TRACE
extern "C" int nfft_dbg_set_stream_trace(void *device_buffer)
{
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_stream_trace), &device_buffer, sizeof(device_buffer));
}
extern "C" int nfft_dbg_set_stream_phase(void *device_buffer)  // 16 words per workgroup, as g_stream_trace's 8
{
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_stream_phase), &device_buffer, sizeof(device_buffer));
}
#endif

bool interp_stream_pays(const Geom &g, const PlanLayout &L, int64_t n)
{
    return stream_items(n, range_split(g, L, n).nsets, device_cu_count(), g.M);
}

bool interp_stream_supported(const Geom &g) { return g.dim == 3 && g.wide && !g.owned && g.W <= 16; }

int launch_interp_stream(const Geom &g, const PlanLayout &L, const void *plan, const float *grid, int64_t n, int64_t Cr,
                         int64_t plane0, int64_t nplanes, float *yr, int *tickets, hipStream_t stream)
{
    if (nplanes <= 0 || n <= 0) return 0;
    const int *gs = (const int *)((const char *)plan + L.off_groups);
    return with_window<7>(g.m, "matrix-core interpolation supports cutoff 1..7", [&](auto w) {
        constexpr int W = decltype(w)::value;
        int *const status = device_status_block();
        const auto launch = [&](auto kernel, dim3 blocks, const RangeArgs &a) {
            hipLaunchKernelGGL(kernel, blocks, dim3(kIsThreads), sizeof(StreamLds), stream, g, a.tile_offsets, gs, a.spos, grid,
                               (int)Cr, (int)plane0, yr, a.work, a.sorted, a.tickets, status);
        };
        return L.grouped ? launch_range_kernels<interp_stream_kernel<W, false, 3>, interp_stream_kernel<W, true, 3>>(
                               g, L, plan, n, nplanes, sizeof(StreamLds), tickets, launch)
                         : launch_range_kernels<interp_stream_kernel<W, false, 1>, interp_stream_kernel<W, true, 1>>(
                               g, L, plan, n, nplanes, sizeof(StreamLds), tickets, launch);
    });
}

} // namespace nfft
