// C-ABI entry points (include/nfft_hip.h): validation, workspace carving and stage orchestration.
//
// Host drivers being replaced: nfft_adjoint_cuda (csrc/cuda/core_cuda.cu:144-336) and
// nfft_forward_cuda (:340-531) of the reference, including its validators check_point_input (:38-66),
// check_spatial_coeffs_input (:69-86), check_spectral_coeffs_input (:89-115) and
// setup_spectral_dimensions (:118-137).  Differences in behaviour, all on the safe side:
//   * nothing synchronises the device and nothing is allocated or freed here (the reference issues six
//     cudaDeviceSynchronize and four cudaMalloc/cudaFree per call);
//   * errors are returned (the reference calls exit() on a CUDA error, cuda_utils.cu:7-14);
//   * the preconditions the reference only documents (1 <= m, 2m+2 <= 2N, N even) are checked.
#include "../../include/nfft_hip.h"

#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "common.h"
#include "host_util.h"
#include "kernels.h"
#include "range_items.h"

namespace nfft {

static thread_local std::string g_last_error;
void set_error(const std::string &msg) { g_last_error = msg; }

// ---- optional stage timing -------------------------------------------------------------------
namespace {
struct TimedSpan { int stage; hipEvent_t start, stop; };
std::atomic<bool> g_profile{false};
std::atomic<unsigned> g_profile_stages{~0u};  // stages that are timed while g_profile is set (bit s = stage s)
std::mutex g_spans_mutex;  // guards g_spans / g_free_events (the entry points may be called from several threads)
std::vector<TimedSpan> g_spans;
std::vector<hipEvent_t> g_free_events;
hipEvent_t get_event()
{
    if (!g_free_events.empty()) { hipEvent_t e = g_free_events.back(); g_free_events.pop_back(); return e; }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}
} // namespace

StageTimer::StageTimer(Stage stage, hipStream_t s) : slot(-1), stream(s)
{
    if (!g_profile.load(std::memory_order_relaxed)) return;
    if (!((g_profile_stages.load(std::memory_order_relaxed) >> (int)stage) & 1u)) return;
    std::lock_guard<std::mutex> lock(g_spans_mutex);
    TimedSpan sp{(int)stage, get_event(), get_event()};
    (void)hipEventRecord(sp.start, stream);
    slot = (int)g_spans.size();
    g_spans.push_back(sp);
}
StageTimer::~StageTimer()
{
    if (slot < 0) return;
    std::lock_guard<std::mutex> lock(g_spans_mutex);
    if (slot < (int)g_spans.size()) (void)hipEventRecord(g_spans[slot].stop, stream);
}

int current_device()
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) dev = 0;
    return dev;
}

// CU count of the CURRENT device (cached per device: a process may drive several)
int device_cu_count()
{
    static std::atomic<int> cache[kMaxDevices];
    const int dev = current_device();
    if (dev >= kMaxDevices) return 256;
    int v = cache[dev].load(std::memory_order_relaxed);
    if (v <= 0) {
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
        cache[dev].store(v, std::memory_order_relaxed);
    }
    return v;
}

bool DeviceOnce::first_use()
{
    const int dev = current_device();
    if (dev >= kMaxDevices) return true;
    return !done[dev].load(std::memory_order_acquire);
}
void DeviceOnce::mark()
{
    const int dev = current_device();
    if (dev < kMaxDevices) done[dev].store(true, std::memory_order_release);
}

// ---- device-side failure reports (common.h) ---------------------------------------------------------------
namespace {
std::mutex g_status_mutex;
int *g_status_host = nullptr;      // pinned, portable: kMaxDevices blocks of kStatusInts ints
bool g_status_failed = false;
int *status_host_blocks()
{
    std::lock_guard<std::mutex> lock(g_status_mutex);
    if (!g_status_host && !g_status_failed) {
        void *p = nullptr;
        if (hipHostMalloc(&p, sizeof(int) * kStatusInts * kMaxDevices, hipHostMallocPortable | hipHostMallocMapped) == hipSuccess && p) {
            std::memset(p, 0, sizeof(int) * kStatusInts * kMaxDevices);
            g_status_host = (int *)p;
        } else {
            (void)hipGetLastError();
            g_status_failed = true;  // no reports on this platform; the kernels get a null pointer
        }
    }
    return g_status_host;
}
const char *const kFaultText[kNumFaults] = {
    "device fault: the streamed interpolation kernel gave up waiting inside a work item (bounded spin ran out); "
    "the result of that forward transform is invalid",
    "Input mismatch: batch holds an index outside [0, batch_size) (the batch vector must be sorted with "
    "batch[-1] + 1 == batch_size)",
    "Input mismatch: the batch vector is not sorted (a row carries another index than its point set's row range, or a "
    "coefficient exceeds the largest one of its range)",
    "stale point plan: pos or batch were modified (behind the version counter) after the cached plan was built; the "
    "transform that used it is invalid -- clear or disable the plan cache (torch_nfft_amd.ops.plan_cache_clear)",
};
}  // namespace

int *device_status_block()
{
    int *host = status_host_blocks();
    const int dev = current_device();
    if (!host || dev >= kMaxDevices) return nullptr;
    void *d = nullptr;
    if (hipHostGetDevicePointer(&d, host + dev * kStatusInts, 0) != hipSuccess || !d) {
        (void)hipGetLastError();
        return nullptr;
    }
    return (int *)d;
}

int take_pending_fault()
{
    int *host = status_host_blocks();
    const int dev = current_device();
    if (!host || dev >= kMaxDevices) return 0;
    volatile int *blk = host + dev * kStatusInts;
    for (int k = 0; k < kNumFaults; ++k) {
        if (blk[k]) {
            blk[k] = 0;
            set_error(kFaultText[k]);
            return k == kFaultStreamStall ? NFFT_HIP_EKERNEL : NFFT_HIP_EINVAL;
        }
    }
    return 0;
}

// ---- environment switches ------------------------------------------------------------------------------------------
// Every NFFT_HIP_* variable the library reads (INTEGRATION.md lists them).  All but two are read together, once per
// process; NFFT_HIP_CHUNK_BYTES, NFFT_HIP_NO_COLFFT and NFFT_HIP_TOEPLITZ_FUSED are read on every call (tests change
// them between calls).
namespace {
const char *env(const char *name)
{
    const char *v = std::getenv(name);
    return v ? v : "";
}
struct Switches {
    SpreadMode spread;    // NFFT_HIP_SPREAD=reg|lds: register-tile / LDS-atomic spreading instead of the matrix cores
    char gather;          // NFFT_HIP_GATHER=lds|mfma: 'l' lane-per-point gather only, 'm' never the wave-per-column or
                          // streamed kernels; 0 by default
    int owned;            // NFFT_HIP_OWNED=0|1: never / always the owner-computes plan; -1: by point density
    bool work_list;       // NFFT_HIP_WORK_LIST=1: every wide plan runs from its work list
    bool colgroups;       // NFFT_HIP_COLGROUPS=0: plans without the column-group order
    bool small_grid;      // NFFT_HIP_SMALL_GRID=0: no one-kernel path for small grids
    bool small_narrow;    // NFFT_HIP_SMALL_NARROW=0: the 64^3 grid keeps the wide tiling
    int stream_min;       // NFFT_HIP_STREAM_MIN (tuning): smallest streamed work item in points; 3000
    double items_per_cu;  // NFFT_HIP_ITEMS_PER_CU (tuning): work items per CU the items of a pencil are sized for; 5.4
    bool fine_tail;       // NFFT_HIP_FINE_TAIL=0 (tuning): no finer ranges for the last pencils of a launch of several rounds
    int grade;            // NFFT_HIP_GRADE=1|2 (tuning): work items cut per pencil by point count with a graded tail, for launches
                          // of more than one round of workgroups / always; 0 (default): equal ranges of slabs
};
const Switches &switches()
{
    static const Switches s = [] {
        Switches w;
        const char *v = env("NFFT_HIP_SPREAD");
        w.spread = v[0] == 'r' ? kSpreadReg : v[0] == 'l' ? kSpreadLds : kSpreadMfma;
        v = env("NFFT_HIP_GATHER");
        w.gather = (v[0] == 'l' || v[0] == 'm') ? v[0] : 0;
        v = env("NFFT_HIP_OWNED");
        w.owned = v[0] == '0' ? 0 : v[0] == '1' ? 1 : -1;
        w.work_list = env("NFFT_HIP_WORK_LIST")[0] == '1';
        w.colgroups = env("NFFT_HIP_COLGROUPS")[0] != '0';
        w.small_grid = env("NFFT_HIP_SMALL_GRID")[0] != '0';
        w.small_narrow = env("NFFT_HIP_SMALL_NARROW")[0] != '0';
        const int sm = std::atoi(env("NFFT_HIP_STREAM_MIN"));
        w.stream_min = sm > 0 ? sm : 3000;
        const double ipc = std::atof(env("NFFT_HIP_ITEMS_PER_CU"));
        w.items_per_cu = ipc >= 1.0 && ipc <= 64.0 ? ipc : 5.4;
        w.fine_tail = env("NFFT_HIP_FINE_TAIL")[0] != '0';
        v = env("NFFT_HIP_GRADE");
        w.grade = v[0] == '1' ? 1 : v[0] == '2' ? 2 : 0;
        return w;
    }();
    return s;
}
// upper bound for (real grid + half spectrum) of one chunk of planes; the rest of the 288 GB stays free for the caller
int64_t chunk_budget_bytes()
{
    const long long v = std::atoll(env("NFFT_HIP_CHUNK_BYTES"));
    return v > 0 ? (int64_t)v : int64_t(16) << 30;
}
bool colfft_enabled() { return env("NFFT_HIP_NO_COLFFT")[0] != '1'; }
bool toeplitz_fused_enabled() { return env("NFFT_HIP_TOEPLITZ_FUSED")[0] != '0'; }
} // namespace

SpreadMode spread_mode() { return switches().spread; }
bool column_groups_enabled() { return switches().colgroups; }
bool work_list_forced() { return switches().work_list; }
double items_per_cu() { return switches().items_per_cu; }
int grading_mode() { return switches().grade; }
bool fine_tail_enabled() { return switches().fine_tail; }
int stream_min_item_points() { return switches().stream_min; }
int owned_override() { return switches().owned; }

// ---- the route of a call -------------------------------------------------------------------------------------------
// Which kernels a call runs is decided here and nowhere else: the kernel files' *_supported functions only say whether
// a kernel can run a geometry.  Every entry point builds a Route and reads nothing else.
namespace {

// Geometry of a problem's (halo-tiling) plan.  The column-group order of the plan (common.h Geom::CG) pays where the
// streamed gather runs, i.e. for big work items; below that it only costs sorting time (+0.03 ms at 10^6 points).
// The 64^3 grid (N = 32, the reference's default bandwidth: torch_nfft/nfft.py:150-156) is 3 x 2 pencils of the wide tiling,
// two of which hold 70 % of the cells: the matrix-core kernels' work items (ranges of slabs of one pencil, at most 16 pieces
// per range) cannot spread a dense point set over 256 CUs -- 10^6 points, m = 3: 1.46 ms per adjoint + forward against 0.51
// with the narrow tiling, whose LDS kernels share a (pencil, segment) among up to 32 workgroups.  What the narrow path pays is
// one LDS atomic per window tap: it wins for the narrow windows and for few points (sweep: profiles/r04_experiments.md).
bool prefer_narrow(const nfft_hip_problem *p)
{
    if (!switches().small_narrow || p->dim != 3) return false;
    // 128^3 grid, narrow window, many point sets: every (set, pencil) is a chain of nearly empty K-blocks (2e4 points per set:
    // 9 per pencil and slab), and from eight sets up there are more chains than CUs -- 16 sets x 2e4 points, m = 2: 1.17 ms
    // against 0.90 on the narrow tiling; with four sets the matrix-core path is still ahead (0.42 against 0.45)
    // (one column only: with eight columns and 2e4 points per set the paired owner-computes spreading is 5x ahead of the LDS
    // kernel, 0.24 against 1.28 ms)
    if (p->N == 64) return p->m <= 3 && p->batch_size >= 8 && p->num_columns == 1;
    if (p->N != 32) return false;
    return p->m <= 3 || p->num_points <= 30000;
}
Geom problem_geom(const nfft_hip_problem *p)
{
    Geom g = make_geom(p->dim, p->N, p->m, false, false, prefer_narrow(p));
    if (g.CG > 1 && !stream_items(p->num_points, p->batch_size, device_cu_count(), g.M)) g.CG = 1;
    return g;
}

// Grids of at most 4096 cells run as one kernel per direction when no plan is supplied (smallgrid.hip).  Average window
// taps per point set: a set is ONE workgroup's loop, ~0.35 ns per tap and direction (LDS atomics of a single CU) on top of
// ~25 us per adjoint + forward pair, against 80-145 us for the general path on these sizes -- measured break-even ~10^5
// taps (profiles/r03_experiments.md).  8e4 since round 4: the reference's own test shape (test/test_adjoint.py: 2-D N = 16,
// m = 3, 1 000 points per set = 64 000 taps) sat just above the first limit of 6e4 and took the general path (0.122 ms
// against 0.07 here, profiles/r04_experiments.md)
bool small_grid_route(const nfft_hip_problem *p)
{
    if (!switches().small_grid || !small_grid_supported(p)) return false;
    int64_t taps = 1;
    for (int k = 0; k < p->dim; ++k) taps *= 2 * p->m + 2;
    const int64_t sets = p->batch_size < 1 ? 1 : (p->batch_size > 8 ? 8 : p->batch_size);
    return p->num_points * taps <= int64_t(80000) * sets;
}

enum GatherKernel { kGatherCols, kGatherStream, kGatherRing, kGatherLanes };
// FFT stage of a chunk: full rocFFT + the roll-off kernel; rocFFT rows + the pruned column passes; own rows + the planar
// column passes (column_layout transposes for C > 1); own rows + the column-innermost passes (C > 1, >= 32 planes)
enum FftRoute { kFftFull, kFftRocRows, kFftOwnPlanar, kFftOwnCi };

struct Route {
    // The point plan: the tile-sorted points (pencils with halo: what the interpolation kernels and the scatter spreading
    // kernels walk) and, for sparse 3-D problems, a second sort by owned tiles with an entry per touched tile for the
    // owner-computes spreading kernel (common.h choose_owned), stored behind the first.
    Geom g;
    PlanLayout L;
    bool owned;
    Geom go;
    PlanLayout Lo;
    int64_t off_own, plan_bytes;
    int64_t n, B, Cr;       // points, point sets, real planes per point set
    SpreadMode spread;      // spreading kernel: matrix cores, register tiles or LDS atomics
    bool x_through_plan;    // the spreading kernel reads x through the plan (no gather_rows pass)
    GatherKernel gather;
    // FFT stage (make_route only)
    FftRoute fft;           // kFftFull, kFftRocRows or kFftOwnPlanar; chunk_fft() says when a chunk goes column-innermost
    bool ci;                // several columns on a grid the column-innermost passes take
    bool toeplitz_fused;    // normal operator: both row passes and the product with K in one kernel (toeplitz_fused_chunk)
    int64_t C, ppc, total_planes, chunk_planes, half_cells;
    // the workspace carve; off_part and the `end` it continues from: forward_grad_route
    int64_t off_plan, off_xs, off_xmax, off_grid, off_spec, off_col, off_work, off_tickets, off_part, work_bytes, end, total;

    const Geom &spread_geom() const { return owned ? go : g; }
    const PlanLayout &spread_layout() const { return owned ? Lo : L; }
    const void *spread_plan(const void *plan) const { return owned ? (const char *)plan + off_own : (const char *)plan; }
    // the column-innermost passes need at least two groups of 16 planes
    FftRoute chunk_fft(int64_t np) const { return fft == kFftOwnPlanar && ci && np >= 32 ? kFftOwnCi : fft; }
};

// body(p0, np) for every chunk of planes [p0, p0 + np) of the route, in order; stops at the first non-zero return code
template <class F>
int for_chunks(const Route &r, F &&body)
{
    for (int64_t p0 = 0; p0 < r.total_planes; p0 += r.chunk_planes)
        if (int rc = body(p0, std::min(r.chunk_planes, r.total_planes - p0))) return rc;
    return 0;
}

// bytes of a band spectrum [B, N^dim, C] complex64
int64_t band_size_of(const nfft_hip_problem *p)
{
    int64_t band = p->batch_size * p->num_columns * 8;
    for (int d = 0; d < p->dim; ++d) band *= p->N;
    return band;
}

// The least workspace of a gradient gather, the partial gradients plus one chunk of grid planes: a missing workspace, or
// one below this, is refused before the route makes its rocFFT plans.
int64_t grad_least_bytes(const nfft_hip_problem *p, int real_output)
{
    const int64_t Cr = p->num_columns * (real_output ? 1 : 2);
    return (Cr > 1 ? Cr * p->num_points * p->dim * 4 : 0) + problem_geom(p).cells * 4 * (real_output ? 1 : 2);
}

// fastsum geometry: every point within radius 1/4 (the kernel is only defined there)
void quarter_ball(const nfft_hip_problem *in, nfft_hip_problem &out)
{
    out = *in;
    out.flags |= NFFT_HIP_POINTS_IN_QUARTER_BALL;
}

// Plans and point-side kernels of a problem whose calls have Cr real planes per point set.
Route plan_route(const nfft_hip_problem *p, int64_t Cr)
{
    Route r{};
    r.g = problem_geom(p);
    r.L = plan_layout(r.g, p->num_points, p->batch_size);
    r.owned = choose_owned(p->dim, p->N, p->m, p->num_points, p->batch_size,
                           (p->flags & NFFT_HIP_POINTS_IN_QUARTER_BALL) ? 0.125 : 1.0);
    // (a single column on a 128^3 grid: what the owner-computes kernel saves -- 10 us of zero-fill, the atomics of a few
    // thousand K-blocks -- is less than its second sort costs: plan 0.074 against 0.038 ms at 2e4 points, round 4)
    if (p->N < 128 && p->num_columns < 2 && owned_override() < 0) r.owned = false;
    if (!r.g.wide) r.owned = false;  // (the narrow tiling was preferred: no matrix-core spreading, no owned plan)
    r.go = r.g;
    r.Lo = r.L;
    r.plan_bytes = r.L.total;
    if (r.owned) {
        // two or more coefficient columns: 32 x 32 tiles, one sweep of the points per PAIR of columns (spread_mfma.hip)
        r.go = make_geom(p->dim, p->N, p->m, true, p->num_columns >= 2);
        r.Lo = plan_layout(r.go, p->num_points, p->batch_size);
        r.off_own = align_up(r.L.total, 256);
        r.plan_bytes = r.off_own + r.Lo.total;
    }
    r.n = p->num_points;
    r.B = p->batch_size;
    r.Cr = Cr;
    const Geom &gs = r.spread_geom();
    r.spread = spread_mfma_supported(gs) ? kSpreadMfma
             : spread_reg_supported(gs) && spread_mode() == kSpreadReg ? kSpreadReg : kSpreadLds;
    // The matrix-core spreading kernel reads one or two real coefficient columns in place: every plan record carries the
    // index of its point in the caller's arrays and the staging pipeline fetches x[index] two steps ahead of its use -- no
    // permutation pass (0.18 ms at C3 as a kernel of its own, a 23 us latency-bound prologue per work item inside the
    // spreading kernel).  With more columns one pass (gather_rows) reads every row once for all of them.  (The LDS-tile
    // kernel of the narrow tilings reads x through the plan's permutation as well; the register-tile kernel does not.)
    r.x_through_plan = Cr <= 2 && r.spread != kSpreadReg;
    // interpolation on the wide 3-D tiling: the wave-per-column kernel from 4 real columns up (half its waves busy), the
    // streamed one for big work items, else the plane-ring kernel
    const char gsw = switches().gather;
    if (!gsw && interp_cols_supported(r.g) && Cr >= 4) r.gather = kGatherCols;
    else if (!gsw && interp_stream_supported(r.g) && interp_stream_pays(r.g, r.L, r.n)) r.gather = kGatherStream;
    else if (gsw != 'l' && interp_mfma_supported(r.g)) r.gather = kGatherRing;
    else r.gather = kGatherLanes;
    return r;
}

// dxhat of the second-order backward of the point gradient, given the adjoint route of its problem:
// the derivative spreading + the adjoint's FFT stage where the LDS spreading kernel takes the plan's tiling (1-D, 2-D and
// the narrow 3-D tiling), else dim adjoints of omega v_a with the spectral multipliers 2 pi i k_a.  (The wide tiling's
// spreading runs on matrix cores, whose tap weights are a product of per-axis windows: the derivative's sum over the axes
// is not.)  NFFT_HIP_DXHAT=compose takes the composition everywhere (scripts/bench_pos_hvp.py compares the two).
bool hvp_fused_dxhat(const Route &ra)
{
    return spread_deriv_supported(ra.g) && env("NFFT_HIP_DXHAT")[0] != 'c';
}

// The whole route of an adjoint (x: ppc real planes per column), a forward transform (y: ppc real planes per column) or
// an application of the Toeplitz normal operator (the forward FFT stage, the product with the
// kernel grid and the adjoint FFT stage on the same chunk of planes -- no points, no plan, and no roll-off in either
// stage), the chunk size and the workspace carve included.  size_fft_work = false (nfft_dbg_fft_route only: no device needed)
// leaves rocFFT's work area out: every decision is made as usual, but `total` is no workspace size then.
enum RouteKind { kRouteForward, kRouteAdjoint, kRouteToeplitz };
int make_route(const nfft_hip_problem *p, int ppc, RouteKind kind, Route &r, bool size_fft_work = true)
{
    const bool adjoint = kind == kRouteAdjoint, toeplitz = kind == kRouteToeplitz;
    if (toeplitz) {
        // FFT stages only: the grid of the problem, whatever tiling its points would get
        r = Route{};
        r.g = make_geom(p->dim, p->N, p->m);
        r.g.rolloff = 0;
        r.B = p->batch_size;
        r.Cr = p->num_columns * ppc;
    } else {
        r = plan_route(p, p->num_columns * ppc);
    }
    r.C = p->num_columns;
    r.ppc = ppc;
    r.total_planes = r.B * r.Cr;
    r.half_cells = half_cells_of(r.g);
    const bool colfft = colfft_supported(r.g) && colfft_enabled();
    r.fft = !colfft ? kFftFull : rowfft_supported(r.g) ? kFftOwnPlanar : kFftRocRows;
    r.ci = r.C > 1 && colfft_ci_supported(r.g);
    // the normal operator on the planar route with its own row passes: the rows stay in LDS between the two transforms
    // (NFFT_HIP_TOEPLITZ_FUSED=0: the three kernels of the general route, which every other FFT route takes)
    r.toeplitz_fused = toeplitz && r.fft == kFftOwnPlanar && r.C < 2 && toeplitz_fused_enabled();
    // (the work area is sized for the rocFFT row transforms wherever the column passes run)
    const FftKind fkind = colfft ? (adjoint ? kR2CRows : kC2RRows) : (adjoint ? kR2C : kC2R);
    const int64_t plane_bytes = r.g.cells * 4 + r.half_cells * 8 + (colfft ? colfft_scratch_bytes(r.g, 1) : 0);
    // (the budget is a soft one: the group padding of the column-innermost passes, <= 15 planes of scratch, comes on top)
    int64_t chunk = chunk_budget_bytes() / plane_bytes;
    chunk -= chunk % ppc;
    if (chunk < ppc) chunk = ppc;
    if (chunk > r.total_planes) chunk = r.total_planes;
    if (chunk > 32768) chunk = 32768 - 32768 % ppc;  // blockIdx.y limit
    r.chunk_planes = chunk;
    r.work_bytes = 0;
    if (r.total_planes > 0 && size_fft_work) {
        // plans for the full chunk and for the remainder chunk (the normal operator runs both directions)
        const FftKind kinds[2] = {fkind, colfft ? kR2CRows : kR2C};
        const int64_t rem = r.total_planes % chunk;
        for (int i = 0; i < (toeplitz ? 2 : 1); ++i) {
            const FftKind k = kinds[i];
            for (const int64_t planes : {chunk, rem}) {
                if (!planes) continue;
                const int64_t w = fft_work_bytes(k, r.g.dim, r.g.M, planes);
                if (w < 0) return NFFT_HIP_EFFT;
                if (w > r.work_bytes) r.work_bytes = w;
            }
        }
    }
    const bool need_xs = adjoint;
    Carve c;
    r.off_plan = c.take(r.plan_bytes);
    r.off_xs = c.take(need_xs ? (align_up(r.spread_layout().cap * r.Cr, 64) + 64) * 4 : 0);
    r.off_xmax = c.take(need_xs ? r.total_planes * 4 : 0);
    // (the fused normal operator keeps its grid rows in LDS)
    r.off_grid = c.take(r.toeplitz_fused ? 0 : chunk * r.g.cells * 4);
    r.off_spec = c.take(chunk * r.half_cells * 8);
    // (several columns: the column-innermost passes work on whole groups of 16 planes)
    r.off_col = c.take(colfft ? colfft_scratch_bytes(r.g, r.C > 1 ? colfft_ci_planes(chunk) : chunk) : 0);
    r.off_work = c.take(r.work_bytes);
    // (the counters of the persistent work-list launches: every launch of the call in turn, on its stream)
    r.off_tickets = c.take(kTicketPlanes * 4);
    r.end = c.end();
    r.total = c.total();
    return 0;
}

int build_plans(const Route &r, const float *pos, const int64_t *batch, void *plan, hipStream_t s)
{
    if (int rc = launch_plan_points(r.g, r.L, pos, batch, r.n, r.B, plan, s)) return rc;
    if (r.owned) return launch_plan_points(r.go, r.Lo, pos, batch, r.n, r.B, (char *)plan + r.off_own, s);
    return 0;
}

// planes [p0, p0 + np) of the grid; xs: the planar copy in plan order; xr: nullptr when gather_rows has filled xs, else x
// (x_through_plan); xmax: per-plane largest |x| (matrix-core kernel only: launch_plane_absmax); tickets: the work-list
// counters (kernels.h: launch_spread_mfma)
int spread_chunk(const Route &r, const void *plan, const float *xr, float *xs, const unsigned *xmax, int64_t p0, int64_t np,
                 float *grid, int *tickets, hipStream_t s)
{
    const Geom &g = r.spread_geom();
    const PlanLayout &L = r.spread_layout();
    plan = r.spread_plan(plan);
    switch (r.spread) {
    case kSpreadMfma: {
        // (the owner-computes variant writes every cell itself)
        if (!g.owned) { StageTimer t(kStageZero, s); NFFT_HIP_CHECK(hipMemsetAsync(grid, 0, (size_t)(np * g.cells * 4), s)); }
        StageTimer t(kStageSpread, s);
        return launch_spread_mfma(g, L, plan, xr, xs, xmax, r.n, r.Cr, p0, np, grid, tickets, s);
    }
    case kSpreadReg: {
        StageTimer t(kStageSpread, s);
        return launch_spread_reg(g, L, plan, xs, r.n, r.Cr, p0, np, grid, s);
    }
    case kSpreadLds: break;
    }
    { StageTimer t(kStageZero, s); NFFT_HIP_CHECK(hipMemsetAsync(grid, 0, (size_t)(np * g.cells * 4), s)); }
    StageTimer t(kStageSpread, s);
    return launch_spread(g, L, plan, xr, xs, r.n, r.Cr, p0, np, grid, s);
}

int gather_chunk(const Route &r, const void *plan, const float *grid, int64_t p0, int64_t np, float *yr, int *tickets,
                 hipStream_t s)
{
    switch (r.gather) {
    case kGatherCols: return launch_interp_cols(r.g, r.L, plan, grid, r.n, r.Cr, p0, np, yr, tickets, s);
    case kGatherStream: return launch_interp_stream(r.g, r.L, plan, grid, r.n, r.Cr, p0, np, yr, tickets, s);
    case kGatherRing: return launch_interp_mfma(r.g, r.L, plan, grid, r.n, r.Cr, p0, np, yr, tickets, s);
    case kGatherLanes: break;
    }
    return launch_interp(r.g, r.L, plan, grid, r.n, r.Cr, p0, np, yr, s);
}

// FFT stage of the planes [p0, p0 + np) of an adjoint: grid -> spec -> y
int fft_adjoint_chunk(const Route &r, char *ws, float *grid, float2 *spec, int x_is_complex, int real_output, int64_t p0,
                      int64_t np, void *y, const void *mult, int mult_kind, hipStream_t s)
{
    const Geom &g = r.g;
    void *col = ws + r.off_col;
    const FftRoute route = r.chunk_fft(np);
    switch (route) {
    case kFftFull: {
        { StageTimer t(kStageFft, s); if (int rc = fft_execute(kR2C, g.dim, g.M, np, grid, spec, ws + r.off_work, r.work_bytes, s)) return rc; }
        StageTimer t(kStageDeconv, s);
        return launch_deconv_adjoint(g, spec, r.C, x_is_complex, real_output, p0, np, y, mult, mult_kind, s);
    }
    case kFftOwnCi: {
        // several columns: the planes travel in groups of 16, plane index innermost, and the last pass writes the
        // reference's [B, N^3, C] layout directly
        { StageTimer t(kStageFft, s); if (int rc = launch_row_r2c_ci(g, grid, np, spec, s)) return rc; }
        StageTimer t(kStageDeconv, s);
        return launch_colfft_adjoint_ci(g, spec, col, r.C, x_is_complex, real_output, p0, np, y, mult, mult_kind, s);
    }
    case kFftRocRows: {
        StageTimer t(kStageFft, s);
        if (int rc = fft_execute(kR2CRows, g.dim, g.M, np, grid, spec, ws + r.off_work, r.work_bytes, s)) return rc;
        break;
    }
    case kFftOwnPlanar: {
        StageTimer t(kStageFft, s);
        if (int rc = launch_row_r2c(g, grid, col, r.chunk_planes, np, spec, s)) return rc;
        break;
    }
    }
    const bool own_rows = route == kFftOwnPlanar;
    StageTimer t(kStageDeconv, s);
    if (r.C < 2)
        return launch_colfft_adjoint(g, spec, own_rows, col, r.chunk_planes, r.C, x_is_complex, real_output, p0, np, y, mult, mult_kind, s);
    // several columns: the passes write a planar copy (into the grid buffer, free by now), one tiled transpose brings it
    // into the reference's column-interleaved layout
    const int64_t K = g.dim == 2 ? g.N * (int64_t)g.N : g.N * (int64_t)g.N * g.N;
    if (int rc = launch_colfft_adjoint(g, spec, own_rows, col, r.chunk_planes, 1, x_is_complex, real_output, 0, np, grid, mult, mult_kind, s)) return rc;
    return launch_column_layout(true, grid, y, K, r.C, p0 / r.ppc, np / r.ppc, real_output ? 4 : 8, s);
}

// FFT stage of the planes [p0, p0 + np) of a forward transform: xhat -> spec -> grid
int fft_forward_chunk(const Route &r, char *ws, const void *xhat, int x_is_complex, int real_output, int64_t p0, int64_t np,
                      float *grid, float2 *spec, hipStream_t s)
{
    const Geom &g = r.g;
    void *col = ws + r.off_col;
    const FftRoute route = r.chunk_fft(np);
    switch (route) {
    case kFftFull: {
        { StageTimer t(kStageDeconv, s); if (int rc = launch_deconv_forward(g, xhat, r.C, x_is_complex, real_output, p0, np, spec, s)) return rc; }
        StageTimer t(kStageFft, s);
        return fft_execute(kC2R, g.dim, g.M, np, spec, grid, ws + r.off_work, r.work_bytes, s);
    }
    case kFftOwnCi: {
        { StageTimer t(kStageDeconv, s); if (int rc = launch_colfft_forward_ci(g, xhat, spec, col, r.C, x_is_complex, real_output, p0, np, s)) return rc; }
        StageTimer t(kStageFft, s);
        return launch_row_c2r_ci(g, spec, np, grid, s);
    }
    case kFftRocRows:
    case kFftOwnPlanar: break;
    }
    const bool own_rows = route == kFftOwnPlanar;
    {
        StageTimer t(kStageDeconv, s);
        if (r.C < 2) {
            if (int rc = launch_colfft_forward(g, xhat, col, r.chunk_planes, r.C, x_is_complex, real_output, p0, np, spec, own_rows, s)) return rc;
        } else {
            // several columns: planar copy of this chunk's columns first (the grid buffer is free until the row pass)
            const int64_t K = g.dim == 2 ? g.N * (int64_t)g.N : g.N * (int64_t)g.N * g.N;
            if (int rc = launch_column_layout(false, xhat, grid, K, r.C, p0 / r.ppc, np / r.ppc, x_is_complex ? 8 : 4, s)) return rc;
            if (int rc = launch_colfft_forward(g, grid, col, r.chunk_planes, 1, x_is_complex, real_output, 0, np, spec, own_rows, s)) return rc;
        }
    }
    StageTimer t(kStageFft, s);
    if (own_rows) return launch_row_c2r(g, spec, col, r.chunk_planes, np, grid, s);
    return fft_execute(kC2RRows, g.dim, g.M, np, spec, grid, ws + r.off_work, r.work_bytes, s);
}

// The normal operator's planes [p0, p0 + np) on the fused route (Route::toeplitz_fused; one column: np is even):
// xhat -> column passes -> spec -> row passes around the product with K, in place -> column passes -> y
int toeplitz_fused_chunk(const Route &r, char *ws, const void *xhat, int x_is_complex, const float *K, int64_t p0, int64_t np,
                         float2 *spec, void *y, hipStream_t s)
{
    void *col = ws + r.off_col;
    {
        StageTimer t(kStageDeconv, s);
        if (int rc = launch_colfft_forward(r.g, xhat, col, r.chunk_planes, r.C, x_is_complex, 0, p0, np, spec, true, s)) return rc;
    }
    {
        StageTimer t(kStageFft, s);
        if (int rc = launch_row_toeplitz(r.g, spec, K, r.Cr / 2, p0 / 2, np / 2, s)) return rc;
    }
    StageTimer t(kStageDeconv, s);
    return launch_colfft_adjoint(r.g, spec, true, col, r.chunk_planes, r.C, 1, 0, p0, np, y, nullptr, 0, s);
}

int validate(const nfft_hip_problem *p)
{
    if (!p) { set_error("Input mismatch: null problem"); return NFFT_HIP_EINVAL; }
    if (p->dim < 1 || p->dim > 3) { set_error("Input mismatch: dim must be 1, 2 or 3"); return NFFT_HIP_EINVAL; }
    if (p->num_points < 0 || p->num_columns < 0 || p->batch_size < 1) {
        set_error("Input mismatch: negative size");
        return NFFT_HIP_EINVAL;
    }
    if (p->N < 2 || (p->N & 1)) { set_error("Input mismatch: bandwidth N must be even and >= 2"); return NFFT_HIP_EINVAL; }
    if (p->m < 1 || p->m > kMaxCutoff) { set_error("Input mismatch: cutoff m must be in 1..8"); return NFFT_HIP_EINVAL; }
    if (2 * p->m + 2 > 2 * p->N) { set_error("Input mismatch: window 2m+2 exceeds the oversampled grid 2N"); return NFFT_HIP_EINVAL; }
    if (p->N > (1 << 20)) { set_error("Input mismatch: bandwidth too large"); return NFFT_HIP_EINVAL; }
    if (p->num_points >= (int64_t(1) << 31)) { set_error("Input mismatch: too many points"); return NFFT_HIP_EINVAL; }
    {
        // the point plan indexes its (point set, tile) bins with 32-bit integers
        const Geom g = problem_geom(p);
        if ((double)g.tiles_per_batch * (double)p->batch_size * (double)g.SB >= 2.0e9) {
            set_error("Input mismatch: too many point sets for this grid (plan bins exceed 2^31)");
            return NFFT_HIP_EINVAL;
        }
    }
    return 0;
}

} // namespace
} // namespace nfft

using namespace nfft;

extern "C" {

int nfft_hip_abi_version(void) { return NFFT_HIP_ABI_VERSION; }
const char *nfft_hip_last_error(void) { return g_last_error.c_str(); }

int nfft_hip_check_status(void *stream, int synchronize)
{
    if (synchronize) NFFT_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    return take_pending_fault();
}

void nfft_hip_profile_enable(int enable)
{
    g_profile.store(enable != 0);
}

void nfft_hip_profile_stages(unsigned stage_mask)
{
    g_profile_stages.store(stage_mask);
}

int nfft_hip_profile_collect(double *ms_per_stage, int64_t *launches_per_stage, int num_stages)
{
    for (int i = 0; i < num_stages; ++i) { ms_per_stage[i] = 0.0; launches_per_stage[i] = 0; }
    std::lock_guard<std::mutex> lock(g_spans_mutex);
    for (const TimedSpan &sp : g_spans) {
        float ms = 0.f;
        NFFT_HIP_CHECK(hipEventSynchronize(sp.stop));
        NFFT_HIP_CHECK(hipEventElapsedTime(&ms, sp.start, sp.stop));
        if (sp.stage < num_stages) { ms_per_stage[sp.stage] += ms; launches_per_stage[sp.stage] += 1; }
        g_free_events.push_back(sp.start);
        g_free_events.push_back(sp.stop);
    }
    g_spans.clear();
    return 0;
}

int64_t nfft_hip_adjoint_workspace_bytes(const nfft_hip_problem *p, int x_is_complex, int real_output)
{
    (void)real_output;
    if (validate(p)) return -1;
    Route r;
    if (make_route(p, x_is_complex ? 2 : 1, kRouteAdjoint, r)) return -1;
    return r.total;
}

int64_t nfft_hip_forward_workspace_bytes(const nfft_hip_problem *p, int x_is_complex, int real_output)
{
    (void)x_is_complex;
    if (validate(p)) return -1;
    Route r;
    if (make_route(p, real_output ? 1 : 2, kRouteForward, r)) return -1;
    return r.total;
}

int64_t nfft_hip_plan_bytes(const nfft_hip_problem *p)
{
    if (validate(p)) return -1;
    return plan_route(p, 0).plan_bytes;
}

int nfft_hip_plan_points(const nfft_hip_problem *p, const float *pos, const int64_t *batch, void *plan,
                         int64_t plan_bytes, void *stream)
{
    if (int rc = take_pending_fault()) return rc;  // a kernel of an earlier call gave up: say so
    if (int rc = validate(p)) return rc;
    const Route r = plan_route(p, 0);
    if (!plan || plan_bytes < r.plan_bytes) { set_error("plan buffer too small"); return NFFT_HIP_EWORKSPACE; }
    if (p->num_points > 0 && !pos) { set_error("Input mismatch: pos is null"); return NFFT_HIP_EINVAL; }
    StageTimer t(kStagePlan, (hipStream_t)stream);
    return build_plans(r, pos, batch, plan, (hipStream_t)stream);
}

int nfft_hip_plan_verify(const nfft_hip_problem *p, const float *pos, const int64_t *batch, void *plan, void *stream)
{
    if (int rc = validate(p)) return rc;
    if (!plan || (p->num_points > 0 && !pos)) { set_error("Input mismatch: null plan or pos"); return NFFT_HIP_EINVAL; }
    static std::atomic<unsigned> slot{0};  // eight verifications of one plan may be in flight (on different streams)
    return launch_points_verify(pos, batch, p->num_points, p->dim, (char *)plan + plan_route(p, 0).L.off_seal,
                                (int)(slot++ & 7u), (hipStream_t)stream);
}

// Test entry (tests/test_gpu_graded_items.py; not part of the C ABI of include/nfft_hip.h, like nfft_dbg_eft): copies the
// work list of a plan of the wide tiling to the host.  which = 0: the plan of the gather (and of scatter spreading), 1: the
// plan the spreading kernel uses (the owned one if the problem has one).  info[8] = {entries written by the plan, 1 if the
// plan runs from the persistent launch, capacity of the list (work_cap), workgroups of the per-entry launch, pencils per
// point set, point sets, slabs per pencil, items of an average pencil}; set_hdr[2 * sets] = {entries, first entry} of every
// point set; entries[4 * min(capacity, max_entries)] = the list in launch order, rows {point set * pencils + pencil, first
// slab, end slab, points}.  All three are host buffers; the call waits for the stream.
int nfft_dbg_work_list(const nfft_hip_problem *p, const void *plan, int which, int64_t *info, int32_t *set_hdr, int32_t *entries,
                       int64_t max_entries, void *stream)
{
    if (int rc = validate(p)) return rc;
    const Route r = plan_route(p, 0);
    const Geom &g = which ? r.spread_geom() : r.g;
    const PlanLayout &L = which ? r.spread_layout() : r.L;
    if (!g.wide || !plan || !info || !set_hdr || !entries) { set_error("Input mismatch: no work list"); return NFFT_HIP_EINVAL; }
    const char *base = (const char *)(which ? r.spread_plan(plan) : plan) + L.off_work;
    hipStream_t s = (hipStream_t)stream;
    int32_t hdr[4];
    NFFT_HIP_CHECK(hipMemcpyAsync(hdr, base, 16, hipMemcpyDeviceToHost, s));
    NFFT_HIP_CHECK(hipMemcpyAsync(set_hdr, base + 16, (size_t)r.B * 8, hipMemcpyDeviceToHost, s));
    const int64_t rows = std::min<int64_t>(L.work_cap, max_entries);
    NFFT_HIP_CHECK(hipMemcpyAsync(entries, base + (L.work_head + L.work_cap) * 16, (size_t)rows * 16, hipMemcpyDeviceToHost, s));
    NFFT_HIP_CHECK(hipStreamSynchronize(s));
    const RangeSplit rs = range_split(g, L, r.n);
    info[0] = hdr[0];
    info[1] = hdr[2];
    info[2] = L.work_cap;
    info[3] = std::min<int64_t>(per_entry_workgroups(r.n, rs.nsets, rs.pencils, rs.runs, g.M, device_cu_count()), L.work_cap);
    info[4] = rs.pencils;
    info[5] = rs.nsets;
    info[6] = g.M;
    info[7] = rs.runs;
    return 0;
}

// Test entry (tests/test_route.py, tests/test_gpu_value_widths.py; not part of the C ABI either): the route plan_route gives
// a problem whose calls have `real_columns` real planes per point set.  out[8] = {g.wide, owned, spread_geom().pair, spread
// (SpreadMode), x_through_plan, gather (GatherKernel), g.CG, 1 if a call without a plan takes the one-kernel path of
// small_grid_route}.  Host code only: no launch, no device memory.
int nfft_dbg_route(const nfft_hip_problem *p, int64_t real_columns, int32_t *out)
{
    if (int rc = validate(p)) return rc;
    if (!out || real_columns < 0) { set_error("Input mismatch: no route"); return NFFT_HIP_EINVAL; }
    const Route r = plan_route(p, real_columns);
    out[0] = r.g.wide;
    out[1] = r.owned ? 1 : 0;
    out[2] = r.spread_geom().pair;
    out[3] = (int32_t)r.spread;
    out[4] = r.x_through_plan ? 1 : 0;
    out[5] = (int32_t)r.gather;
    out[6] = r.g.CG;
    out[7] = small_grid_route(p) ? 1 : 0;
    return 0;
}

// Test entry (tests/test_plan_ref.py, tests/test_gpu_plan_edges.py; not part of the C ABI either): geometry, layout and
// host decisions of the point plans plan_route gives a problem.  main[kPlanLayoutFields]: the plan at the start of the
// buffer; own[kPlanLayoutFields]: the owned plan behind it, filled when the route has one (main[39] = own[39] = 1).
// Fields: {dim, m, M, W, Ta[1], Ta[2], nta[1], nta[2], np0, bin0, SB, sb2, CG, wide, owned, pair, pstride,
// tiles_per_batch | ntiles, cap, l1bins, l1seg, npencils, block_points, nblocks, two_level, grouped, off_offsets,
// off_cursor, off_seal, off_perm, off_spos, off_groups (byte offsets from the plan's own start), off_own (start of this
// plan in the buffer) | one_level, local_scan, fuse, scan items, scan kind (kernels.h PlanDecisions) | has an owned plan}.
// Host code only: no launch, no device memory.
constexpr int kPlanLayoutFields = 40;
static void fill_plan_layout(const Geom &g, const PlanLayout &L, int64_t base, bool has_own, int64_t *o)
{
    const PlanDecisions d = plan_decisions(g, L);
    const int64_t v[kPlanLayoutFields] = {
        g.dim, g.m, g.M, g.W, g.Ta[1], g.Ta[2], g.nta[1], g.nta[2], g.np0, g.bin0, g.SB, g.sb2, g.CG, g.wide, g.owned, g.pair,
        g.pstride, g.tiles_per_batch,
        L.ntiles, L.cap, L.l1bins, L.l1seg, L.npencils, L.block_points, L.nblocks, L.two_level ? 1 : 0, L.grouped ? 1 : 0,
        L.off_offsets, L.off_cursor, L.off_seal, L.off_perm, L.off_spos, L.off_groups, base,
        d.one_level ? 1 : 0, d.local_scan ? 1 : 0, d.fuse ? 1 : 0, d.scan_items, d.scan_kind,
        has_own ? 1 : 0};
    for (int i = 0; i < kPlanLayoutFields; ++i) o[i] = v[i];
}
int nfft_dbg_plan_layout(const nfft_hip_problem *p, int64_t real_columns, int64_t *main, int64_t *own)
{
    if (int rc = validate(p)) return rc;
    if (!main || !own || real_columns < 0) { set_error("Input mismatch: no plan layout"); return NFFT_HIP_EINVAL; }
    const Route r = plan_route(p, real_columns);
    fill_plan_layout(r.g, r.L, 0, r.owned, main);
    for (int i = 0; i < kPlanLayoutFields; ++i) own[i] = 0;
    if (r.owned) fill_plan_layout(r.go, r.Lo, r.off_own, true, own);
    return 0;
}

// make_route as adjoint_impl / forward_impl call it (planes per column: of x for an adjoint, of y for a forward transform)
static int stage_route(const nfft_hip_problem *p, int adjoint, int x_is_complex, int real_output, Route &r, bool size_fft_work)
{
    if (adjoint) return make_route(p, x_is_complex ? 2 : 1, kRouteAdjoint, r, size_fft_work);
    return make_route(p, real_output ? 1 : 2, kRouteForward, r, size_fft_work);
}

// Test entry (tests/test_route.py, tests/test_gpu_fft_stage.py; not part of the C ABI either): what make_route decides for
// the FFT stage of an adjoint (adjoint != 0) or a forward transform, under the process's NFFT_HIP_CHUNK_BYTES and
// NFFT_HIP_NO_COLFFT, and what a chunk of `chunk_np` planes (<= 0: chunk_planes) runs.  out[11] = {fft (FftRoute), ci,
// chunk_planes, total_planes, chunk_fft(chunk_np), then {NC, 1 if col_dispatch takes a compile-time instantiation} of the
// adjoint's axis-1 pass, of its axis-0 pass and of the forward passes (colfft.hip colfft_tile_widths: the adjoint pairs
// are 0 for a forward route and the forward pair for an adjoint one, all are 0 on kFftFull)}.  Host code only: no launch,
// no device memory (make_route without rocFFT's work-area query).
int nfft_dbg_fft_route(const nfft_hip_problem *p, int adjoint, int x_is_complex, int real_output, int64_t chunk_np, int64_t *out)
{
    if (int rc = validate(p)) return rc;
    if (!out) { set_error("Input mismatch: no route"); return NFFT_HIP_EINVAL; }
    Route r;
    if (int rc = stage_route(p, adjoint, x_is_complex, real_output, r, false)) return rc;
    const int64_t np = chunk_np > 0 ? chunk_np : r.chunk_planes;
    const FftRoute route = r.chunk_fft(np);
    int32_t nc[6] = {0, 0, 0, 0, 0, 0};
    if (route != kFftFull) colfft_tile_widths(r.g, route == kFftOwnPlanar, route == kFftOwnCi, x_is_complex, np, nc);
    out[0] = (int64_t)r.fft;
    out[1] = r.ci ? 1 : 0;
    out[2] = r.chunk_planes;
    out[3] = r.total_planes;
    out[4] = (int64_t)route;
    for (int i = 0; i < 6; ++i) out[5 + i] = (i < 4) == (adjoint != 0) ? nc[i] : 0;
    return 0;
}

// Test entry (tests/test_gpu_fft_stage.py; not part of the C ABI either): the FFT stage alone, on the Route and through
// the chunk loop of adjoint_impl / forward_impl, with a copy between the caller's planes and the chunk's grids where
// those spread or gather.  adjoint != 0: planes [B * C * ppc, (2N)^d] real grids -> band = y [B, N^d, C] (mult / mult_kind
// as in the fastsum); else band = xhat [B, N^d, C] -> planes.  The workspace is that of nfft_hip_adjoint_workspace_bytes /
// nfft_hip_forward_workspace_bytes.  Never the one-kernel path of small_grid_route (tests/test_gpu_smallgrid.py).
int nfft_dbg_fft_stage(const nfft_hip_problem *p, int adjoint, int x_is_complex, int real_output, void *planes, void *band,
                       const void *mult, int mult_kind, void *workspace, int64_t workspace_bytes, void *stream)
{
    if (int rc = take_pending_fault()) return rc;
    if (int rc = validate(p)) return rc;
    hipStream_t s = (hipStream_t)stream;
    Route r;
    if (int rc = stage_route(p, adjoint, x_is_complex, real_output, r, true)) return rc;
    if (r.total_planes == 0) return 0;
    if (!planes || !band) { set_error("Input mismatch: null input"); return NFFT_HIP_EINVAL; }
    char *ws = workspace_base(workspace, workspace_bytes, r.total);
    if (!ws) return NFFT_HIP_EWORKSPACE;
    float *grid = (float *)(ws + r.off_grid);
    float2 *spec = (float2 *)(ws + r.off_spec);
    return for_chunks(r, [&](int64_t p0, int64_t np) -> int {
        float *mine = (float *)planes + p0 * r.g.cells;
        const size_t bytes = (size_t)(np * r.g.cells * 4);
        if (adjoint) {
            NFFT_HIP_CHECK(hipMemcpyAsync(grid, mine, bytes, hipMemcpyDeviceToDevice, s));
            return fft_adjoint_chunk(r, ws, grid, spec, x_is_complex, real_output, p0, np, band, mult, mult_kind, s);
        }
        if (int rc = fft_forward_chunk(r, ws, band, x_is_complex, real_output, p0, np, grid, spec, s)) return rc;
        NFFT_HIP_CHECK(hipMemcpyAsync(mine, grid, bytes, hipMemcpyDeviceToDevice, s));
        return 0;
    });
}

int64_t nfft_hip_spread_scratch_bytes(const nfft_hip_problem *p, int64_t real_columns)
{
    if (validate(p) || real_columns < 0) return -1;
    // plan-ordered copy of the coefficients + one word per plane (its largest |x|) + the work-list counters
    return (align_up(plan_route(p, real_columns).spread_layout().cap * real_columns, 64) + 64 +
            align_up(p->batch_size * real_columns, 64) + kTicketPlanes) * 4;
}

int nfft_hip_spread(const nfft_hip_problem *p, const void *plan, const float *xr, int64_t real_columns, float *grid,
                    float *scratch, void *stream)
{
    if (int rc = take_pending_fault()) return rc;  // a kernel of an earlier call gave up: say so
    if (int rc = validate(p)) return rc;
    const Route r = plan_route(p, real_columns);
    hipStream_t s = (hipStream_t)stream;
    const int64_t planes = r.B * real_columns;
    if (planes > 32768) { set_error("Input mismatch: too many planes for one spread call"); return NFFT_HIP_EINVAL; }
    unsigned *xmax = (unsigned *)(scratch + align_up(r.spread_layout().cap * real_columns, 64) + 64);
    int *tickets = (int *)(xmax + align_up(r.B * real_columns, 64));
    if (r.spread == kSpreadMfma)
        if (int rc = launch_plane_absmax(r.g, r.L, plan, xr, r.n, r.B, real_columns, xmax, s)) return rc;
    if (r.x_through_plan) return spread_chunk(r, plan, xr, scratch, xmax, 0, planes, grid, tickets, s);
    if (int rc = launch_gather_rows(r.spread_geom(), r.spread_layout(), r.spread_plan(plan), r.n, xr, real_columns, scratch, s))
        return rc;
    return spread_chunk(r, plan, nullptr, scratch, xmax, 0, planes, grid, tickets, s);
}

int nfft_hip_interpolate(const nfft_hip_problem *p, const void *plan, const float *grid, int64_t real_columns,
                         float *yr, void *stream)
{
    if (int rc = take_pending_fault()) return rc;  // a kernel of an earlier call gave up: say so
    if (int rc = validate(p)) return rc;
    const Route r = plan_route(p, real_columns);
    const int64_t planes = r.B * real_columns;
    if (planes > 32768) { set_error("Input mismatch: too many planes for one interpolate call"); return NFFT_HIP_EINVAL; }
    // (no workspace here: the persistent launches of unbalanced plans deal their work lists round robin)
    return gather_chunk(r, plan, grid, 0, planes, yr, nullptr, (hipStream_t)stream);
}

static int adjoint_impl(const nfft_hip_problem *p, const float *pos, const int64_t *batch, const void *ext_plan,
                        const void *x, int x_is_complex, int real_output, void *y, void *workspace,
                        int64_t workspace_bytes, void *stream, const void *mult = nullptr, int mult_kind = 0)
{
    if (int rc = take_pending_fault()) return rc;  // a kernel of an earlier call gave up: say so
    if (int rc = validate(p)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (!ext_plan && small_grid_route(p)) {
        // grid in one workgroup's LDS: one kernel, no plan, no workspace (smallgrid.hip)
        if (p->batch_size * p->num_columns == 0) return 0;
        if (!y) { set_error("Input mismatch: y is null"); return NFFT_HIP_EINVAL; }
        if (p->num_points > 0 && (!pos || !x)) { set_error("Input mismatch: null input"); return NFFT_HIP_EINVAL; }
        StageTimer t(kStageSpread, s);
        return launch_small_grid_adjoint(p, pos, batch, x, x_is_complex, real_output, y, mult, mult_kind, s);
    }
    Route r;
    if (int rc = make_route(p, x_is_complex ? 2 : 1, kRouteAdjoint, r)) return rc;
    if (r.total_planes == 0) return 0;
    if (!y) { set_error("Input mismatch: y is null"); return NFFT_HIP_EINVAL; }
    if (r.n > 0 && ((!pos && !ext_plan) || !x)) { set_error("Input mismatch: null input"); return NFFT_HIP_EINVAL; }
    char *ws = workspace_base(workspace, workspace_bytes, r.total);
    if (!ws) return NFFT_HIP_EWORKSPACE;
    const void *plan = ext_plan;
    float *xs = (float *)(ws + r.off_xs);
    unsigned *xmax = (unsigned *)(ws + r.off_xmax);
    float *grid = (float *)(ws + r.off_grid);
    float2 *spec = (float2 *)(ws + r.off_spec);
    int *tickets = (int *)(ws + r.off_tickets);

    if (!ext_plan) {
        StageTimer t(kStagePlan, s);
        if (int rc = build_plans(r, pos, batch, ws + r.off_plan, s)) return rc;
        plan = ws + r.off_plan;
    }
    if (r.spread == kSpreadMfma) {
        // operand scales of the matrix-core kernel: one streaming pass over x for all planes of the call
        StageTimer t(kStageGather, s);
        if (int rc = launch_plane_absmax(r.g, r.L, plan, (const float *)x, r.n, r.B, r.Cr, xmax, s)) return rc;
    }
    if (!r.x_through_plan) {
        StageTimer t(kStageGather, s);
        if (int rc = launch_gather_rows(r.spread_geom(), r.spread_layout(), r.spread_plan(plan), r.n, (const float *)x, r.Cr, xs, s))
            return rc;
    }
    return for_chunks(r, [&](int64_t p0, int64_t np) -> int {
        if (int rc = spread_chunk(r, plan, r.x_through_plan ? (const float *)x : nullptr, xs, xmax, p0, np, grid, tickets, s))
            return rc;
        return fft_adjoint_chunk(r, ws, grid, spec, x_is_complex, real_output, p0, np, y, mult, mult_kind, s);
    });
}

static int forward_impl(const nfft_hip_problem *p, const float *pos, const int64_t *batch, const void *ext_plan,
                        const void *xhat, int x_is_complex, int real_output, void *y, void *workspace,
                        int64_t workspace_bytes, void *stream)
{
    if (int rc = take_pending_fault()) return rc;  // a kernel of an earlier call gave up: say so
    if (int rc = validate(p)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (!ext_plan && small_grid_route(p)) {
        if (p->batch_size * p->num_columns == 0 || p->num_points == 0) return 0;
        if (!y || !pos || !xhat) { set_error("Input mismatch: null input"); return NFFT_HIP_EINVAL; }
        StageTimer t(kStageInterp, s);
        return launch_small_grid_forward(p, pos, batch, xhat, x_is_complex, real_output, y, s);
    }
    Route r;
    if (int rc = make_route(p, real_output ? 1 : 2, kRouteForward, r)) return rc;
    if (r.total_planes == 0 || r.n == 0) return 0;
    if (!y || (!pos && !ext_plan) || !xhat) { set_error("Input mismatch: null input"); return NFFT_HIP_EINVAL; }
    char *ws = workspace_base(workspace, workspace_bytes, r.total);
    if (!ws) return NFFT_HIP_EWORKSPACE;
    const void *plan = ext_plan;
    float *grid = (float *)(ws + r.off_grid);
    float2 *spec = (float2 *)(ws + r.off_spec);
    int *tickets = (int *)(ws + r.off_tickets);

    if (!ext_plan) {
        // (only the first sort: the forward transform never spreads)
        StageTimer t(kStagePlan, s);
        if (int rc = launch_plan_points(r.g, r.L, pos, batch, r.n, r.B, ws + r.off_plan, s)) return rc;
        plan = ws + r.off_plan;
    }
    return for_chunks(r, [&](int64_t p0, int64_t np) -> int {
        if (int rc = fft_forward_chunk(r, ws, xhat, x_is_complex, real_output, p0, np, grid, spec, s)) return rc;
        StageTimer t(kStageInterp, s);
        return gather_chunk(r, plan, grid, p0, np, (float *)y, tickets, s);
    });
}

int nfft_hip_adjoint(const nfft_hip_problem *p, const float *pos, const void *x, int x_is_complex,
                     const int64_t *batch, int real_output, void *y, void *workspace, int64_t workspace_bytes,
                     void *stream)
{
    return adjoint_impl(p, pos, batch, nullptr, x, x_is_complex, real_output, y, workspace, workspace_bytes, stream);
}

int nfft_hip_forward(const nfft_hip_problem *p, const float *pos, const void *xhat, int x_is_complex,
                     const int64_t *batch, int real_output, void *y, void *workspace, int64_t workspace_bytes,
                     void *stream)
{
    return forward_impl(p, pos, batch, nullptr, xhat, x_is_complex, real_output, y, workspace, workspace_bytes, stream);
}

int nfft_hip_plan_needed(const nfft_hip_problem *p)
{
    if (validate(p)) return 1;
    return small_grid_route(p) ? 0 : 1;
}

int nfft_hip_adjoint_planned(const nfft_hip_problem *p, const void *plan, const void *x, int x_is_complex,
                             int real_output, void *y, void *workspace, int64_t workspace_bytes, void *stream)
{
    if (!plan) { set_error("Input mismatch: plan is null"); return NFFT_HIP_EINVAL; }
    return adjoint_impl(p, nullptr, nullptr, plan, x, x_is_complex, real_output, y, workspace, workspace_bytes, stream);
}

int nfft_hip_forward_planned(const nfft_hip_problem *p, const void *plan, const void *xhat, int x_is_complex,
                             int real_output, void *y, void *workspace, int64_t workspace_bytes, void *stream)
{
    if (!plan) { set_error("Input mismatch: plan is null"); return NFFT_HIP_EINVAL; }
    return forward_impl(p, nullptr, nullptr, plan, xhat, x_is_complex, real_output, y, workspace, workspace_bytes, stream);
}

// ---- gradient with respect to the points ---------------------------------------------------------
namespace {
// Route of nfft_hip_forward_grad_points: the forward transform's, its workspace extended, with two or more real planes per
// point set, by the per-plane partial gradients [Cr, n, dim] that grad_reduce sums in plane order.
int forward_grad_route(const nfft_hip_problem *p, int real_output, Route &r)
{
    if (int rc = make_route(p, real_output ? 1 : 2, kRouteForward, r)) return rc;
    Carve c(r.end);
    r.off_part = c.take(r.Cr > 1 ? r.Cr * r.n * p->dim * 4 : 0);
    r.end = c.end();
    r.total = c.total();
    return 0;
}
} // namespace

int64_t nfft_hip_forward_grad_workspace_bytes(const nfft_hip_problem *p, int x_is_complex, int real_output)
{
    (void)x_is_complex;
    if (validate(p)) return -1;
    Route r;
    if (forward_grad_route(p, real_output, r)) return -1;
    return r.total;
}

namespace {
// The weighted gradient gather of a forward transform on its point plan; y non-null: the value-writing gather, which also
// stores the transform itself (nfft_hip_forward's layout).
int forward_grad_impl(const nfft_hip_problem *p, const void *plan, const void *xhat, int x_is_complex, int real_output,
                      const float *w, float *y, float *dpos, void *workspace, int64_t workspace_bytes, hipStream_t s)
{
    if (int rc = take_pending_fault()) return rc;  // a kernel of an earlier call gave up: say so
    if (int rc = validate(p)) return rc;
    if (p->num_points > 0 && p->num_columns > 0 && !workspace_base(workspace, workspace_bytes, grad_least_bytes(p, real_output)))
        return NFFT_HIP_EWORKSPACE;
    Route r;
    if (int rc = forward_grad_route(p, real_output, r)) return rc;
    if (r.n == 0) return 0;
    if (!dpos) { set_error("Input mismatch: dpos is null"); return NFFT_HIP_EINVAL; }
    if (r.total_planes == 0) {  // no columns: the transform is empty and so is its gradient
        NFFT_HIP_CHECK(hipMemsetAsync(dpos, 0, (size_t)(r.n * p->dim * 4), s));
        return 0;
    }
    if (!plan || !xhat || !w) { set_error("Input mismatch: null input"); return NFFT_HIP_EINVAL; }
    char *ws = workspace_base(workspace, workspace_bytes, r.total);
    if (!ws) return NFFT_HIP_EWORKSPACE;
    float *grid = (float *)(ws + r.off_grid);
    float2 *spec = (float2 *)(ws + r.off_spec);
    float *part = r.Cr > 1 ? (float *)(ws + r.off_part) : dpos;  // one plane per set: the kernel writes dpos itself
    const int rc = for_chunks(r, [&](int64_t p0, int64_t np) -> int {
        if (int rc = fft_forward_chunk(r, ws, xhat, x_is_complex, real_output, p0, np, grid, spec, s)) return rc;
        StageTimer t(kStageInterp, s);
        if (y) return launch_interp_value_grad(r.g, r.L, plan, grid, r.n, r.Cr, p0, np, w, part, y, s);
        return launch_interp_grad(r.g, r.L, plan, grid, r.n, r.Cr, p0, np, w, part, s);
    });
    if (rc || r.Cr < 2) return rc;
    return launch_grad_reduce(part, r.n * p->dim, r.Cr, dpos, s);
}
} // namespace

int nfft_hip_forward_grad_points_planned(const nfft_hip_problem *p, const void *plan, const void *xhat, int x_is_complex,
                                         int real_output, const float *w, float *dpos, void *workspace,
                                         int64_t workspace_bytes, void *stream)
{
    return forward_grad_impl(p, plan, xhat, x_is_complex, real_output, w, nullptr, dpos, workspace, workspace_bytes,
                             (hipStream_t)stream);
}

int nfft_hip_forward_value_grad_points_planned(const nfft_hip_problem *p, const void *plan, const void *xhat,
                                               int x_is_complex, int real_output, const float *w, void *y, float *dpos,
                                               void *workspace, int64_t workspace_bytes, void *stream)
{
    if (!y && p && p->num_points > 0 && p->num_columns > 0) { set_error("Input mismatch: y is null"); return NFFT_HIP_EINVAL; }
    return forward_grad_impl(p, plan, xhat, x_is_complex, real_output, w, (float *)y, dpos, workspace, workspace_bytes,
                             (hipStream_t)stream);
}

// ---- backward of the point gradient: second derivatives -------------------------------------
namespace {
// Workspace: the gradient gather's (forward route + partial sums) for dw / dpos, then, reusing the same bytes, for dxhat
// an adjoint of the same problem (u = omega v_a as its input: complex unless real_output) + u [n, Cr] + its output
// [B, N^dim, C] complex.
struct HvpCarve {
    Route grad, adj;
    int64_t off_u, off_y, total;
};
int hvp_carve(const nfft_hip_problem *p, int real_output, HvpCarve &h)
{
    if (int rc = forward_grad_route(p, real_output, h.grad)) return rc;
    if (int rc = make_route(p, real_output ? 1 : 2, kRouteAdjoint, h.adj)) return rc;
    Carve c(h.adj.total);
    h.off_u = c.take(p->num_points * h.adj.Cr * 4);
    h.off_y = c.take(band_size_of(p));
    h.total = std::max(h.grad.total, c.total());
    return 0;
}
} // namespace

int64_t nfft_hip_forward_grad_points_backward_workspace_bytes(const nfft_hip_problem *p, int x_is_complex, int real_output)
{
    (void)x_is_complex;
    if (validate(p)) return -1;
    HvpCarve h;
    if (hvp_carve(p, real_output, h)) return -1;
    return h.total;
}

int nfft_hip_forward_grad_points_backward_planned(const nfft_hip_problem *p, const void *plan, const void *xhat,
                                                  int x_is_complex, int real_output, const float *w, const float *v,
                                                  void *dxhat, float *dw, float *dpos, void *workspace,
                                                  int64_t workspace_bytes, void *stream)
{
    if (int rc = take_pending_fault()) return rc;  // a kernel of an earlier call gave up: say so
    if (int rc = validate(p)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (!dxhat && !dw && !dpos) return 0;
    const int64_t n = p->num_points, C = p->num_columns, Cr = C * (real_output ? 1 : 2);
    if (n == 0 || C == 0) {  // no points or no columns: G is empty or identically zero, and so is every derivative of it
        if (dxhat) NFFT_HIP_CHECK(hipMemsetAsync(dxhat, 0, (size_t)(band_size_of(p) / (x_is_complex ? 1 : 2)), s));
        if (dpos) NFFT_HIP_CHECK(hipMemsetAsync(dpos, 0, (size_t)(n * p->dim * 4), s));
        return 0;  // (dw has n * Cr = 0 elements)
    }
    if (!plan || !xhat || !v || ((dpos || dxhat) && !w)) { set_error("Input mismatch: null input"); return NFFT_HIP_EINVAL; }
    if (!workspace_base(workspace, workspace_bytes, grad_least_bytes(p, real_output))) return NFFT_HIP_EWORKSPACE;
    HvpCarve h;
    if (int rc = hvp_carve(p, real_output, h)) return rc;
    char *ws = workspace_base(workspace, workspace_bytes, h.total);
    if (!ws) return NFFT_HIP_EWORKSPACE;
    if (dw || dpos) {
        // the moment gather on the forward transform's grid, chunk by chunk as the gradient gather runs
        const Route &r = h.grad;
        float *grid = (float *)(ws + r.off_grid);
        float2 *spec_buf = (float2 *)(ws + r.off_spec);
        float *part = !dpos ? nullptr : r.Cr > 1 ? (float *)(ws + r.off_part) : dpos;
        if (int rc = for_chunks(r, [&](int64_t p0, int64_t np) -> int {
                if (int rc = fft_forward_chunk(r, ws, xhat, x_is_complex, real_output, p0, np, grid, spec_buf, s)) return rc;
                StageTimer t(kStageInterp, s);
                return launch_interp_hvp(r.g, r.L, plan, grid, n, r.Cr, p0, np, w, v, dw, part, s);
            }))
            return rc;
        if (dpos && r.Cr > 1)
            if (int rc = launch_grad_reduce(part, n * p->dim, r.Cr, dpos, s)) return rc;
    }
    if (dxhat) {
        const Route &ra = h.adj;
        if (hvp_fused_dxhat(ra)) {
            // the derivative spreading of w, then the adjoint's own FFT stage and roll-off, chunk by chunk
            float *grid = (float *)(ws + ra.off_grid);
            float2 *spec_buf = (float2 *)(ws + ra.off_spec);
            return for_chunks(ra, [&](int64_t p0, int64_t np) -> int {
                { StageTimer t(kStageZero, s); NFFT_HIP_CHECK(hipMemsetAsync(grid, 0, (size_t)(np * ra.g.cells * 4), s)); }
                {
                    StageTimer t(kStageSpread, s);
                    if (int rc = launch_spread_deriv(ra.g, ra.L, plan, w, v, n, ra.Cr, p0, np, grid, s)) return rc;
                }
                return fft_adjoint_chunk(ra, ws, grid, spec_buf, real_output ? 0 : 1, x_is_complex ? 0 : 1, p0, np, dxhat,
                                         nullptr, 0, s);
            });
        }
        // sum_a 2 pi i k_a adjoint(omega v_a), axes in order (hvp_spectral.hip)
        float *u = (float *)(ws + h.off_u);
        void *y = ws + h.off_y;
        for (int a = 0; a < p->dim; ++a) {
            if (int rc = launch_hvp_stage(w, v, n, Cr, p->dim, a, u, s)) return rc;
            if (int rc = adjoint_impl(p, nullptr, nullptr, plan, u, real_output ? 0 : 1, 0, y, ws, ra.total, stream)) return rc;
            if (int rc = launch_hvp_combine(y, p->batch_size, p->N, p->dim, C, a, a > 0, x_is_complex, dxhat, s)) return rc;
        }
    }
    return 0;
}

// ---- fast summation -------------------------------------------------------------------------
namespace {
struct FastsumCarve {
    Route src, tgt;  // adjoint at the sources, forward transform at the targets
    int64_t band_size, inner, off_band, off_plan_s, off_plan_t, off_inner, total;
};
int fastsum_check(const nfft_hip_problem *src, const nfft_hip_problem *tgt)
{
    if (int rc = validate(src)) return rc;
    if (int rc = validate(tgt)) return rc;
    if (src->dim != tgt->dim || src->N != tgt->N || src->m != tgt->m || src->batch_size != tgt->batch_size ||
        src->num_columns != tgt->num_columns) {
        set_error("Input mismatch: sources and targets disagree in dim / N / m / batch size / columns");
        return NFFT_HIP_EINVAL;
    }
    return 0;
}
int fastsum_carve(const nfft_hip_problem *src, const nfft_hip_problem *tgt, int x_is_complex, bool own_plans,
                  bool shared_points, FastsumCarve &f)
{
    if (int rc = make_route(src, x_is_complex ? 2 : 1, kRouteAdjoint, f.src)) return rc;
    if (int rc = make_route(tgt, x_is_complex ? 2 : 1, kRouteForward, f.tgt)) return rc;
    f.band_size = band_size_of(src);
    f.inner = std::max(f.src.total, f.tgt.total);
    Carve c;
    f.off_band = c.take(f.band_size);
    f.off_plan_s = c.take(own_plans ? f.src.plan_bytes : 0);
    f.off_plan_t = c.take(own_plans && !shared_points ? f.tgt.plan_bytes : 0);
    f.off_inner = c.take(f.inner);
    f.total = c.total();
    return 0;
}
int fastsum_impl(const nfft_hip_problem *src_in, const float *sources, const int64_t *source_batch,
                 const void *source_plan, const nfft_hip_problem *tgt_in, const float *targets,
                 const int64_t *target_batch, const void *target_plan, const void *x, int x_is_complex,
                 const void *coeffs, int coeffs_are_complex, void *y, void *workspace, int64_t workspace_bytes,
                 void *stream, void *band_out = nullptr)
{
    if (!src_in || !tgt_in) { set_error("Input mismatch: null problem"); return NFFT_HIP_EINVAL; }
    // fastsum geometry: every point within radius 1/4 (the kernel is only defined there)
    nfft_hip_problem src_q, tgt_q;
    quarter_ball(src_in, src_q);
    quarter_ball(tgt_in, tgt_q);
    const nfft_hip_problem *src = &src_q, *tgt = &tgt_q;
    if (int rc = fastsum_check(src, tgt)) return rc;
    const bool own_plans = source_plan == nullptr;
    const bool shared = own_plans ? (sources == targets && source_batch == target_batch && src->num_points == tgt->num_points)
                                  : (source_plan == target_plan);
    FastsumCarve f;
    if (int rc = fastsum_carve(src, tgt, x_is_complex, own_plans, shared, f)) return rc;
    if (tgt->num_points == 0 || src->num_columns == 0) return 0;
    if (!coeffs || !y) { set_error("Input mismatch: null input"); return NFFT_HIP_EINVAL; }
    char *ws = workspace_base(workspace, workspace_bytes, f.total);
    if (!ws) return NFFT_HIP_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    // problems whose grid fits one workgroup's LDS: adjoint (with the kernel's coefficients folded into its roll-off)
    // and forward transform are one fused kernel each on the caller's points -- no plans (smallgrid.hip)
    const bool fused1d = own_plans && small_grid_route(src) && small_grid_route(tgt);
    if (own_plans) {
        if (src->num_points > 0 && !sources) { set_error("Input mismatch: sources is null"); return NFFT_HIP_EINVAL; }
        if (!targets) { set_error("Input mismatch: targets is null"); return NFFT_HIP_EINVAL; }
    }
    if (own_plans && !fused1d) {
        {
            StageTimer t(kStagePlan, s);
            if (int rc = build_plans(f.src, sources, source_batch, ws + f.off_plan_s, s)) return rc;
        }
        source_plan = ws + f.off_plan_s;
        target_plan = source_plan;
        if (!shared) {
            StageTimer t(kStagePlan, s);
            if (int rc = build_plans(f.tgt, targets, target_batch, ws + f.off_plan_t, s)) return rc;
            target_plan = ws + f.off_plan_t;
        }
        sources = targets = nullptr;  // (the transforms run on the plans)
        source_batch = target_batch = nullptr;
    }
    // (the fused kernels run on the caller's points and need no workspace)
    void *inner = fused1d ? nullptr : ws + f.off_inner;
    const int64_t inner_bytes = fused1d ? 0 : f.inner;
    // (band_out: the caller keeps the band spectrum, the carve's band is not used)
    void *band = band_out ? band_out : ws + f.off_band;
    if (src->num_points == 0) {
        NFFT_HIP_CHECK(hipMemsetAsync(band, 0, (size_t)f.band_size, s));
    } else {
        // adjoint of the sources; the kernel's Fourier coefficients are multiplied in by the last spectral pass
        if (int rc = adjoint_impl(src, sources, source_batch, source_plan, x, x_is_complex, 0, band, inner, inner_bytes, stream,
                                  coeffs, coeffs_are_complex ? 2 : 1)) return rc;
    }
    // forward transform at the targets; real coefficients give a real result (core_cuda.cu:817-821)
    return forward_impl(tgt, targets, target_batch, target_plan, band, 1, x_is_complex ? 0 : 1, y, inner, inner_bytes, stream);
}
} // namespace

int64_t nfft_hip_fastsum_workspace_bytes(const nfft_hip_problem *src, const nfft_hip_problem *tgt, int x_is_complex,
                                         int shared_points, int planned)
{
    if (!src || !tgt) return -1;
    nfft_hip_problem s, t;
    quarter_ball(src, s);
    quarter_ball(tgt, t);
    if (fastsum_check(&s, &t)) return -1;
    FastsumCarve f;
    if (fastsum_carve(&s, &t, x_is_complex, planned == 0, shared_points != 0, f)) return -1;
    return f.total;
}

int nfft_hip_fastsum(const nfft_hip_problem *src, const float *sources, const int64_t *source_batch,
                     const nfft_hip_problem *tgt, const float *targets, const int64_t *target_batch, const void *x,
                     int x_is_complex, const void *coeffs, int coeffs_are_complex, void *y, void *workspace,
                     int64_t workspace_bytes, void *stream)
{
    return fastsum_impl(src, sources, source_batch, nullptr, tgt, targets, target_batch, nullptr, x, x_is_complex, coeffs,
                        coeffs_are_complex, y, workspace, workspace_bytes, stream);
}

int nfft_hip_fastsum_planned(const nfft_hip_problem *src, const void *source_plan, const nfft_hip_problem *tgt,
                             const void *target_plan, const void *x, int x_is_complex, const void *coeffs,
                             int coeffs_are_complex, void *y, void *workspace, int64_t workspace_bytes, void *stream)
{
    if (!source_plan || !target_plan) { set_error("Input mismatch: plan is null"); return NFFT_HIP_EINVAL; }
    return fastsum_impl(src, nullptr, nullptr, source_plan, tgt, nullptr, nullptr, target_plan, x, x_is_complex, coeffs,
                        coeffs_are_complex, y, workspace, workspace_bytes, stream);
}

int nfft_hip_fastsum_band(const nfft_hip_problem *src, const float *sources, const int64_t *source_batch,
                          const nfft_hip_problem *tgt, const float *targets, const int64_t *target_batch, const void *x,
                          int x_is_complex, const void *coeffs, int coeffs_are_complex, void *y, void *band,
                          void *workspace, int64_t workspace_bytes, void *stream)
{
    if (!band) { set_error("Input mismatch: band is null"); return NFFT_HIP_EINVAL; }
    return fastsum_impl(src, sources, source_batch, nullptr, tgt, targets, target_batch, nullptr, x, x_is_complex, coeffs,
                        coeffs_are_complex, y, workspace, workspace_bytes, stream, band);
}

int nfft_hip_fastsum_band_planned(const nfft_hip_problem *src, const void *source_plan, const nfft_hip_problem *tgt,
                                  const void *target_plan, const void *x, int x_is_complex, const void *coeffs,
                                  int coeffs_are_complex, void *y, void *band, void *workspace, int64_t workspace_bytes,
                                  void *stream)
{
    if (!source_plan || !target_plan) { set_error("Input mismatch: plan is null"); return NFFT_HIP_EINVAL; }
    if (!band) { set_error("Input mismatch: band is null"); return NFFT_HIP_EINVAL; }
    return fastsum_impl(src, nullptr, nullptr, source_plan, tgt, nullptr, nullptr, target_plan, x, x_is_complex, coeffs,
                        coeffs_are_complex, y, workspace, workspace_bytes, stream, band);
}

} // extern "C"

// ---- gradient of the fast summation with respect to its points ---------------------------------
namespace {
// Workspace of the fastsum backward: the grid H of the sources' gather (a band spectrum) and one area that the adjoint at
// the targets and the two gradient gathers use in turn.
struct FastsumGradCarve {
    int64_t band_size, off_h, off_inner, inner, total;
};
int fastsum_grad_carve(const nfft_hip_problem *src, const nfft_hip_problem *tgt, int x_is_complex, FastsumGradCarve &f)
{
    Route adj;
    if (int rc = make_route(tgt, x_is_complex ? 2 : 1, kRouteAdjoint, adj)) return rc;
    f.inner = adj.total;
    for (const nfft_hip_problem *p : {src, tgt}) {
        Route r;
        if (int rc = forward_grad_route(p, x_is_complex ? 0 : 1, r)) return rc;
        f.inner = std::max(f.inner, r.total);
    }
    f.band_size = band_size_of(src);
    Carve c;
    f.off_h = c.take(f.band_size);
    f.off_inner = c.take(f.inner);
    f.total = c.total();
    return 0;
}
} // namespace

extern "C" {

int64_t nfft_hip_fastsum_grad_workspace_bytes(const nfft_hip_problem *src, const nfft_hip_problem *tgt, int x_is_complex)
{
    if (!src || !tgt) return -1;
    nfft_hip_problem s, t;
    quarter_ball(src, s);
    quarter_ball(tgt, t);
    if (fastsum_check(&s, &t)) return -1;
    FastsumGradCarve f;
    if (fastsum_grad_carve(&s, &t, x_is_complex, f)) return -1;
    return f.total;
}

int nfft_hip_fastsum_backward_planned(const nfft_hip_problem *src_in, const void *source_plan,
                                      const nfft_hip_problem *tgt_in, const void *target_plan, const void *x,
                                      int x_is_complex, const void *dy, const void *coeffs, int coeffs_are_complex,
                                      const void *band, void *dx, float *dsources, float *dtargets, void *workspace,
                                      int64_t workspace_bytes, void *stream)
{
    if (int rc = take_pending_fault()) return rc;  // a kernel of an earlier call gave up: say so
    if (!src_in || !tgt_in) { set_error("Input mismatch: null problem"); return NFFT_HIP_EINVAL; }
    // the problems of the forward pass (fastsum_impl), so that its cached plans are the ones used
    nfft_hip_problem src_q, tgt_q;
    quarter_ball(src_in, src_q);
    quarter_ball(tgt_in, tgt_q);
    const nfft_hip_problem *src = &src_q, *tgt = &tgt_q;
    if (int rc = fastsum_check(src, tgt)) return rc;
    if (!source_plan || !target_plan) { set_error("Input mismatch: plan is null"); return NFFT_HIP_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    const int64_t ns = src->num_points, nt = tgt->num_points, C = src->num_columns;
    const int real_output = x_is_complex ? 0 : 1;  // as the forward pass: a real x gives a real y
    const bool sources_side = (dsources || dx) && ns > 0;
    const bool targets_side = dtargets && nt > 0;
    const bool work = C > 0 && ns > 0 && nt > 0 && (sources_side || targets_side);
    if (work) {
        // refused before any route makes its rocFFT plans: the grid H plus one grid plane per real plane of a column
        const int64_t least = align_up(band_size_of(src), 256) + problem_geom(src).cells * 4 * (x_is_complex ? 2 : 1);
        if (!workspace_base(workspace, workspace_bytes, least)) return NFFT_HIP_EWORKSPACE;
    }
    // nothing to gather (no columns, or one side empty: the sum and every gradient of it are zero)
    if (!work) {
        if (dsources && ns > 0) NFFT_HIP_CHECK(hipMemsetAsync(dsources, 0, (size_t)(ns * src->dim * 4), s));
        if (dx && ns > 0 && C > 0) NFFT_HIP_CHECK(hipMemsetAsync(dx, 0, (size_t)(ns * C * (x_is_complex ? 8 : 4)), s));
        if (dtargets && nt > 0) NFFT_HIP_CHECK(hipMemsetAsync(dtargets, 0, (size_t)(nt * tgt->dim * 4), s));
        return 0;
    }
    if (!dy || (sources_side && !coeffs) || (dsources && !x) || (targets_side && !band)) {
        set_error("Input mismatch: null input");
        return NFFT_HIP_EINVAL;
    }
    FastsumGradCarve f;
    if (int rc = fastsum_grad_carve(src, tgt, x_is_complex, f)) return rc;
    char *ws = workspace_base(workspace, workspace_bytes, f.total);
    if (!ws) return NFFT_HIP_EWORKSPACE;
    void *inner = ws + f.off_inner;
    if (sources_side) {
        // H = coeffs * A_t(dy): the adjoint at the targets with the coefficients folded into its roll-off, as fastsum_impl
        // does at the sources; then ONE forward FFT stage at the sources and one gather: dsources weighted by x, and with
        // dx its value -- the swapped fastsum when coeffs is the forward's (real) array
        void *h = ws + f.off_h;
        if (int rc = adjoint_impl(tgt, nullptr, nullptr, target_plan, dy, x_is_complex, 0, h, inner, f.inner, stream,
                                  coeffs, coeffs_are_complex ? 2 : 1)) return rc;
        if (dsources) {
            if (int rc = forward_grad_impl(src, source_plan, h, 1, real_output, (const float *)x, (float *)dx, dsources,
                                           inner, f.inner, s)) return rc;
        } else {
            if (int rc = forward_impl(src, nullptr, nullptr, source_plan, h, 1, real_output, dx, inner, f.inner, stream))
                return rc;
        }
    }
    if (targets_side) {
        // y = forward_t(band): the gradient gather of the saved band at the targets, weighted by dy
        if (int rc = forward_grad_impl(tgt, target_plan, band, 1, real_output, (const float *)dy, nullptr, dtargets, inner,
                                       f.inner, s)) return rc;
    }
    return 0;
}

} // extern "C"

// ---- Toeplitz normal operator A^H W A ------------------------------------------------------------
namespace {
// Workspace of the kernel-grid set-up: the half spectrum of K for all point sets + rocFFT's work area.
struct ToeplitzKernelCarve {
    Geom g;
    int64_t off_spec, off_work, work_bytes, total;
};
int toeplitz_kernel_carve(const nfft_hip_problem *p, ToeplitzKernelCarve &c)
{
    c.g = make_geom(p->dim, p->N, p->m);
    c.work_bytes = fft_work_bytes(kC2R, c.g.dim, c.g.M, p->batch_size);
    if (c.work_bytes < 0) return NFFT_HIP_EFFT;
    Carve carve;
    c.off_spec = carve.take(p->batch_size * half_cells_of(c.g) * 8);
    c.off_work = carve.take(c.work_bytes);
    c.total = carve.total();
    return 0;
}
bool aligned16(const void *ptr) { return ((uintptr_t)ptr & 15u) == 0; }
} // namespace

extern "C" {

int64_t nfft_hip_toeplitz_kernel_workspace_bytes(const nfft_hip_problem *p)
{
    if (validate(p)) return -1;
    ToeplitzKernelCarve c;
    if (toeplitz_kernel_carve(p, c)) return -1;
    return c.total;
}

int nfft_hip_toeplitz_kernel(const nfft_hip_problem *p, const void *t, float *K, void *workspace, int64_t workspace_bytes,
                             void *stream)
{
    if (int rc = take_pending_fault()) return rc;  // a kernel of an earlier call gave up: say so
    if (int rc = validate(p)) return rc;
    if (!t || !K) { set_error("Input mismatch: null input"); return NFFT_HIP_EINVAL; }
    ToeplitzKernelCarve c;
    if (int rc = toeplitz_kernel_carve(p, c)) return rc;
    char *ws = workspace_base(workspace, workspace_bytes, c.total);
    if (!ws) return NFFT_HIP_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    float2 *spec = (float2 *)(ws + c.off_spec);
    if (int rc = launch_toeplitz_spectrum(c.g, (const float2 *)t, p->batch_size, spec, s)) return rc;
    StageTimer tm(kStageFft, s);
    return fft_execute(kC2R, c.g.dim, c.g.M, p->batch_size, spec, K, ws + c.off_work, c.work_bytes, s);
}

int64_t nfft_hip_toeplitz_workspace_bytes(const nfft_hip_problem *p)
{
    if (validate(p)) return -1;
    Route r;
    if (make_route(p, 2, kRouteToeplitz, r)) return -1;
    return r.total;
}

int nfft_hip_toeplitz_apply(const nfft_hip_problem *p, const float *K, const void *xhat, int x_is_complex, void *y,
                            void *workspace, int64_t workspace_bytes, void *stream)
{
    if (int rc = take_pending_fault()) return rc;  // a kernel of an earlier call gave up: say so
    if (int rc = validate(p)) return rc;
    if (p->num_columns == 0) return 0;
    if (!K || !xhat || !y) { set_error("Input mismatch: null input"); return NFFT_HIP_EINVAL; }
    if (!aligned16(K)) { set_error("Input mismatch: the kernel grid must be 16-byte aligned"); return NFFT_HIP_EINVAL; }
    // the grid of x is complex whether x is or not: two real planes per column through both FFT stages
    Route r;
    if (int rc = make_route(p, 2, kRouteToeplitz, r)) return rc;
    char *ws = workspace_base(workspace, workspace_bytes, r.total);
    if (!ws) return NFFT_HIP_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    float *grid = (float *)(ws + r.off_grid);
    float2 *spec = (float2 *)(ws + r.off_spec);
    return for_chunks(r, [&](int64_t p0, int64_t np) -> int {
        if (r.toeplitz_fused) return toeplitz_fused_chunk(r, ws, xhat, x_is_complex, K, p0, np, spec, y, s);
        if (int rc = fft_forward_chunk(r, ws, xhat, x_is_complex, 0, p0, np, grid, spec, s)) return rc;
        {
            StageTimer t(kStageMultiply, s);
            if (int rc = launch_toeplitz_multiply(r.g, grid, K, r.Cr, p0, np, s)) return rc;
        }
        return fft_adjoint_chunk(r, ws, grid, spec, 1, 0, p0, np, y, nullptr, 0, s);
    });
}

} // extern "C"
