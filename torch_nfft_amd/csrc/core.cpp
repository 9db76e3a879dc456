// core.so -- the native operator registry of the package: the eight torch_nfft::* operators of the reference
// (csrc/core.cpp:43-121, 176-184; prototypes csrc/core.h:6-65), registered from C++ and loaded by the package's
// __init__ with torch.ops.load_library exactly like the reference's core.so (torch_nfft/__init__.py:11).
//
// This file is host glue only: input checks and error texts of the reference's validators
// (csrc/cuda/core_cuda.cu:38-137), output allocation from torch's caching allocator, the one blocking read of
// batch[-1] (core_cuda.cu:60), the point-plan cache, and the call into the C ABI of include/nfft_hip.h
// (libnfft_hip.so), which does all the arithmetic on torch's current stream.  There is no CPU path.
#include <ATen/ATen.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <c10/core/DeviceGuard.h>
#include <hip/hip_runtime_api.h>
#include <torch/library.h>

#include <mutex>
#include <tuple>
#include <vector>

#include "../../include/nfft_hip.h"

namespace {

#define CHECK_INPUT(cond) TORCH_CHECK((cond), "Input mismatch")  // csrc/cuda/cuda_utils.cu:3

void check_rc(int rc)
{
    if (rc == NFFT_HIP_OK) return;
    std::string msg = nfft_hip_last_error();
    if (rc == NFFT_HIP_EINVAL && msg.rfind("Input mismatch", 0) != 0) msg = "Input mismatch: " + msg;
    TORCH_CHECK(false, msg);
}

void *stream_of(const at::Tensor &t)
{
    return (void *)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.device().index()).stream();
}

at::Tensor byte_buffer(int64_t nbytes, const at::Tensor &like)
{
    return at::empty({nbytes}, like.options().dtype(at::kByte));
}

struct Points {
    int dim;
    int64_t n, B;
    at::Tensor pos, batch;  // contiguous; batch undefined when the caller passed None
};

// ---- ends of the batch vector -------------------------------------------------------------------------------
// B = batch[-1] + 1 needs a blocking read-back (as in the reference, core_cuda.cu:60): ~35 us per operator call -- more
// than a small transform takes, and paid again by the forward transform, the backward pass and the next step on the very
// same vector.  The two ends of the last few batch vectors are remembered by tensor identity + version counter: the same
// rules, the same limitation (writes that bypass the version counter) and the same switches as the point-plan cache
// below (ops.plan_cache_enabled / plan_cache_clear).  Inference tensors carry no version counter: always read back.
struct BatchEnds {
    const void *ptr = nullptr;
    int64_t version = -1, n = -1, first = 0, last = 0;
    int device = -1;
    // The entry belongs to ONE tensor object, held weakly: it neither pins the vector's memory (80 MB at 10^7 points, four
    // entries) nor survives the tensor -- an address the allocator hands to another tensor is a miss, not a stale hit.
    c10::weak_intrusive_ptr<c10::TensorImpl> owner{c10::intrusive_ptr<c10::TensorImpl>()};
    uint64_t last_use = 0;
    bool owned_by(const at::Tensor &t) const
    {
        const auto alive = owner.lock();
        return alive && alive.get() == t.unsafeGetTensorImpl();
    }
};
struct BatchEndsCache {
    std::mutex mutex;
    BatchEnds entries[4];
    bool enabled = true;
    uint64_t tick = 0;
    void clear() { for (BatchEnds &e : entries) e = BatchEnds(); }
};
BatchEndsCache &g_ends = *new BatchEndsCache;  // (never destroyed: see the plan cache)

void batch_ends(const at::Tensor &batch, int64_t n, int64_t &first, int64_t &last)
{
    const bool cacheable = !batch.is_inference();
    const void *ptr = batch.data_ptr();
    const int device = batch.device().index();
    int64_t version = -1;
    if (cacheable) {
        std::lock_guard<std::mutex> lock(g_ends.mutex);
        if (g_ends.enabled) {
            version = (int64_t)batch._version();
            for (BatchEnds &e : g_ends.entries) {
                if (e.ptr == ptr && e.version == version && e.n == n && e.device == device && e.owned_by(batch)) {
                    e.last_use = ++g_ends.tick;
                    first = e.first;
                    last = e.last;
                    return;
                }
            }
        }
    }
    const at::Tensor ends = at::stack({batch[0], batch[n - 1]}).cpu();
    first = ends[0].item<int64_t>();
    last = ends[1].item<int64_t>();
    if (cacheable && version >= 0) {
        std::lock_guard<std::mutex> lock(g_ends.mutex);
        if (!g_ends.enabled) return;
        BatchEnds *slot = &g_ends.entries[0];
        for (BatchEnds &e : g_ends.entries)
            if (e.last_use < slot->last_use) slot = &e;
        slot->ptr = ptr; slot->version = version; slot->n = n; slot->device = device;
        slot->first = first; slot->last = last; slot->last_use = ++g_ends.tick;
        slot->owner = c10::weak_intrusive_ptr<c10::TensorImpl>(batch.getIntrusivePtr());
    }
}

// check_point_input (core_cuda.cu:38-66).  One blocking read-back, as in the reference (:60) -- it also fetches
// batch[0], so that a negative first entry of the (sorted) batch vector is rejected instead of being clamped -- unless
// the ends of this very vector are remembered (batch_ends above).
Points check_points(const at::Tensor &pos, const c10::optional<at::Tensor> &opt_batch, const char *batch_name)
{
    TORCH_CHECK(pos.is_cuda(), "pos must be CUDA tensor");
    CHECK_INPUT(pos.dim() == 2);
    CHECK_INPUT(pos.scalar_type() == at::kFloat);
    Points p;
    p.n = pos.size(0);
    p.dim = (int)pos.size(1);
    CHECK_INPUT(p.dim >= 1 && p.dim <= 3);
    p.pos = pos.contiguous();
    p.B = 1;
    if (opt_batch.has_value() && opt_batch->defined()) {
        const at::Tensor &batch = *opt_batch;
        TORCH_CHECK(batch.is_cuda(), batch_name, " must be CUDA tensor");
        CHECK_INPUT(batch.dim() == 1);
        CHECK_INPUT(batch.scalar_type() == at::kLong);
        CHECK_INPUT(batch.numel() == p.n);
        CHECK_INPUT(batch.device() == pos.device());
        p.batch = batch.contiguous();
        if (p.n > 0) {
            int64_t first = 0, last = 0;
            batch_ends(p.batch, p.n, first, last);
            CHECK_INPUT(first >= 0 && last >= first);
            p.B = last + 1;
        }
    }
    return p;
}

bool real_dtype(const at::Tensor &t)
{
    if (t.scalar_type() == at::kFloat) return true;
    CHECK_INPUT(t.scalar_type() == at::kComplexFloat);
    return false;
}

nfft_hip_problem problem(const Points &p, int64_t C, int64_t N, int64_t m, int32_t flags = 0)
{
    nfft_hip_problem q;
    q.dim = p.dim;
    q.flags = flags;
    q.num_points = p.n;
    q.num_columns = C;
    q.batch_size = p.B;
    q.N = N;
    q.m = m;
    return q;
}

// The workspace of a native call from its size query.  A negative size raises what the query reported: an input error where
// the text says so, else a failed rocFFT plan.
at::Tensor workspace_or_raise(int64_t ws_bytes, const at::Tensor &like)
{
    if (ws_bytes < 0) check_rc(std::string(nfft_hip_last_error()).rfind("Input mismatch", 0) == 0 ? NFFT_HIP_EINVAL : NFFT_HIP_EFFT);
    return byte_buffer(ws_bytes, like);
}

// A coefficient tensor: its bandwidth (spectral only), columns per row, type and trailing (column) shape
struct Coeffs {
    int64_t N = 0, C = 1;
    bool real_input = true;
    std::vector<int64_t> cols;
    int64_t Cr() const { return real_input ? C : 2 * C; }  // real columns: a complex value is two
    std::vector<int64_t> shape(std::vector<int64_t> lead) const { lead.insert(lead.end(), cols.begin(), cols.end()); return lead; }
};

// check_spectral_coeffs_input (core_cuda.cu:89-115): x [B, N, ..., N, *cols]
Coeffs check_spectral(const at::Tensor &x, const Points &p)
{
    Coeffs c;
    c.real_input = real_dtype(x);
    CHECK_INPUT(x.dim() >= p.dim + 1);
    CHECK_INPUT(x.size(0) == p.B);
    CHECK_INPUT(x.device() == p.pos.device());
    c.N = x.size(1);
    CHECK_INPUT(c.N >= 2);
    for (int d = 2; d <= p.dim; ++d) CHECK_INPUT(x.size(d) == c.N);
    for (int64_t d = p.dim + 1; d < x.dim(); ++d) {
        c.C *= x.size(d);
        c.cols.push_back(x.size(d));
    }
    return c;
}

// check_spatial_coeffs_input (core_cuda.cu:69-86): x [n, ...] with `lead` leading dimensions before the columns
Coeffs check_spatial(const at::Tensor &x, int64_t n, int64_t lead = 1)
{
    Coeffs c;
    c.real_input = real_dtype(x);
    CHECK_INPUT(x.dim() >= lead);
    CHECK_INPUT(x.size(0) == n);
    for (int64_t d = lead; d < x.dim(); ++d) {
        c.C *= x.size(d);
        c.cols.push_back(x.size(d));
    }
    return c;
}

// Sources and targets of a pair sum, checked as the reference's fastsum does (core_cuda.cu:552-568): one point set on both
// sides (the same tensors) is checked once.
struct PointPair { Points ps, pt; bool shared; };
PointPair check_point_pair(const at::Tensor &sources, const at::Tensor &targets, const c10::optional<at::Tensor> &opt_source_batch,
                           const c10::optional<at::Tensor> &opt_target_batch)
{
    PointPair pp;
    pp.ps = check_points(sources, opt_source_batch, "(*out_batch)");
    const bool same_batch = (!opt_source_batch.has_value() && !opt_target_batch.has_value()) ||
                            (opt_source_batch.has_value() && opt_target_batch.has_value() &&
                             opt_source_batch->is_same(*opt_target_batch));
    pp.shared = sources.is_same(targets) && same_batch;
    pp.pt = pp.shared ? pp.ps : check_points(targets, opt_target_batch, "(*out_batch)");
    CHECK_INPUT(pp.pt.dim == pp.ps.dim);
    CHECK_INPUT(pp.pt.B == pp.ps.B);
    return pp;
}

// rows [n, row] float32 of x (complex values: real and imaginary parts as columns) in the order `order`
at::Tensor real_rows(const at::Tensor &x, bool real_input, int64_t n, int64_t row, const at::Tensor &order)
{
    const at::Tensor xc = x.contiguous();
    return (real_input ? xc : at::view_as_real(xc)).reshape({n, row}).index_select(0, order);
}

// the way back: z [n, row] float32 (n > 0) as x's type in `shape`
at::Tensor complex_back(const at::Tensor &z, bool real_input, const std::vector<int64_t> &shape)
{
    return (real_input ? z : at::view_as_complex(z.reshape({z.size(0), -1, 2}))).reshape(shape);
}

// ---- point-plan cache -------------------------------------------------------------------------------------
// The tile-sorted copy of the points depends only on (pos, batch, N, m).  Adjoint <-> forward pairs on the same
// points (autograd backward, a forward fed by an adjoint, fastsum -- the reference exploits
// sources.is_same(targets), core_cuda.cu:552-564) reuse it instead of re-binning.  Two entries (sources and
// targets of a fastsum), least recently used out.  Keyed on tensor identity + version counter: in-place edits
// through the tensor invalidate a plan; writes that bypass the version counter (pos.data, foreign kernels,
// DLPack aliases) do NOT -- callers who do that turn the cache off (torch_nfft_amd.ops.plan_cache_enabled(False))
// or clear it.  A plan is built on one stream and may be consumed on another: the consumer's stream waits for the
// build event and the plan's storage is recorded on it, so the allocator does not recycle it early.
struct PlanKey {
    const void *pos_ptr = nullptr, *batch_ptr = nullptr;
    int64_t pos_version = -1, batch_version = -1, n = -1, B = -1, N = -1, m = -1;
    int dim = 0, device = -1, flags = 0;  // (a plan is only valid for the geometry hints it was built with)
    bool operator==(const PlanKey &o) const
    {
        return pos_ptr == o.pos_ptr && batch_ptr == o.batch_ptr && pos_version == o.pos_version &&
               batch_version == o.batch_version && n == o.n && B == o.B && N == o.N && m == o.m && dim == o.dim &&
               device == o.device && flags == o.flags;
    }
};
struct PlanEntry {
    PlanKey key;
    at::Tensor plan, pos, batch;  // pos / batch kept alive so that their addresses cannot be recycled
    void *stream = nullptr;
    hipEvent_t built = nullptr;
    uint64_t last_use = 0;
};
struct PlanCache {
    std::mutex mutex;
    PlanEntry entries[2];
    bool enabled = true;
    bool verify = true;  // check a cached plan's seal on every hit (plan_cache_control 5 / 6)
    int64_t hits = 0, misses = 0;
    uint64_t tick = 0;
    void clear()
    {
        for (PlanEntry &e : entries) {
            if (e.built) (void)hipEventDestroy(e.built);
            e = PlanEntry();
        }
    }
};
// (never destroyed: at process exit the tensors it holds would otherwise be released after torch's allocator and
// the HIP runtime have been torn down)
PlanCache &g_cache = *new PlanCache;

// Cache key of a point set, or std::nullopt-like `cacheable == false` for points the cache must not hold.
struct PlanLookup {
    PlanKey key;
    bool use_cache = false;
    void *stream = nullptr;
};

PlanLookup plan_lookup_key(const Points &p, const nfft_hip_problem &q)
{
    PlanLookup lk;
    lk.stream = stream_of(p.pos);
    // Inference tensors carry no version counter (Tensor::_version() throws): such points are planned afresh in
    // every call and never enter the cache -- an in-place edit could not be told from the cached state.
    const bool cacheable = !p.pos.is_inference() && !(p.batch.defined() && p.batch.is_inference());
    PlanKey &key = lk.key;
    key.pos_ptr = p.pos.data_ptr();
    key.batch_ptr = p.batch.defined() ? p.batch.data_ptr() : nullptr;
    key.n = p.n; key.B = p.B; key.N = q.N; key.m = q.m; key.dim = p.dim; key.device = p.pos.device().index();
    // (the owner-computes spreading plan of a sparse problem has another tiling from two columns up: api.hip plan_route)
    key.flags = q.flags | (q.num_columns >= 2 ? (1 << 30) : 0);
    lk.use_cache = g_cache.enabled && cacheable;  // (read under the lock by the callers below)
    if (lk.use_cache) {
        key.pos_version = (int64_t)p.pos._version();
        key.batch_version = p.batch.defined() ? (int64_t)p.batch._version() : -1;
    }
    return lk;
}

// a cached plan for these points, made safe to use on the caller's stream; undefined tensor on a miss (lock held)
at::Tensor cache_find(const PlanLookup &lk)
{
    if (!lk.use_cache) return at::Tensor();
    for (PlanEntry &e : g_cache.entries) {
        if (e.plan.defined() && e.key == lk.key) {
            ++g_cache.hits;
            e.last_use = ++g_cache.tick;
            if (e.stream != lk.stream) {
                TORCH_CHECK(hipStreamWaitEvent((hipStream_t)lk.stream, e.built, 0) == hipSuccess,
                            "hipStreamWaitEvent failed");
                e.plan.record_stream(c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(lk.key.device));
            }
            return e.plan;
        }
    }
    return at::Tensor();
}

// enter a plan that has just been enqueued on lk.stream (lock held)
void cache_insert(const PlanLookup &lk, const Points &p, const at::Tensor &plan)
{
    if (!lk.use_cache) return;
    PlanEntry *slot = &g_cache.entries[0];
    if (g_cache.entries[0].plan.defined() &&
        (!g_cache.entries[1].plan.defined() || g_cache.entries[1].last_use < g_cache.entries[0].last_use))
        slot = &g_cache.entries[1];
    if (slot->built && slot->key.device != lk.key.device) {  // events belong to the device they were created on
        (void)hipEventDestroy(slot->built);
        slot->built = nullptr;
    }
    if (!slot->built)
        TORCH_CHECK(hipEventCreateWithFlags(&slot->built, hipEventDisableTiming) == hipSuccess, "hipEventCreate failed");
    TORCH_CHECK(hipEventRecord(slot->built, (hipStream_t)lk.stream) == hipSuccess, "hipEventRecord failed");
    slot->key = lk.key;
    slot->plan = plan;
    slot->pos = p.pos;
    slot->batch = p.batch;
    slot->stream = lk.stream;
    slot->last_use = ++g_cache.tick;
}

at::Tensor new_plan_buffer(const Points &p, const nfft_hip_problem &q, int64_t &nbytes)
{
    nbytes = nfft_hip_plan_bytes(&q);
    if (nbytes < 0) check_rc(NFFT_HIP_EINVAL);
    return byte_buffer(nbytes, p.pos);
}

at::Tensor get_plan(const Points &p, const nfft_hip_problem &q)
{
    std::lock_guard<std::mutex> lock(g_cache.mutex);
    const PlanLookup lk = plan_lookup_key(p, q);
    const float *pos = p.pos.data_ptr<float>();
    const int64_t *batch = p.batch.defined() ? p.batch.data_ptr<int64_t>() : nullptr;
    at::Tensor plan = cache_find(lk);
    if (plan.defined()) {
        // A plan from an earlier call: identity + version say the points are the same, the seal checks that they ARE (a
        // write behind the version counter -- pos.data, a foreign kernel, a DLPack alias -- would otherwise give a wrong
        // transform silently; the reference recomputes per call, core_cuda.cu:188-211).  One streaming pass over pos /
        // batch on the caller's stream; a mismatch is reported like every device-side fault: the next operator raises.
        if (g_cache.verify) check_rc(nfft_hip_plan_verify(&q, pos, batch, plan.data_ptr(), lk.stream));
        return plan;
    }
    ++g_cache.misses;
    int64_t nbytes = 0;
    plan = new_plan_buffer(p, q, nbytes);
    check_rc(nfft_hip_plan_points(&q, pos, batch, plan.data_ptr(), nbytes, lk.stream));
    cache_insert(lk, p, plan);
    return plan;
}

// action: 0 clear, 1 enable, 2 disable (and clear), 3 -> hits, 4 -> misses, 5 / 6 seal verification on / off
int64_t plan_cache_control(int64_t action)
{
    std::lock_guard<std::mutex> lock(g_cache.mutex);
    if (action >= 0 && action <= 2) {  // the remembered batch-vector ends follow the same switches
        std::lock_guard<std::mutex> lock2(g_ends.mutex);
        g_ends.clear();
        if (action != 0) g_ends.enabled = action == 1;
    }
    switch (action) {
    case 0: g_cache.clear(); return 0;
    case 1: g_cache.enabled = true; return 0;
    case 2: g_cache.enabled = false; g_cache.clear(); return 0;
    case 3: return g_cache.hits;
    case 4: return g_cache.misses;
    case 5: g_cache.verify = true; return 0;
    case 6: g_cache.verify = false; return 0;  // (for callers who guarantee they never write behind the version counter)
    }
    TORCH_CHECK(false, "unknown plan cache action");
}

// Faults a kernel reported since the last look (include/nfft_hip.h nfft_hip_check_status): raises, or returns 0.
// synchronize != 0 drains the current stream of the current device first.
int64_t check_status(int64_t synchronize)
{
    int dev = 0;
    TORCH_CHECK(hipGetDevice(&dev) == hipSuccess, "hipGetDevice failed");
    void *stream = (void *)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA((c10::DeviceIndex)dev).stream();
    check_rc(nfft_hip_check_status(stream, synchronize != 0 ? 1 : 0));
    return 0;
}

// ---- operators ----------------------------------------------------------------------------------------------
// torch_nfft::nfft_adjoint (csrc/core.cpp:43-55; driver core_cuda.cu:144-336)
at::Tensor nfft_adjoint(at::Tensor pos, at::Tensor x, c10::optional<at::Tensor> opt_batch, int64_t N, int64_t m,
                        int64_t real_output)
{
    TORCH_CHECK(x.is_cuda(), "torch_nfft.nfft_adjoint is currently only implemented for GPU tensors");
    const Points p = check_points(pos, opt_batch, "(*out_batch)");
    const Coeffs c = check_spatial(x, p.n);
    CHECK_INPUT(x.device() == pos.device());
    std::vector<int64_t> band{p.B};  // core_cuda.cu:298-304
    band.insert(band.end(), (size_t)p.dim, N);
    at::Tensor y = at::empty(c.shape(band), x.options().dtype(real_output ? at::kFloat : at::kComplexFloat));
    if (y.numel() == 0) return y;
    const at::Tensor xc = x.contiguous();
    const nfft_hip_problem q = problem(p, c.C, N, m);
    c10::DeviceGuard guard(x.device());
    if (!nfft_hip_plan_needed(&q)) {  // one fused kernel on the caller's points: no plan, no workspace
        check_rc(nfft_hip_adjoint(&q, p.pos.data_ptr<float>(), xc.data_ptr(), c.real_input ? 0 : 1,
                                  p.batch.defined() ? p.batch.data_ptr<int64_t>() : nullptr, real_output ? 1 : 0,
                                  y.data_ptr(), nullptr, 0, stream_of(x)));
        return y;
    }
    at::Tensor ws = workspace_or_raise(nfft_hip_adjoint_workspace_bytes(&q, c.real_input ? 0 : 1, real_output ? 1 : 0), x);
    const at::Tensor plan = get_plan(p, q);
    check_rc(nfft_hip_adjoint_planned(&q, plan.data_ptr(), xc.data_ptr(), c.real_input ? 0 : 1, real_output ? 1 : 0,
                                      y.data_ptr(), ws.data_ptr(), ws.numel(), stream_of(x)));
    return y;
}

// torch_nfft::nfft_forward (csrc/core.cpp:94-105; driver core_cuda.cu:340-531)
at::Tensor nfft_forward(at::Tensor pos, at::Tensor x, c10::optional<at::Tensor> opt_batch, int64_t m, int64_t real_output)
{
    TORCH_CHECK(x.is_cuda(), "torch_nfft.nfft_forward is currently only implemented for GPU tensors");
    const Points p = check_points(pos, opt_batch, "(*out_batch)");
    const Coeffs c = check_spectral(x, p);
    at::Tensor y = at::empty(c.shape({p.n}), x.options().dtype(real_output ? at::kFloat : at::kComplexFloat));
    if (y.numel() == 0) return y;
    const at::Tensor xc = x.contiguous();
    const nfft_hip_problem q = problem(p, c.C, c.N, m);
    c10::DeviceGuard guard(x.device());
    if (!nfft_hip_plan_needed(&q)) {
        check_rc(nfft_hip_forward(&q, p.pos.data_ptr<float>(), xc.data_ptr(), c.real_input ? 0 : 1,
                                  p.batch.defined() ? p.batch.data_ptr<int64_t>() : nullptr, real_output ? 1 : 0,
                                  y.data_ptr(), nullptr, 0, stream_of(x)));
        return y;
    }
    at::Tensor ws = workspace_or_raise(nfft_hip_forward_workspace_bytes(&q, c.real_input ? 0 : 1, real_output ? 1 : 0), x);
    const at::Tensor plan = get_plan(p, q);
    check_rc(nfft_hip_forward_planned(&q, plan.data_ptr(), xc.data_ptr(), c.real_input ? 0 : 1, real_output ? 1 : 0,
                                      y.data_ptr(), ws.data_ptr(), ws.numel(), stream_of(x)));
    return y;
}

// not in the reference: the gradient of nfft_forward(pos, x, batch, m, real_output) with respect to pos, weighted by w
// [n, Cr] (the real view of the upstream gradient, or of the adjoint's input: include/nfft_hip.h
// nfft_hip_forward_grad_points_planned).  Same checks and the same problem as the transform, so the plan the forward
// pass cached is reused; always planned.  Returns dpos [n, dim] float32.
at::Tensor nfft_forward_grad_points(at::Tensor pos, at::Tensor x, c10::optional<at::Tensor> opt_batch, int64_t m,
                                    int64_t real_output, at::Tensor w)
{
    TORCH_CHECK(x.is_cuda(), "torch_nfft._nfft_forward_grad_points is only implemented for GPU tensors");
    const Points p = check_points(pos, opt_batch, "(*out_batch)");
    const Coeffs c = check_spectral(x, p);
    const int64_t C = c.C, Cr = real_output ? C : 2 * C;
    CHECK_INPUT(w.is_cuda() && w.device() == pos.device());
    CHECK_INPUT(w.scalar_type() == at::kFloat);
    CHECK_INPUT(w.numel() == p.n * Cr);
    at::Tensor dpos = at::empty({p.n, (int64_t)p.dim}, pos.options());
    if (p.n == 0) return dpos;
    if (C == 0) return dpos.zero_();
    const at::Tensor xc = x.contiguous(), wc = w.contiguous();
    const nfft_hip_problem q = problem(p, C, c.N, m);
    c10::DeviceGuard guard(x.device());
    at::Tensor ws = workspace_or_raise(nfft_hip_forward_grad_workspace_bytes(&q, c.real_input ? 0 : 1, real_output ? 1 : 0), x);
    const at::Tensor plan = get_plan(p, q);
    check_rc(nfft_hip_forward_grad_points_planned(&q, plan.data_ptr(), xc.data_ptr(), c.real_input ? 0 : 1,
                                                  real_output ? 1 : 0, wc.data_ptr<float>(), dpos.data_ptr<float>(),
                                                  ws.data_ptr(), ws.numel(), stream_of(x)));
    return dpos;
}

// not in the reference: the backward of _nfft_forward_grad_points for an upstream v [n, dim] (second derivatives of both
// transforms; include/nfft_hip.h nfft_hip_forward_grad_points_backward_planned).  Returns (dxhat, dw, dpos) -- xhat's shape
// and type, [n, Cr] and [n, dim] float32; what was not asked for is an empty tensor.  Same checks and problem as
// _nfft_forward_grad_points, so the plan its forward pass cached is reused.
std::tuple<at::Tensor, at::Tensor, at::Tensor> nfft_forward_grad_points_backward(
    at::Tensor pos, at::Tensor x, c10::optional<at::Tensor> opt_batch, int64_t m, int64_t real_output, at::Tensor w,
    at::Tensor v, int64_t need_xhat, int64_t need_w, int64_t need_pos)
{
    TORCH_CHECK(x.is_cuda(), "torch_nfft._nfft_forward_grad_points_backward is only implemented for GPU tensors");
    const Points p = check_points(pos, opt_batch, "(*out_batch)");
    const Coeffs c = check_spectral(x, p);
    const int64_t C = c.C, Cr = real_output ? C : 2 * C;
    CHECK_INPUT(w.is_cuda() && w.device() == pos.device());
    CHECK_INPUT(w.scalar_type() == at::kFloat);
    CHECK_INPUT(w.numel() == p.n * Cr);
    CHECK_INPUT(v.is_cuda() && v.device() == pos.device());
    CHECK_INPUT(v.scalar_type() == at::kFloat);
    CHECK_INPUT(v.numel() == p.n * p.dim);
    const at::TensorOptions fo = pos.options();
    at::Tensor dx = need_xhat ? at::empty_like(x, at::MemoryFormat::Contiguous) : at::empty({0}, x.options());
    at::Tensor dw = need_w ? at::empty({p.n, Cr}, fo) : at::empty({0}, fo);
    at::Tensor dp = need_pos ? at::empty({p.n, (int64_t)p.dim}, fo) : at::empty({0}, fo);
    if (!need_xhat && !need_w && !need_pos) return {dx, dw, dp};
    if (p.n == 0 || C == 0) {  // G is empty or zero: so is every derivative of it, no native call
        if (need_xhat) dx.zero_();
        if (need_pos) dp.zero_();
        return {dx, dw, dp};
    }
    const at::Tensor xc = x.contiguous(), wc = w.contiguous(), vc = v.contiguous();
    const nfft_hip_problem q = problem(p, C, c.N, m);
    c10::DeviceGuard guard(x.device());
    at::Tensor ws = workspace_or_raise(
        nfft_hip_forward_grad_points_backward_workspace_bytes(&q, c.real_input ? 0 : 1, real_output ? 1 : 0), x);
    const at::Tensor plan = get_plan(p, q);
    check_rc(nfft_hip_forward_grad_points_backward_planned(
        &q, plan.data_ptr(), xc.data_ptr(), c.real_input ? 0 : 1, real_output ? 1 : 0, wc.data_ptr<float>(),
        vc.data_ptr<float>(), need_xhat ? dx.data_ptr() : nullptr, need_w ? dw.data_ptr<float>() : nullptr,
        need_pos ? dp.data_ptr<float>() : nullptr, ws.data_ptr(), ws.numel(), stream_of(x)));
    return {dx, dw, dp};
}

// Inputs of a fast summation, checked as the reference does (core_cuda.cu:535-590), and its two problems.
struct Fastsum : PointPair {
    bool real_coeffs, real_input;
    int64_t N, C;
    std::vector<int64_t> out_shape;  // [n_t, *x.shape[1:]]
    nfft_hip_problem qs, qt;
};

Fastsum check_fastsum(const at::Tensor &sources, const at::Tensor &targets, const at::Tensor &x, const at::Tensor &coeffs,
                      const c10::optional<at::Tensor> &opt_source_batch, const c10::optional<at::Tensor> &opt_target_batch,
                      int64_t m)
{
    TORCH_CHECK(x.is_cuda(), "torch_nfft.nfft_fastsum is currently only implemented for GPU tensors");
    TORCH_CHECK(coeffs.is_cuda(), "coeffs must be CUDA tensor");
    Fastsum f;
    static_cast<PointPair &>(f) = check_point_pair(sources, targets, opt_source_batch, opt_target_batch);
    CHECK_INPUT(coeffs.dim() == f.ps.dim);  // core_cuda.cu:585-590
    f.N = coeffs.size(0);
    for (int d = 1; d < f.ps.dim; ++d) CHECK_INPUT(coeffs.size(d) == f.N);
    f.real_coeffs = real_dtype(coeffs);
    const Coeffs cx = check_spatial(x, f.ps.n);
    CHECK_INPUT(x.device() == sources.device() && targets.device() == sources.device() &&
                coeffs.device() == sources.device());
    f.real_input = cx.real_input;
    f.C = cx.C;
    f.out_shape = cx.shape({f.pt.n});
    f.qs = problem(f.ps, f.C, f.N, m, NFFT_HIP_POINTS_IN_QUARTER_BALL);
    f.qt = problem(f.pt, f.C, f.N, m, NFFT_HIP_POINTS_IN_QUARTER_BALL);
    return f;
}

// y = K x, and with `band` the band spectrum coeffs * A_s(x) [B, N^dim, *cols] complex64 (nfft_hip_fastsum_band)
at::Tensor fastsum_run(const at::Tensor &x, const at::Tensor &coeffs, const Fastsum &f, at::Tensor *band)
{
    at::Tensor y = at::empty(f.out_shape, x.options());  // same dtype as x (core_cuda.cu:817-821)
    if (band) {
        std::vector<int64_t> shape{f.ps.B};
        for (int d = 0; d < f.ps.dim; ++d) shape.push_back(f.N);
        for (size_t d = 1; d < f.out_shape.size(); ++d) shape.push_back(f.out_shape[d]);
        *band = y.numel() == 0 ? at::zeros(shape, x.options().dtype(at::kComplexFloat))
                               : at::empty(shape, x.options().dtype(at::kComplexFloat));
    }
    if (y.numel() == 0) return y;
    const at::Tensor xc = x.contiguous(), cc = coeffs.contiguous();
    void *bp = band ? band->data_ptr() : nullptr;
    c10::DeviceGuard guard(x.device());
    const bool planned = nfft_hip_plan_needed(&f.qs) != 0 || nfft_hip_plan_needed(&f.qt) != 0;
    at::Tensor ws = workspace_or_raise(
        nfft_hip_fastsum_workspace_bytes(&f.qs, &f.qt, f.real_input ? 0 : 1, f.shared ? 1 : 0, planned ? 1 : 0), x);
    const int64_t ws_bytes = ws.numel();
    const Points &ps = f.ps, &pt = f.pt;
    if (!planned) {  // two fused kernels on the caller's points (1-D, grid in LDS): no plans
        const float *spos = ps.pos.data_ptr<float>(), *tpos = pt.pos.data_ptr<float>();
        const int64_t *sb = ps.batch.defined() ? ps.batch.data_ptr<int64_t>() : nullptr;
        const int64_t *tb = pt.batch.defined() ? pt.batch.data_ptr<int64_t>() : nullptr;
        if (band)
            check_rc(nfft_hip_fastsum_band(&f.qs, spos, sb, &f.qt, tpos, tb, xc.data_ptr(), f.real_input ? 0 : 1,
                                           cc.data_ptr(), f.real_coeffs ? 0 : 1, y.data_ptr(), bp, ws.data_ptr(), ws_bytes,
                                           stream_of(x)));
        else
            check_rc(nfft_hip_fastsum(&f.qs, spos, sb, &f.qt, tpos, tb, xc.data_ptr(), f.real_input ? 0 : 1, cc.data_ptr(),
                                      f.real_coeffs ? 0 : 1, y.data_ptr(), ws.data_ptr(), ws_bytes, stream_of(x)));
        return y;
    }
    const at::Tensor plan_s = get_plan(ps, f.qs);
    const at::Tensor plan_t = f.shared ? plan_s : get_plan(pt, f.qt);
    if (band)
        check_rc(nfft_hip_fastsum_band_planned(&f.qs, plan_s.data_ptr(), &f.qt, plan_t.data_ptr(), xc.data_ptr(),
                                               f.real_input ? 0 : 1, cc.data_ptr(), f.real_coeffs ? 0 : 1, y.data_ptr(), bp,
                                               ws.data_ptr(), ws_bytes, stream_of(x)));
    else
        check_rc(nfft_hip_fastsum_planned(&f.qs, plan_s.data_ptr(), &f.qt, plan_t.data_ptr(), xc.data_ptr(),
                                          f.real_input ? 0 : 1, cc.data_ptr(), f.real_coeffs ? 0 : 1, y.data_ptr(),
                                          ws.data_ptr(), ws_bytes, stream_of(x)));
    return y;
}

// torch_nfft::nfft_fastsum (csrc/core.cpp:108-121; driver core_cuda.cu:535-852)
at::Tensor nfft_fastsum(at::Tensor sources, at::Tensor targets, at::Tensor x, at::Tensor coeffs,
                        c10::optional<at::Tensor> opt_source_batch, c10::optional<at::Tensor> opt_target_batch, int64_t m)
{
    const Fastsum f = check_fastsum(sources, targets, x, coeffs, opt_source_batch, opt_target_batch, m);
    return fastsum_run(x, coeffs, f, nullptr);
}

// not in the reference: nfft_fastsum that also returns its band spectrum coeffs * A_s(x) [B, N^dim, *x.shape[1:]]
// complex64, which the gradient with respect to the targets gathers from.  Same checks, route and y as nfft_fastsum.
std::tuple<at::Tensor, at::Tensor> nfft_fastsum_band(at::Tensor sources, at::Tensor targets, at::Tensor x, at::Tensor coeffs,
                                                     c10::optional<at::Tensor> opt_source_batch,
                                                     c10::optional<at::Tensor> opt_target_batch, int64_t m)
{
    const Fastsum f = check_fastsum(sources, targets, x, coeffs, opt_source_batch, opt_target_batch, m);
    at::Tensor band;
    at::Tensor y = fastsum_run(x, coeffs, f, &band);
    return {y, band};
}

// not in the reference: the backward of nfft_fastsum with respect to x (real coeffs only), the sources and the targets
// (include/nfft_hip.h nfft_hip_fastsum_backward_planned).  dy: the gradient of y; band: nfft_fastsum_band's, needed for the
// targets.  The native call gets conj(coeffs), the array of the sources' grid.  Same problems as nfft_fastsum, so the
// plans its forward pass cached are reused.  Returns (dx, dsources, dtargets); what was not asked for is an empty tensor.
std::tuple<at::Tensor, at::Tensor, at::Tensor> nfft_fastsum_backward(
    at::Tensor sources, at::Tensor targets, at::Tensor x, at::Tensor dy, at::Tensor coeffs, c10::optional<at::Tensor> band,
    c10::optional<at::Tensor> opt_source_batch, c10::optional<at::Tensor> opt_target_batch, int64_t m, int64_t need_x,
    int64_t need_sources, int64_t need_targets)
{
    const Fastsum f = check_fastsum(sources, targets, x, coeffs, opt_source_batch, opt_target_batch, m);
    TORCH_CHECK(!need_x || f.real_coeffs, "_nfft_fastsum_backward: dx needs real coeffs (complex ones: the swapped fastsum)");
    CHECK_INPUT(dy.is_cuda() && dy.device() == x.device() && dy.scalar_type() == x.scalar_type());
    CHECK_INPUT(dy.sizes().vec() == f.out_shape);
    const bool want_band = need_targets && band.has_value() && band->defined();
    TORCH_CHECK(!need_targets || want_band, "_nfft_fastsum_backward: the targets' gradient needs the band");
    if (want_band) {
        CHECK_INPUT(band->is_cuda() && band->device() == x.device() && band->scalar_type() == at::kComplexFloat);
        int64_t size = f.ps.B * f.C;
        for (int d = 0; d < f.ps.dim; ++d) size *= f.N;
        CHECK_INPUT(band->numel() == size);
    }
    const at::TensorOptions fo = sources.options().dtype(at::kFloat);
    at::Tensor dx = need_x ? at::empty_like(x, at::MemoryFormat::Contiguous) : at::empty({0}, x.options());
    at::Tensor ds = need_sources ? at::empty({f.ps.n, (int64_t)f.ps.dim}, fo) : at::empty({0}, fo);
    at::Tensor dt = need_targets ? at::empty({f.pt.n, (int64_t)f.pt.dim}, fo) : at::empty({0}, fo);
    if (!need_x && !need_sources && !need_targets) return {dx, ds, dt};
    if (f.ps.n == 0 || f.pt.n == 0 || f.C == 0) {  // an empty sum: zero gradients, no native call
        if (need_x) dx.zero_();
        if (need_sources) ds.zero_();
        if (need_targets) dt.zero_();
        return {dx, ds, dt};
    }
    const at::Tensor xc = x.contiguous(), dyc = dy.contiguous();
    const at::Tensor cc = f.real_coeffs ? coeffs.contiguous() : coeffs.conj_physical().contiguous();
    const at::Tensor bc = want_band ? band->contiguous() : at::Tensor();
    c10::DeviceGuard guard(x.device());
    at::Tensor ws = workspace_or_raise(nfft_hip_fastsum_grad_workspace_bytes(&f.qs, &f.qt, f.real_input ? 0 : 1), x);
    // (gradient gathers always run on plans: on the small-grid routes the forward pass made none and they are built here)
    const at::Tensor plan_s = get_plan(f.ps, f.qs);
    const at::Tensor plan_t = f.shared ? plan_s : get_plan(f.pt, f.qt);
    check_rc(nfft_hip_fastsum_backward_planned(&f.qs, plan_s.data_ptr(), &f.qt, plan_t.data_ptr(), xc.data_ptr(),
                                               f.real_input ? 0 : 1, dyc.data_ptr(), cc.data_ptr(), f.real_coeffs ? 0 : 1,
                                               want_band ? bc.data_ptr() : nullptr, need_x ? dx.data_ptr() : nullptr,
                                               need_sources ? ds.data_ptr<float>() : nullptr,
                                               need_targets ? dt.data_ptr<float>() : nullptr, ws.data_ptr(), ws.numel(),
                                               stream_of(x)));
    return {dx, ds, dt};
}

// ---- Toeplitz normal operator A^H W A (not in the reference; include/nfft_hip.h) ---------------
// The bandwidth-N problem of a kernel grid [B, M, ..., M] (M = 2N); the cutoff only has to be valid.
nfft_hip_problem toeplitz_problem(int64_t dim, int64_t B, int64_t N, int64_t C)
{
    nfft_hip_problem q;
    q.dim = (int32_t)dim;
    q.flags = 0;
    q.num_points = 0;
    q.num_columns = C;
    q.batch_size = B;
    q.N = N;
    q.m = 1;
    return q;
}

// t = nfft_adjoint(weights, pos, batch, bandwidth 2N) [B, 2N, ..., 2N] complex64 -> the real kernel grid K [B, M, ..., M]
at::Tensor nfft_toeplitz_kernel(at::Tensor t)
{
    TORCH_CHECK(t.is_cuda(), "torch_nfft._nfft_toeplitz_kernel is currently only implemented for GPU tensors");
    CHECK_INPUT(t.scalar_type() == at::kComplexFloat);
    const int64_t dim = t.dim() - 1;
    CHECK_INPUT(dim >= 1 && dim <= 3);
    const int64_t B = t.size(0), M = t.size(1);
    CHECK_INPUT(B >= 1 && M >= 4 && M % 4 == 0);  // M = 2N, N even
    for (int64_t d = 2; d <= dim; ++d) CHECK_INPUT(t.size(d) == M);
    const at::Tensor tc = t.contiguous();
    at::Tensor K = at::empty(t.sizes(), t.options().dtype(at::kFloat));
    const nfft_hip_problem q = toeplitz_problem(dim, B, M / 2, 1);
    c10::DeviceGuard guard(t.device());
    at::Tensor ws = workspace_or_raise(nfft_hip_toeplitz_kernel_workspace_bytes(&q), t);
    check_rc(nfft_hip_toeplitz_kernel(&q, tc.data_ptr(), K.data_ptr<float>(), ws.data_ptr(), ws.numel(), stream_of(t)));
    return K;
}

// y = A^H W A x for x [B, N, ..., N, *cols] float32 or complex64 and the kernel grid of the same points; complex64
at::Tensor nfft_normal(at::Tensor kernel, at::Tensor x)
{
    TORCH_CHECK(x.is_cuda(), "torch_nfft._nfft_normal is currently only implemented for GPU tensors");
    TORCH_CHECK(kernel.is_cuda(), "kernel must be CUDA tensor");
    CHECK_INPUT(kernel.scalar_type() == at::kFloat);
    const bool real_input = real_dtype(x);
    const int64_t dim = kernel.dim() - 1;
    CHECK_INPUT(dim >= 1 && dim <= 3);
    CHECK_INPUT(x.dim() >= dim + 1);
    CHECK_INPUT(x.device() == kernel.device());
    const int64_t B = kernel.size(0), M = kernel.size(1);
    CHECK_INPUT(x.size(0) == B);
    const int64_t N = x.size(1);
    CHECK_INPUT(N >= 2 && M == 2 * N);
    for (int64_t d = 2; d <= dim; ++d) CHECK_INPUT(x.size(d) == N && kernel.size(d) == M);
    int64_t C = 1;
    for (int64_t d = dim + 1; d < x.dim(); ++d) C *= x.size(d);
    at::Tensor y = at::empty(x.sizes(), x.options().dtype(at::kComplexFloat));
    if (y.numel() == 0) return y;
    const at::Tensor xc = x.contiguous();
    at::Tensor kc = kernel.contiguous();
    if ((uintptr_t)kc.data_ptr() & 15u) kc = kc.clone();  // (a view at an odd offset: the multiply loads 16 bytes)
    const nfft_hip_problem q = toeplitz_problem(dim, B, N, C);
    c10::DeviceGuard guard(x.device());
    at::Tensor ws = workspace_or_raise(nfft_hip_toeplitz_workspace_bytes(&q), x);
    check_rc(nfft_hip_toeplitz_apply(&q, kc.data_ptr<float>(), xc.data_ptr(), real_input ? 0 : 1, y.data_ptr(),
                                     ws.data_ptr(), ws.numel(), stream_of(x)));
    return y;
}

// ---- near field of the fast summation for singular kernels (not in the reference) --------------
// A point set ordered by (point set, cell) for the pair kernels: the keys of include/nfft_hip.h, one stable sort and the
// first point of every cell by a sorted search.  Device work on the current stream only: no read-back.
struct CellOrder {
    at::Tensor pos, order, start;  // [n, dim] float32 in cell order; [n] int64: the caller's row; [B prod G + 1] int32
};

// Axis a has G[a] cells: cell = floor((pos[a] + shift) * scale[a]), clamped; the first axis is the fastest of the key.
//   nfft_hip_nearfield:       the ball of radius 1/4, cells of edge 1 / (2 G):    shift 1/4, scale 2 G
//   nfft_hip_ewald_near:      pos reduced to [-1/2, 1/2)^3, cells of edge 1 / G:   shift 1/2, scale G
//   nfft_hip_ewald_near_box:  the same with a cell count per axis
CellOrder cell_order(const at::Tensor &pos, const at::Tensor &batch, int64_t B, double shift, const int64_t *scale,
                     const int64_t *G, int dim)
{
    at::Tensor key;
    int64_t stride = 1;
    for (int a = 0; a < dim; ++a) {
        const at::Tensor cell = ((pos.select(1, a) + shift) * (double)scale[a]).floor().clamp(0, G[a] - 1).to(at::kLong);
        key = a == 0 ? cell : key + cell * stride;
        stride *= G[a];
    }
    if (batch.defined()) key = key + batch * stride;
    const auto sorted = at::sort(key, /*stable=*/true, /*dim=*/0, /*descending=*/false);
    CellOrder o;
    o.order = std::get<1>(sorted);
    o.start = at::searchsorted(std::get<0>(sorted), at::arange(B * stride + 1, key.options()), /*out_int32=*/true);
    o.pos = pos.index_select(0, o.order);
    return o;
}

CellOrder nearfield_cell_order(const Points &p, int64_t G)
{
    const int64_t Ga[3] = {G, G, G}, scale[3] = {2 * G, 2 * G, 2 * G};
    return cell_order(p.pos, p.batch, p.B, 0.25, scale, Ga, p.dim);
}

// The near-field problem of `n_in` streamed and `n_out` output points with Cr real columns.  poly: the coefficients of T_I;
// with gpoly those of T_I'(r) / r for the gradient kernels instead, copied to gpoly[8] (T_I itself is not read then).
nfft_hip_nearfield_problem nearfield_problem(const Points &ps, int64_t n_in, int64_t n_out, int64_t Cr, int64_t kernel, double c,
                                             double eps_I, at::ArrayRef<double> poly, double *gpoly = nullptr)
{
    nfft_hip_nearfield_problem q;
    q.dim = ps.dim;
    q.kernel = (int32_t)kernel;
    q.poly_terms = (int32_t)poly.size() + (gpoly ? 1 : 0);
    q.num_sources = n_in;
    q.num_targets = n_out;
    q.num_columns = Cr;
    q.batch_size = ps.B;
    q.c = c;
    q.eps_I = eps_I;
    for (size_t e = 0; e < 8; ++e) {
        q.poly[e] = 0.0;
        (gpoly ? gpoly : q.poly)[e] = e < poly.size() ? poly[e] : 0.0;
    }
    const int64_t G = nfft_hip_nearfield_cells(q.dim, eps_I, q.batch_size);
    if (G < 0) check_rc(NFFT_HIP_EINVAL);
    q.cells_per_axis = (int32_t)G;
    return q;
}

// z[i] = sum_{j: same point set, |t_i - s_j| < eps_I} (K(r_ij) - T_I(r_ij)) x[j]; x's type and trailing shape
at::Tensor nfft_nearfield(at::Tensor sources, at::Tensor targets, at::Tensor x, c10::optional<at::Tensor> opt_source_batch,
                          c10::optional<at::Tensor> opt_target_batch, int64_t kernel, double c, double eps_I,
                          at::ArrayRef<double> poly)
{
    TORCH_CHECK(x.is_cuda(), "torch_nfft._nfft_nearfield is currently only implemented for GPU tensors");
    const PointPair pp = check_point_pair(sources, targets, opt_source_batch, opt_target_batch);
    const Points &ps = pp.ps, &pt = pp.pt;
    const Coeffs cx = check_spatial(x, ps.n);
    CHECK_INPUT(x.device() == sources.device() && targets.device() == sources.device());
    CHECK_INPUT(poly.size() >= 1 && poly.size() <= 8);
    const std::vector<int64_t> out_shape = cx.shape({pt.n});
    const nfft_hip_nearfield_problem q = nearfield_problem(ps, ps.n, pt.n, cx.Cr(), kernel, c, eps_I, poly);
    const int64_t ws_bytes = nfft_hip_nearfield_workspace_bytes(&q);
    if (ws_bytes < 0) check_rc(NFFT_HIP_EINVAL);
    if (ps.n == 0 || pt.n == 0 || cx.C == 0) return at::zeros(out_shape, x.options());  // an empty sum: no launch
    c10::DeviceGuard guard(x.device());
    const CellOrder os = nearfield_cell_order(ps, q.cells_per_axis);
    const CellOrder ot = pp.shared ? os : nearfield_cell_order(pt, q.cells_per_axis);
    const at::Tensor xr = real_rows(x, cx.real_input, ps.n, q.num_columns, os.order);
    // (zeros: a target whose coordinates are not numbers has no cell and is not written)
    at::Tensor z = at::zeros({pt.n, q.num_columns}, x.options().dtype(at::kFloat));
    at::Tensor ws = byte_buffer(ws_bytes, x);
    check_rc(nfft_hip_nearfield(&q, os.pos.data_ptr<float>(), xr.data_ptr<float>(), os.start.data_ptr<int32_t>(),
                                ot.pos.data_ptr<float>(), ot.order.data_ptr<int64_t>(), ot.start.data_ptr<int32_t>(),
                                z.data_ptr<float>(), ws.data_ptr(), ws_bytes, stream_of(x)));
    return complex_back(z, cx.real_input, out_shape);
}

// The gradient of that sum at the targets and its transpose, g = (K' - T_I') / r:
//   transpose = false: x [n_s, *cols] -> G [n_t, dim, *cols],  G[i, a] = sum_j g(r_ij^2) (t_i - s_j)[a] x[j]
//   transpose = true:  x [n_t, dim, *cols] -> [n_s, *cols],    out[j] = sum_i g(r_ij^2) (t_i - s_j) . x[i]
// poly: the p - 1 Horner coefficients of T_I'(r) / r in (r / eps_I)^2.  The output side of the pair kernel is the targets
// for the gradient and the sources for the transpose: the two cell orders change places.
at::Tensor nfft_nearfield_gradient(at::Tensor sources, at::Tensor targets, at::Tensor x,
                                   c10::optional<at::Tensor> opt_source_batch, c10::optional<at::Tensor> opt_target_batch,
                                   int64_t kernel, double c, double eps_I, at::ArrayRef<double> poly, bool transpose)
{
    TORCH_CHECK(x.is_cuda(), "torch_nfft._nfft_nearfield_gradient is currently only implemented for GPU tensors");
    const PointPair pp = check_point_pair(sources, targets, opt_source_batch, opt_target_batch);
    const Points &ps = pp.ps, &pt = pp.pt;
    const Points &pin = transpose ? pt : ps, &pout = transpose ? ps : pt;  // streamed side, output side
    const int64_t dim = ps.dim;
    const Coeffs cx = check_spatial(x, pin.n, transpose ? 2 : 1);
    if (transpose) CHECK_INPUT(x.size(1) == dim);
    CHECK_INPUT(x.device() == sources.device() && targets.device() == sources.device());
    CHECK_INPUT(poly.size() >= 1 && poly.size() <= 7);
    const std::vector<int64_t> out_shape = transpose ? cx.shape({pout.n}) : cx.shape({pout.n, dim});
    double gpoly[8];
    const nfft_hip_nearfield_problem q = nearfield_problem(ps, pin.n, pout.n, cx.Cr(), kernel, c, eps_I, poly, gpoly);
    const int64_t ws_bytes = nfft_hip_nearfield_gradient_workspace_bytes(&q);
    if (ws_bytes < 0) check_rc(NFFT_HIP_EINVAL);
    if (ps.n == 0 || pt.n == 0 || cx.C == 0) return at::zeros(out_shape, x.options());  // an empty sum: no launch
    c10::DeviceGuard guard(x.device());
    const CellOrder oin = nearfield_cell_order(pin, q.cells_per_axis);
    const CellOrder oout = pp.shared ? oin : nearfield_cell_order(pout, q.cells_per_axis);
    const int64_t in_row = (transpose ? dim : 1) * q.num_columns, out_row = (transpose ? 1 : dim) * q.num_columns;
    const at::Tensor xr = real_rows(x, cx.real_input, pin.n, in_row, oin.order);
    // (zeros: an output point whose coordinates are not numbers has no cell and is not written)
    at::Tensor z = at::zeros({pout.n, out_row}, x.options().dtype(at::kFloat));
    at::Tensor ws = byte_buffer(ws_bytes, x);
    check_rc(nfft_hip_nearfield_gradient(&q, transpose ? 1 : 0, gpoly, oin.pos.data_ptr<float>(), xr.data_ptr<float>(),
                                         oin.start.data_ptr<int32_t>(), oout.pos.data_ptr<float>(),
                                         oout.order.data_ptr<int64_t>(), oout.start.data_ptr<int32_t>(), z.data_ptr<float>(),
                                         ws.data_ptr(), ws_bytes, stream_of(x)));
    return complex_back(z, cx.real_input, out_shape);
}

// The gradient of that sum with respect to the points: for z = nfft_nearfield(x) and dy = dL/dz,
//   dt[i, a] = sum_j g(r_ij^2) (t_i - s_j)[a] sum_c dy[i, c] x[j, c]      [n_t, dim]
//   ds[j, a] = sum_i g(r_ij^2) (s_j - t_i)[a] sum_c x[j, c] dy[i, c]      [n_s, dim]
// (ds, dt); a side that is not needed comes back empty.  Real and imaginary parts of complex values are columns.  Each
// cell order is built once and serves both sweeps: for dt the sources are streamed and the targets are the output side,
// for ds the other way round.  Shared points with both sides needed take ONE symmetric sweep: the total is returned as ds
// and dt is zeros.  poly: the p - 1 Horner coefficients of T_I'(r) / r in (r / eps_I)^2.
std::tuple<at::Tensor, at::Tensor> nfft_nearfield_point_gradient(at::Tensor sources, at::Tensor targets, at::Tensor x,
                                                                 at::Tensor dy, c10::optional<at::Tensor> opt_source_batch,
                                                                 c10::optional<at::Tensor> opt_target_batch, int64_t kernel,
                                                                 double c, double eps_I, at::ArrayRef<double> poly,
                                                                 bool need_sources, bool need_targets)
{
    TORCH_CHECK(x.is_cuda(), "torch_nfft._nfft_nearfield_point_gradient is currently only implemented for GPU tensors");
    const PointPair pp = check_point_pair(sources, targets, opt_source_batch, opt_target_batch);
    const Points &ps = pp.ps, &pt = pp.pt;
    const bool shared = pp.shared;
    const int64_t dim = ps.dim;
    const Coeffs cx = check_spatial(x, ps.n);
    const bool real_input = cx.real_input;
    CHECK_INPUT(dy.scalar_type() == x.scalar_type());
    CHECK_INPUT(dy.dim() == x.dim() && dy.size(0) == pt.n);
    CHECK_INPUT(x.device() == sources.device() && targets.device() == sources.device() && dy.device() == sources.device());
    CHECK_INPUT(poly.size() >= 1 && poly.size() <= 7);
    for (int64_t d = 1; d < x.dim(); ++d) CHECK_INPUT(dy.size(d) == x.size(d));
    double gpoly[8];
    const nfft_hip_nearfield_problem q = nearfield_problem(ps, ps.n, pt.n, cx.Cr(), kernel, c, eps_I, poly, gpoly);
    if (nfft_hip_nearfield_point_gradient_workspace_bytes(&q) < 0) check_rc(NFFT_HIP_EINVAL);
    const at::TensorOptions opts = sources.options();
    const bool symmetric = shared && need_sources && need_targets;
    // (zeros: an output point whose coordinates are not numbers has no cell and is not written)
    at::Tensor ds = need_sources ? at::zeros({ps.n, dim}, opts) : at::empty({0, dim}, opts);
    at::Tensor dt = need_targets ? at::zeros({pt.n, dim}, opts) : at::empty({0, dim}, opts);
    if (ps.n == 0 || pt.n == 0 || cx.C == 0 || (!need_sources && !need_targets)) return {ds, dt};  // empty sums: no launch
    c10::DeviceGuard guard(x.device());
    const CellOrder os = nearfield_cell_order(ps, q.cells_per_axis);
    const CellOrder ot = shared ? os : nearfield_cell_order(pt, q.cells_per_axis);
    const at::Tensor xr = real_rows(x, real_input, ps.n, q.num_columns, os.order);
    const at::Tensor dyr = real_rows(dy, real_input, pt.n, q.num_columns, ot.order);
    // one sweep: the streamed side (order, values) and the output side (order, values, result)
    auto sweep = [&](bool sym, const CellOrder &in, const at::Tensor &vin, const CellOrder &o, const at::Tensor &vout,
                     at::Tensor &out) {
        nfft_hip_nearfield_problem r = q;
        r.num_sources = in.pos.size(0);
        r.num_targets = o.pos.size(0);
        const int64_t ws_bytes = nfft_hip_nearfield_point_gradient_workspace_bytes(&r);
        if (ws_bytes < 0) check_rc(NFFT_HIP_EINVAL);
        at::Tensor ws = byte_buffer(ws_bytes, x);
        check_rc(nfft_hip_nearfield_point_gradient(&r, sym ? 1 : 0, gpoly, in.pos.data_ptr<float>(), vin.data_ptr<float>(),
                                                   in.start.data_ptr<int32_t>(), o.pos.data_ptr<float>(),
                                                   vout.data_ptr<float>(), o.order.data_ptr<int64_t>(),
                                                   o.start.data_ptr<int32_t>(), out.data_ptr<float>(), ws.data_ptr(), ws_bytes,
                                                   stream_of(x)));
    };
    if (symmetric) {
        sweep(true, os, xr, os, dyr, ds);
        return {ds, dt};
    }
    if (need_targets) sweep(false, os, xr, ot, dyr, dt);
    if (need_sources) sweep(false, ot, dyr, os, xr, ds);
    return {ds, dt};
}

// ---- near part of the Ewald sum for the periodic 1/r (not in the reference) --------------------
// p modulo 1 in [-1/2, 1/2): p - rint(p) is exact in float32 and equals p - floor(p + 1/2) wherever that sum is; what comes
// out as +1/2 is the point -1/2
at::Tensor torus_reduce(const at::Tensor &pos)
{
    const at::Tensor red = pos - pos.round();
    return at::where(red >= 0.5, red - 1.0, red);
}

// The cell order of points on the torus (nfft_hip_ewald_near_box's key; nfft_hip_ewald_near's with one count on every axis)
CellOrder torus_cell_order(const Points &p, const int32_t *cells)
{
    const int64_t G[3] = {cells[0], cells[1], cells[2]};
    return cell_order(torus_reduce(p.pos), p.batch, p.B, 0.5, G, G, 3);
}

// The charges x [n, *cols] of the Ewald operators, their pair-sum shapes and the (n, 3, *cols) field's
struct EwaldInput { Points p; Coeffs cx; std::vector<int64_t> z_shape, f_shape; };
EwaldInput check_ewald(const at::Tensor &pos, const at::Tensor &x, const c10::optional<at::Tensor> &opt_batch, bool with_field)
{
    EwaldInput in;
    in.p = check_points(pos, opt_batch, "batch");
    CHECK_INPUT(in.p.dim == 3);
    in.cx = check_spatial(x, in.p.n);
    CHECK_INPUT(x.device() == pos.device());
    in.z_shape = in.cx.shape({in.p.n});
    in.f_shape = with_field ? in.cx.shape({in.p.n, 3}) : std::vector<int64_t>{0};
    return in;
}

nfft_hip_ewald_box_problem ewald_box_problem(const Points &p, int64_t Cr, bool with_field, const std::vector<double> &box,
                                             double alpha, double r_cut)
{
    nfft_hip_ewald_box_problem q;
    q.with_field = with_field ? 1 : 0;
    q.num_points = p.n;
    q.num_columns = Cr;
    q.batch_size = p.B;
    q.alpha = alpha;
    q.r_cut = r_cut;
    for (int e = 0; e < 6; ++e) q.box[e] = box[e];
    if (nfft_hip_ewald_box_cells(q.box, r_cut, q.batch_size, q.cells) < 0) check_rc(NFFT_HIP_EINVAL);
    return q;
}

// (z, f) [n, Cr] and [n, 3 Cr] float32 back in x's type and shapes
std::tuple<at::Tensor, at::Tensor> ewald_result(const EwaldInput &in, const at::Tensor &z, const at::Tensor &f, bool with_field)
{
    return {complex_back(z, in.cx.real_input, in.z_shape), with_field ? complex_back(f, in.cx.real_input, in.f_shape) : f};
}

// (z, f): z[i] = sum_{j: same point set, 0 < r_ij < r_cut} erfc(alpha r_ij) / r_ij x[j] with r_ij the length of the minimum
// image d_ij of pos_i - pos_j on the unit torus, x's type and shape; with_field: f[i, a] = -sum_j g(r_ij^2) d_ij[a] x[j],
// [n, 3, *cols] (g = K'(r) / r of K = erfc(alpha r) / r), otherwise f is empty.  pos may hold any real values: they are
// taken modulo 1.
// (`sweep`: nfft_hip_ewald_near, or the dispersion sum's pair weights on the same problem, section 7j, or a closure with
// these arguments that binds the screening of section 7p)
template <class EwaldSweep>
std::tuple<at::Tensor, at::Tensor> ewald_near_op(EwaldSweep sweep, const at::Tensor &pos, const at::Tensor &x,
                                                 const c10::optional<at::Tensor> &opt_batch, double alpha, double r_cut,
                                                 bool with_field)
{
    const EwaldInput in = check_ewald(pos, x, opt_batch, with_field);
    const Points &p = in.p;
    nfft_hip_ewald_problem q;
    q.with_field = with_field ? 1 : 0;
    q.num_points = p.n;
    q.num_columns = in.cx.Cr();
    q.batch_size = p.B;
    q.alpha = alpha;
    q.r_cut = r_cut;
    const int64_t G = nfft_hip_ewald_near_cells(r_cut, q.batch_size);
    if (G < 0) check_rc(NFFT_HIP_EINVAL);
    q.cells_per_axis = (int32_t)G;
    const int64_t ws_bytes = nfft_hip_ewald_near_workspace_bytes(&q);
    if (ws_bytes < 0) check_rc(NFFT_HIP_EINVAL);
    if (p.n == 0 || in.cx.C == 0) return {at::zeros(in.z_shape, x.options()), at::zeros(in.f_shape, x.options())};  // no launch
    c10::DeviceGuard guard(x.device());
    const int32_t cells[3] = {q.cells_per_axis, q.cells_per_axis, q.cells_per_axis};
    const CellOrder o = torus_cell_order(p, cells);
    const at::Tensor xr = real_rows(x, in.cx.real_input, p.n, q.num_columns, o.order);
    // (zeros: a point whose coordinates are not numbers has no cell and is not written)
    const at::TensorOptions opts = x.options().dtype(at::kFloat);
    at::Tensor z = at::zeros({p.n, q.num_columns}, opts);
    at::Tensor f = with_field ? at::zeros({p.n, 3 * q.num_columns}, opts) : at::empty({0}, x.options());
    at::Tensor ws = byte_buffer(ws_bytes, x);
    check_rc(sweep(&q, o.pos.data_ptr<float>(), xr.data_ptr<float>(), o.start.data_ptr<int32_t>(), o.order.data_ptr<int64_t>(),
                   z.data_ptr<float>(), with_field ? f.data_ptr<float>() : nullptr, ws.data_ptr(), ws_bytes, stream_of(x)));
    return ewald_result(in, z, f, with_field);
}

std::tuple<at::Tensor, at::Tensor> nfft_ewald_near(at::Tensor pos, at::Tensor x, c10::optional<at::Tensor> opt_batch,
                                                   double alpha, double r_cut, bool with_field)
{
    TORCH_CHECK(x.is_cuda(), "torch_nfft._nfft_ewald_near is currently only implemented for GPU tensors");
    return ewald_near_op(nfft_hip_ewald_near, pos, x, opt_batch, alpha, r_cut, with_field);
}

// ---- the same pair sum in an orthorhombic or triclinic box (not in the reference) ---------------
// (z, f) of nfft_ewald_near in the box A = box (A00, A10, A11, A20, A21, A22; rows = lattice vectors): pos holds FRACTIONAL
// coordinates, taken modulo 1; r_ij is the length of d_ij = (ds - rint(ds)) A and f is Cartesian.
template <class EwaldBoxSweep>
std::tuple<at::Tensor, at::Tensor> ewald_near_box_op(EwaldBoxSweep sweep, const at::Tensor &pos, const at::Tensor &x,
                                                     const c10::optional<at::Tensor> &opt_batch, const std::vector<double> &box,
                                                     double alpha, double r_cut, bool with_field)
{
    const EwaldInput in = check_ewald(pos, x, opt_batch, with_field);
    const Points &p = in.p;
    CHECK_INPUT(box.size() == 6);
    const nfft_hip_ewald_box_problem q = ewald_box_problem(p, in.cx.Cr(), with_field, box, alpha, r_cut);
    const int64_t ws_bytes = nfft_hip_ewald_near_box_workspace_bytes(&q);
    if (ws_bytes < 0) check_rc(NFFT_HIP_EINVAL);
    if (p.n == 0 || in.cx.C == 0) return {at::zeros(in.z_shape, x.options()), at::zeros(in.f_shape, x.options())};  // no launch
    c10::DeviceGuard guard(x.device());
    const CellOrder o = torus_cell_order(p, q.cells);
    const at::Tensor xr = real_rows(x, in.cx.real_input, p.n, q.num_columns, o.order);
    // (zeros: a point whose coordinates are not numbers has no cell and is not written)
    const at::TensorOptions opts = x.options().dtype(at::kFloat);
    at::Tensor z = at::zeros({p.n, q.num_columns}, opts);
    at::Tensor f = with_field ? at::zeros({p.n, 3 * q.num_columns}, opts) : at::empty({0}, x.options());
    at::Tensor ws = byte_buffer(ws_bytes, x);
    check_rc(sweep(&q, o.pos.data_ptr<float>(), xr.data_ptr<float>(), o.start.data_ptr<int32_t>(), o.order.data_ptr<int64_t>(),
                   z.data_ptr<float>(), with_field ? f.data_ptr<float>() : nullptr, ws.data_ptr(), ws_bytes, stream_of(x)));
    return ewald_result(in, z, f, with_field);
}

std::tuple<at::Tensor, at::Tensor> nfft_ewald_near_box(at::Tensor pos, at::Tensor x, c10::optional<at::Tensor> opt_batch,
                                                       std::vector<double> box, double alpha, double r_cut, bool with_field)
{
    TORCH_CHECK(x.is_cuda(), "torch_nfft._nfft_ewald_near_box is currently only implemented for GPU tensors");
    return ewald_near_box_op(nfft_hip_ewald_near_box, pos, x, opt_batch, box, alpha, r_cut, with_field);
}

// ---- near part of the dispersion Ewald sum, the periodic 1/r^6 (not in the reference) -----------
// (z, f) as nfft_ewald_near and nfft_ewald_near_box with the pair weights w(r) = e^(-a^2) (1 + a^2 + a^4 / 2) / r^6, a = alpha r:
// z[i] = sum_j w(r_ij) x[j], f[i, a] = sum_j (-w'(r_ij) / r_ij) d_ij[a] x[j] (minus the gradient)
std::tuple<at::Tensor, at::Tensor> nfft_ewald_dispersion_near(at::Tensor pos, at::Tensor x, c10::optional<at::Tensor> opt_batch,
                                                              double alpha, double r_cut, bool with_field)
{
    TORCH_CHECK(x.is_cuda(), "torch_nfft._nfft_ewald_dispersion_near is currently only implemented for GPU tensors");
    return ewald_near_op(nfft_hip_ewald_dispersion_near, pos, x, opt_batch, alpha, r_cut, with_field);
}

std::tuple<at::Tensor, at::Tensor> nfft_ewald_dispersion_near_box(at::Tensor pos, at::Tensor x,
                                                                  c10::optional<at::Tensor> opt_batch, std::vector<double> box,
                                                                  double alpha, double r_cut, bool with_field)
{
    TORCH_CHECK(x.is_cuda(), "torch_nfft._nfft_ewald_dispersion_near_box is currently only implemented for GPU tensors");
    return ewald_near_box_op(nfft_hip_ewald_dispersion_near_box, pos, x, opt_batch, box, alpha, r_cut, with_field);
}

// ---- virial tensor of the Ewald sum (not in the reference) --------------------------------------
// [B, 7, *cols] float64: per point set and column the near part of the energy and of the virial W_ab = -dU / d eps_ab
// (xx, yy, zz, yz, xz, xy) of the real charges x at the FRACTIONAL positions pos in the box A = box, taken modulo 1 and
// ordered by cell exactly as nfft_ewald_near_box does
// (`reduce`: nfft_hip_ewald_virial_near, or the dispersion sum's pair weights on the same problem, section 7k, or a closure
// with these arguments that binds the screening of section 7p)
template <class VirialNearReduce>
at::Tensor virial_near_op(VirialNearReduce reduce, const at::Tensor &pos, const at::Tensor &x,
                          const c10::optional<at::Tensor> &opt_batch, const std::vector<double> &box, double alpha, double r_cut)
{
    const EwaldInput in = check_ewald(pos, x, opt_batch, false);
    const Points &p = in.p;
    CHECK_INPUT(box.size() == 6);
    CHECK_INPUT(in.cx.real_input);  // (the energy is bilinear: real charges only)
    const int64_t C = in.cx.C;
    const std::vector<int64_t> shape = in.cx.shape({p.B, 7});
    const nfft_hip_ewald_box_problem q = ewald_box_problem(p, C, false, box, alpha, r_cut);
    const int64_t ws_bytes = nfft_hip_ewald_virial_near_workspace_bytes(&q);
    if (ws_bytes < 0) check_rc(NFFT_HIP_EINVAL);
    const at::TensorOptions opts = x.options().dtype(at::kDouble);
    if (p.n == 0 || C == 0) return at::zeros(shape, opts);  // no launch
    c10::DeviceGuard guard(x.device());
    const CellOrder o = torus_cell_order(p, q.cells);
    const at::Tensor xr = real_rows(x, true, p.n, C, o.order);
    at::Tensor out = at::zeros({p.B, 7, C}, opts);
    at::Tensor ws = byte_buffer(ws_bytes, x);
    check_rc(reduce(&q, o.pos.data_ptr<float>(), xr.data_ptr<float>(), o.start.data_ptr<int32_t>(), out.data_ptr<double>(),
                    ws.data_ptr(), ws_bytes, stream_of(x)));
    return out.reshape(shape);
}

at::Tensor nfft_ewald_virial_near(at::Tensor pos, at::Tensor x, c10::optional<at::Tensor> opt_batch, std::vector<double> box,
                                  double alpha, double r_cut)
{
    TORCH_CHECK(x.is_cuda(), "torch_nfft._nfft_ewald_virial_near is currently only implemented for GPU tensors");
    return virial_near_op(nfft_hip_ewald_virial_near, pos, x, opt_batch, box, alpha, r_cut);
}

// [B, 7, *cols] float64: the far part of the same from band [B, N, N, N, *cols] complex64 (nfft_adjoint of the charges)
// and the splitting's coeffs [N, N, N] float32; kappa = A^-1 k is formed in the kernel from box and the index.
// (`reduce(N, B, C, band, coeffs, A^-1, out, workspace, bytes, stream)`: nfft_hip_ewald_virial_far with its alpha, or the
// dispersion sum's reduction with its second grid, section 7k)
// (`workspace_bytes`: the size query that goes with `reduce`)
template <class Reduce>
at::Tensor virial_far_op(const at::Tensor &band, const at::Tensor &coeffs, const std::vector<double> &box, Reduce &&reduce,
                         int64_t (*workspace_bytes)(int64_t, int64_t, int64_t) = nfft_hip_ewald_virial_far_workspace_bytes)
{
    CHECK_INPUT(band.scalar_type() == at::kComplexFloat);
    CHECK_INPUT(coeffs.scalar_type() == at::kFloat);
    CHECK_INPUT(coeffs.device() == band.device());
    CHECK_INPUT(box.size() == 6);
    CHECK_INPUT(band.dim() >= 4 && coeffs.dim() == 3);
    const int64_t B = band.size(0), N = band.size(1);
    for (int64_t d = 0; d < 3; ++d) CHECK_INPUT(band.size(1 + d) == N && coeffs.size(d) == N);
    int64_t C = 1;
    std::vector<int64_t> shape{B, 7};
    for (int64_t d = 4; d < band.dim(); ++d) {
        C *= band.size(d);
        shape.push_back(band.size(d));
    }
    const at::TensorOptions opts = band.options().dtype(at::kDouble);
    if (B == 0) return at::zeros(shape, opts);
    const double a00 = box[0], a10 = box[1], a11 = box[2], a20 = box[3], a21 = box[4], a22 = box[5];
    CHECK_INPUT(a00 > 0.0 && a11 > 0.0 && a22 > 0.0);
    const double i00 = 1.0 / a00, i11 = 1.0 / a11, i22 = 1.0 / a22;
    const double inv[6] = {i00, -a10 * i00 * i11, i11, (a10 * a21 - a11 * a20) * i00 * i11 * i22, -a21 * i11 * i22, i22};
    const int64_t ws_bytes = workspace_bytes(N, B, C);
    if (ws_bytes < 0) check_rc(NFFT_HIP_EINVAL);
    if (C == 0) return at::zeros(shape, opts);  // no launch
    c10::DeviceGuard guard(band.device());
    const at::Tensor bc = band.contiguous(), cc = coeffs.contiguous();
    at::Tensor out = at::zeros({B, 7, C}, opts);
    at::Tensor ws = byte_buffer(ws_bytes, band);
    check_rc(reduce(N, B, C, bc.data_ptr(), cc.data_ptr<float>(), inv, out.data_ptr<double>(), ws.data_ptr(), ws_bytes,
                    stream_of(band)));
    return out.reshape(shape);
}

at::Tensor nfft_ewald_virial_far(at::Tensor band, at::Tensor coeffs, std::vector<double> box, double alpha)
{
    TORCH_CHECK(band.is_cuda(), "torch_nfft._nfft_ewald_virial_far is currently only implemented for GPU tensors");
    CHECK_INPUT(alpha > 0.0);
    const double pi = 3.14159265358979323846;
    return virial_far_op(band, coeffs, box, [&](int64_t N, int64_t B, int64_t C, const void *b, const float *c, const double *inv,
                                                double *out, void *ws, int64_t ws_bytes, void *stream) {
        return nfft_hip_ewald_virial_far(N, B, C, b, c, inv, pi * pi / (alpha * alpha), out, ws, ws_bytes, stream);
    });
}

// ---- potential, field, energy and virial of the Ewald sum in one pass (not in the reference) ----
// (z, f, seven): z and f of nfft_ewald_near_box with the field and seven of nfft_ewald_virial_near from one walk over the
// pairs: the same checks, reduction of pos, cell order and index as those two, real charges only
std::tuple<at::Tensor, at::Tensor, at::Tensor> nfft_ewald_step_near(at::Tensor pos, at::Tensor x, c10::optional<at::Tensor> opt_batch,
                                                                    std::vector<double> box, double alpha, double r_cut)
{
    TORCH_CHECK(x.is_cuda(), "torch_nfft._nfft_ewald_step_near is currently only implemented for GPU tensors");
    const EwaldInput in = check_ewald(pos, x, opt_batch, true);
    const Points &p = in.p;
    CHECK_INPUT(box.size() == 6);
    CHECK_INPUT(in.cx.real_input);  // (the energy is bilinear: real charges only)
    const int64_t C = in.cx.C;
    const std::vector<int64_t> seven_shape = in.cx.shape({p.B, 7});
    const nfft_hip_ewald_box_problem q = ewald_box_problem(p, C, true, box, alpha, r_cut);
    const int64_t ws_bytes = nfft_hip_ewald_step_near_workspace_bytes(&q);
    if (ws_bytes < 0) check_rc(NFFT_HIP_EINVAL);
    const at::TensorOptions opts = x.options().dtype(at::kFloat), opts64 = x.options().dtype(at::kDouble);
    if (p.n == 0 || C == 0)  // no launch
        return {at::zeros(in.z_shape, x.options()), at::zeros(in.f_shape, x.options()), at::zeros(seven_shape, opts64)};
    c10::DeviceGuard guard(x.device());
    const CellOrder o = torus_cell_order(p, q.cells);
    const at::Tensor xr = real_rows(x, true, p.n, C, o.order);
    // (zeros: a point whose coordinates are not numbers has no cell and is not written)
    at::Tensor z = at::zeros({p.n, C}, opts);
    at::Tensor f = at::zeros({p.n, 3 * C}, opts);
    at::Tensor out = at::zeros({p.B, 7, C}, opts64);
    at::Tensor ws = byte_buffer(ws_bytes, x);
    check_rc(nfft_hip_ewald_step_near(&q, o.pos.data_ptr<float>(), xr.data_ptr<float>(), o.start.data_ptr<int32_t>(),
                                      o.order.data_ptr<int64_t>(), z.data_ptr<float>(), f.data_ptr<float>(),
                                      out.data_ptr<double>(), ws.data_ptr(), ws_bytes, stream_of(x)));
    const auto zf = ewald_result(in, z, f, true);
    return {std::get<0>(zf), std::get<1>(zf), out.reshape(seven_shape)};
}

// (spectra, seven): spectra [B, N, N, N, 4, *cols] complex64 = band times (b_k, 2 pi i kappa_a b_k), the four spectra whose
// forward transform is the far part of (phi, E), and seven of nfft_ewald_virial_far, from one read of band
std::tuple<at::Tensor, at::Tensor> nfft_ewald_step_spectral(at::Tensor band, at::Tensor coeffs, std::vector<double> box, double alpha)
{
    TORCH_CHECK(band.is_cuda(), "torch_nfft._nfft_ewald_step_spectral is currently only implemented for GPU tensors");
    CHECK_INPUT(alpha > 0.0);
    CHECK_INPUT(band.dim() >= 4);
    const double pi = 3.14159265358979323846;
    std::vector<int64_t> shape = band.sizes().vec();
    shape.insert(shape.begin() + 4, 4);
    at::Tensor spectra;
    at::Tensor seven = virial_far_op(band, coeffs, box, [&](int64_t N, int64_t B, int64_t C, const void *b, const float *c,
                                                            const double *inv, double *out, void *ws, int64_t ws_bytes, void *stream) {
        spectra = at::empty(shape, band.options());  // (every entry is written)
        return nfft_hip_ewald_step_spectral(N, B, C, b, c, inv, pi * pi / (alpha * alpha), spectra.data_ptr(), out, ws, ws_bytes, stream);
    }, nfft_hip_ewald_step_spectral_workspace_bytes);
    if (!spectra.defined()) spectra = at::zeros(shape, band.options());  // (no point sets or no columns: no launch)
    return {spectra, seven};
}

// ---- forces, energies and virial of a Lennard-Jones + Coulomb model in one pass (not in the reference; section 7r) ----
// (f, eight): f [n, 3] float32, the pair part of the force on every point, and eight [B, 8] float64 (U_C, U_LJ, then xx, yy,
// zz, yz, xz, xy of the virial), from one walk over the pairs within r_cut.  xs [n, 3] float32 = (q, c, a) per point; pos
// fractional, reduced and ordered by cell as nfft_ewald_step_near does
std::tuple<at::Tensor, at::Tensor> nfft_ewald_lj_step_near(at::Tensor pos, at::Tensor xs, c10::optional<at::Tensor> opt_batch,
                                                           std::vector<double> box, double alpha_coulomb, double alpha_dispersion,
                                                           double r_cut)
{
    TORCH_CHECK(xs.is_cuda(), "torch_nfft._nfft_ewald_lj_step_near is currently only implemented for GPU tensors");
    const Points p = check_points(pos, opt_batch, "batch");
    CHECK_INPUT(p.dim == 3);
    CHECK_INPUT(xs.scalar_type() == at::kFloat && xs.dim() == 2 && xs.size(0) == p.n && xs.size(1) == 3);
    CHECK_INPUT(xs.device() == pos.device());
    CHECK_INPUT(box.size() == 6);
    const nfft_hip_ewald_box_problem q = ewald_box_problem(p, 1, true, box, alpha_coulomb, r_cut);
    const int64_t ws_bytes = nfft_hip_ewald_lj_step_near_workspace_bytes(&q, alpha_dispersion);
    if (ws_bytes < 0) check_rc(NFFT_HIP_EINVAL);
    const at::TensorOptions opts64 = xs.options().dtype(at::kDouble);
    // (zeros: a point whose coordinates are not numbers has no cell and is not written)
    at::Tensor f = at::zeros({p.n, 3}, xs.options());
    at::Tensor out = at::zeros({p.B, 8}, opts64);
    if (p.n == 0) return {f, out};  // no launch
    c10::DeviceGuard guard(xs.device());
    const CellOrder o = torus_cell_order(p, q.cells);
    const at::Tensor xr = real_rows(xs, true, p.n, 3, o.order);
    at::Tensor ws = byte_buffer(ws_bytes, xs);
    check_rc(nfft_hip_ewald_lj_step_near(&q, alpha_dispersion, o.pos.data_ptr<float>(), xr.data_ptr<float>(),
                                         o.start.data_ptr<int32_t>(), o.order.data_ptr<int64_t>(), f.data_ptr<float>(),
                                         out.data_ptr<double>(), ws.data_ptr(), ws_bytes, stream_of(xs)));
    return {f, out};
}

// (spectra, eight): spectra [B, N, N, N, 6] complex64 = 2 pi i kappa_a times (b^C band[.., 0], b^D band[.., 1]), whose forward
// transform is the far part of (E, G), and eight [B, 8] float64 as above from the same read of band [B, N, N, N, 2], the
// adjoint transform of (q, c).  A band that is not contiguous is copied; a contiguous view keeps its alignment.
std::tuple<at::Tensor, at::Tensor> nfft_ewald_lj_step_spectral(at::Tensor band, at::Tensor coeffs_coulomb,
                                                               at::Tensor coeffs_dispersion, at::Tensor strain_dispersion,
                                                               std::vector<double> box, double alpha_coulomb)
{
    TORCH_CHECK(band.is_cuda(), "torch_nfft._nfft_ewald_lj_step_spectral is currently only implemented for GPU tensors");
    CHECK_INPUT(alpha_coulomb > 0.0);
    CHECK_INPUT(band.scalar_type() == at::kComplexFloat && band.dim() == 5 && band.size(4) == 2);
    CHECK_INPUT(box.size() == 6);
    const int64_t B = band.size(0), N = band.size(1);
    CHECK_INPUT(band.size(2) == N && band.size(3) == N);
    at::Tensor tables[3] = {coeffs_coulomb, coeffs_dispersion, strain_dispersion};
    for (at::Tensor &t : tables) {
        CHECK_INPUT(t.scalar_type() == at::kFloat && t.device() == band.device() && t.dim() == 3);
        for (int64_t d = 0; d < 3; ++d) CHECK_INPUT(t.size(d) == N);
        t = t.contiguous();
    }
    const at::TensorOptions opts64 = band.options().dtype(at::kDouble);
    at::Tensor out = at::zeros({B, 8}, opts64);
    if (B == 0) return {at::zeros({B, N, N, N, 6}, band.options()), out};
    const double a00 = box[0], a10 = box[1], a11 = box[2], a20 = box[3], a21 = box[4], a22 = box[5];
    CHECK_INPUT(a00 > 0.0 && a11 > 0.0 && a22 > 0.0);
    const double i00 = 1.0 / a00, i11 = 1.0 / a11, i22 = 1.0 / a22;
    const double inv[6] = {i00, -a10 * i00 * i11, i11, (a10 * a21 - a11 * a20) * i00 * i11 * i22, -a21 * i11 * i22, i22};
    const double pi = 3.14159265358979323846;
    const int64_t ws_bytes = nfft_hip_ewald_lj_step_spectral_workspace_bytes(N, B);
    if (ws_bytes < 0) check_rc(NFFT_HIP_EINVAL);
    c10::DeviceGuard guard(band.device());
    const at::Tensor bc = band.contiguous();
    at::Tensor spectra = at::empty({B, N, N, N, 6}, band.options());  // (every entry is written)
    at::Tensor ws = byte_buffer(ws_bytes, band);
    check_rc(nfft_hip_ewald_lj_step_spectral(N, B, bc.data_ptr(), tables[0].data_ptr<float>(), tables[1].data_ptr<float>(),
                                             tables[2].data_ptr<float>(), inv, pi * pi / (alpha_coulomb * alpha_coulomb),
                                             spectra.data_ptr(), out.data_ptr<double>(), ws.data_ptr(), ws_bytes, stream_of(band)));
    return {spectra, out};
}

// ---- virial tensor of the dispersion Ewald sum (not in the reference) ---------------------------
// [B, 7, *cols] float64 as the two operators above, for U = 1/2 sum_i c_i psi_i of the periodic 1/r^6: the pair part with the
// weights of nfft_ewald_dispersion_near_box (w and mg = -w'(r) / r in place of erfc(alpha r) / r and -g) ...
at::Tensor nfft_ewald_dispersion_virial_near(at::Tensor pos, at::Tensor x, c10::optional<at::Tensor> opt_batch,
                                             std::vector<double> box, double alpha, double r_cut)
{
    TORCH_CHECK(x.is_cuda(), "torch_nfft._nfft_ewald_dispersion_virial_near is currently only implemented for GPU tensors");
    return virial_near_op(nfft_hip_ewald_dispersion_virial_near, pos, x, opt_batch, box, alpha, r_cut);
}

// ... and the far part 1/2 sum_k |band_k|^2 (b_k, b_k delta_ab + t_k kappa_a kappa_b) from the splitting's coeffs (b_k) and
// strain_coeffs (t_k), both [N, N, N] float32
at::Tensor nfft_ewald_dispersion_virial_far(at::Tensor band, at::Tensor coeffs, at::Tensor strain_coeffs, std::vector<double> box)
{
    TORCH_CHECK(band.is_cuda(), "torch_nfft._nfft_ewald_dispersion_virial_far is currently only implemented for GPU tensors");
    CHECK_INPUT(strain_coeffs.scalar_type() == at::kFloat);
    CHECK_INPUT(strain_coeffs.device() == band.device());
    CHECK_INPUT(strain_coeffs.sizes() == coeffs.sizes());
    const at::Tensor tc = strain_coeffs.contiguous();
    return virial_far_op(band, coeffs, box, [&](int64_t N, int64_t B, int64_t C, const void *b, const float *c, const double *inv,
                                                double *out, void *ws, int64_t ws_bytes, void *stream) {
        return nfft_hip_ewald_dispersion_virial_far(N, B, C, b, c, tc.data_ptr<float>(), inv, out, ws, ws_bytes, stream);
    });
}

// ---- Ewald sums of packed sources: charges with point dipoles (section 7l), Stokeslets (section 7m), spheres (section 7n) --
// What tells them apart: the stem of the operators' names, the rows of a packed source, the sums per column at order 1 and 2
// and the entry points, which the operators pass beside it (the near ones share a signature and so do the spectral ones; the
// sum over spheres has a radius more and binds it in a closure).
struct PackedSum {
    const char *stem;  // the operators are stem + "_near" and stem + "_spectral"
    int64_t rows, sums[2];
};

const PackedSum kDipoleSum = {"_nfft_ewald_dipole", 4, {4, 10}};
const PackedSum kStokesletSum = {"_nfft_ewald_stokeslet", 3, {3, 12}};
const PackedSum kRpySum = {"_nfft_ewald_rpy", 3, {3, 12}};

// [n, sums, *cols] float32: the pair sums of the packed sources xs [n, rows, *cols] over the pairs within r_cut.  An empty box:
// the unit torus, pos taken modulo 1; six numbers: the box A of nfft_ewald_near_box, pos FRACTIONAL, vectors Cartesian.
// near and near_box: the two entry points, called with the arguments of nfft_hip_ewald_dipole_near / _near_box.
template <typename Near, typename NearBox>
at::Tensor packed_near(const PackedSum &k, Near near, NearBox near_box, at::Tensor pos, at::Tensor xs,
                       c10::optional<at::Tensor> opt_batch, std::vector<double> box, double alpha, double r_cut, int64_t order)
{
    TORCH_CHECK(xs.is_cuda(), "torch_nfft.", k.stem, "_near is currently only implemented for GPU tensors");
    const Points p = check_points(pos, opt_batch, "batch");
    CHECK_INPUT(p.dim == 3);
    CHECK_INPUT(xs.scalar_type() == at::kFloat);
    const Coeffs cx = check_spatial(xs, p.n, 2);
    CHECK_INPUT(xs.size(1) == k.rows);
    CHECK_INPUT(xs.device() == pos.device());
    CHECK_INPUT(box.empty() || box.size() == 6);
    CHECK_INPUT(order == 1 || order == 2);
    const int64_t sums = k.sums[order - 1], C = cx.C;
    const std::vector<int64_t> shape = cx.shape({p.n, sums});
    nfft_hip_ewald_problem qc;
    nfft_hip_ewald_box_problem qb;
    int32_t cells[3];
    int64_t ws_bytes;
    if (box.empty()) {
        qc.with_field = 1;
        qc.num_points = p.n;
        qc.num_columns = C;
        qc.batch_size = p.B;
        qc.alpha = alpha;
        qc.r_cut = r_cut;
        const int64_t G = nfft_hip_ewald_near_cells(r_cut, qc.batch_size);
        if (G < 0) check_rc(NFFT_HIP_EINVAL);
        qc.cells_per_axis = cells[0] = cells[1] = cells[2] = (int32_t)G;
        ws_bytes = nfft_hip_ewald_near_workspace_bytes(&qc);
    } else {
        qb = ewald_box_problem(p, C, true, box, alpha, r_cut);
        for (int a = 0; a < 3; ++a) cells[a] = qb.cells[a];
        ws_bytes = nfft_hip_ewald_near_box_workspace_bytes(&qb);
    }
    if (ws_bytes < 0) check_rc(NFFT_HIP_EINVAL);
    if (p.n == 0 || C == 0) return at::zeros(shape, xs.options());  // no launch
    c10::DeviceGuard guard(xs.device());
    const CellOrder o = torus_cell_order(p, cells);
    const at::Tensor xr = real_rows(xs, true, p.n, k.rows * C, o.order);
    // (zeros: a point whose coordinates are not numbers has no cell and is not written)
    at::Tensor out = at::zeros({p.n, sums * C}, xs.options());
    at::Tensor ws = byte_buffer(ws_bytes, xs);
    if (box.empty())
        check_rc(near(&qc, o.pos.data_ptr<float>(), xr.data_ptr<float>(), o.start.data_ptr<int32_t>(), o.order.data_ptr<int64_t>(),
                      (int32_t)order, out.data_ptr<float>(), ws.data_ptr(), ws_bytes, stream_of(xs)));
    else
        check_rc(near_box(&qb, o.pos.data_ptr<float>(), xr.data_ptr<float>(), o.start.data_ptr<int32_t>(),
                          o.order.data_ptr<int64_t>(), (int32_t)order, out.data_ptr<float>(), ws.data_ptr(), ws_bytes,
                          stream_of(xs)));
    return out.reshape(shape);
}

// [B, N, N, N, sums, *cols] complex64: the spectra of the far part from band [B, N, N, N, rows, *cols] complex64 (nfft_adjoint of
// the packed sources) and a coefficient grid [N, N, N] float32; kappa = A^-1 k is formed in the kernel from box (empty: the
// unit cube) and the index; spectral: the entry point
at::Tensor packed_spectral(const PackedSum &k, decltype(&nfft_hip_ewald_dipole_spectral) spectral, at::Tensor band,
                           at::Tensor coeffs, std::vector<double> box, int64_t order)
{
    TORCH_CHECK(band.is_cuda(), "torch_nfft.", k.stem, "_spectral is currently only implemented for GPU tensors");
    CHECK_INPUT(band.scalar_type() == at::kComplexFloat);
    CHECK_INPUT(coeffs.scalar_type() == at::kFloat);
    CHECK_INPUT(coeffs.device() == band.device());
    CHECK_INPUT(box.empty() || box.size() == 6);
    CHECK_INPUT(order == 1 || order == 2);
    CHECK_INPUT(band.dim() >= 5 && coeffs.dim() == 3);
    const int64_t B = band.size(0), N = band.size(1);
    for (int64_t d = 0; d < 3; ++d) CHECK_INPUT(band.size(1 + d) == N && coeffs.size(d) == N);
    CHECK_INPUT(band.size(4) == k.rows);
    int64_t C = 1;
    std::vector<int64_t> shape{B, N, N, N, k.sums[order - 1]};
    for (int64_t d = 5; d < band.dim(); ++d) {
        C *= band.size(d);
        shape.push_back(band.size(d));
    }
    double inv[6] = {1.0, 0.0, 1.0, 0.0, 0.0, 1.0};
    if (!box.empty()) {
        const double a00 = box[0], a10 = box[1], a11 = box[2], a20 = box[3], a21 = box[4], a22 = box[5];
        CHECK_INPUT(a00 > 0.0 && a11 > 0.0 && a22 > 0.0);
        const double i00 = 1.0 / a00, i11 = 1.0 / a11, i22 = 1.0 / a22;
        const double lower[6] = {i00, -a10 * i00 * i11, i11, (a10 * a21 - a11 * a20) * i00 * i11 * i22, -a21 * i11 * i22, i22};
        for (int e = 0; e < 6; ++e) inv[e] = lower[e];
    }
    if (B == 0 || C == 0) return at::zeros(shape, band.options());  // no launch
    c10::DeviceGuard guard(band.device());
    const at::Tensor bc = band.contiguous(), cc = coeffs.contiguous();
    at::Tensor out = at::empty(shape, band.options());
    check_rc(spectral(N, B, C, (int32_t)order, bc.data_ptr(), cc.data_ptr<float>(), inv, out.data_ptr(), stream_of(band)));
    return out;
}

// the Ewald sum of charges and point dipoles (not in the reference): xs [n, 4, *cols] = (q, mu); the sums
// are (phi, E) and, at order 2, the six entries xx, yy, zz, yz, xz, xy of T = grad E, with the Smith functions of alpha
at::Tensor nfft_ewald_dipole_near(at::Tensor pos, at::Tensor xs, c10::optional<at::Tensor> batch, std::vector<double> box,
                                  double alpha, double r_cut, int64_t order)
{
    return packed_near(kDipoleSum, nfft_hip_ewald_dipole_near, nfft_hip_ewald_dipole_near_box, pos, xs, batch, box, alpha, r_cut,
                       order);
}

at::Tensor nfft_ewald_dipole_spectral(at::Tensor band, at::Tensor coeffs, std::vector<double> box, int64_t order)
{
    return packed_spectral(kDipoleSum, nfft_hip_ewald_dipole_spectral, band, coeffs, box, order);
}

// the periodic Stokeslet sum (not in the reference): f [n, 3, *cols] Cartesian forces; the sums are u and,
// at order 2, the nine entries of G = grad u, row-major (G_ab = d u_a / d x_b)
at::Tensor nfft_ewald_stokeslet_near(at::Tensor pos, at::Tensor f, c10::optional<at::Tensor> batch, std::vector<double> box,
                                     double alpha, double r_cut, int64_t order)
{
    return packed_near(kStokesletSum, nfft_hip_ewald_stokeslet_near, nfft_hip_ewald_stokeslet_near_box, pos, f, batch, box, alpha,
                       r_cut, order);
}

at::Tensor nfft_ewald_stokeslet_spectral(at::Tensor band, at::Tensor coeffs, std::vector<double> box, int64_t order)
{
    return packed_spectral(kStokesletSum, nfft_hip_ewald_stokeslet_spectral, band, coeffs, box, order);
}

// the periodic Rotne-Prager-Yamakawa sum (not in the reference): f [n, 3, *cols] Cartesian forces on spheres
// of one radius; the sums are those of the Stokeslet sweep.  The far part is nfft_ewald_stokeslet_spectral with another table.
at::Tensor nfft_ewald_rpy_near(at::Tensor pos, at::Tensor f, c10::optional<at::Tensor> batch, std::vector<double> box, double alpha,
                               double r_cut, double radius, int64_t order)
{
    const auto near = [radius](const nfft_hip_ewald_problem *p, const float *points, const float *xs, const int32_t *start,
                               const int64_t *index, int32_t o, float *out, void *ws, int64_t ws_bytes, void *stream) {
        return nfft_hip_ewald_rpy_near(p, points, xs, start, index, o, radius, out, ws, ws_bytes, stream);
    };
    const auto near_box = [radius](const nfft_hip_ewald_box_problem *p, const float *points, const float *xs, const int32_t *start,
                                   const int64_t *index, int32_t o, float *out, void *ws, int64_t ws_bytes, void *stream) {
        return nfft_hip_ewald_rpy_near_box(p, points, xs, start, index, o, radius, out, ws, ws_bytes, stream);
    };
    return packed_near(kRpySum, near, near_box, pos, f, batch, box, alpha, r_cut, order);
}

// ---- Ewald sum of the screened Coulomb potential e^(-lambda r) / r (not in the reference) -------------
// (z, f) as nfft_ewald_near (an empty box: the unit torus) and nfft_ewald_near_box (six numbers) with the pair weights of
// nfft_hip_ewald_yukawa_near, lambda = screening: z[i] = sum_j w(r_ij) x[j], f[i, a] = sum_j (-w'(r_ij) / r_ij) d_ij[a] x[j]
std::tuple<at::Tensor, at::Tensor> nfft_ewald_yukawa_near(at::Tensor pos, at::Tensor x, c10::optional<at::Tensor> opt_batch,
                                                          std::vector<double> box, double alpha, double r_cut, double screening,
                                                          bool with_field)
{
    TORCH_CHECK(x.is_cuda(), "torch_nfft._nfft_ewald_yukawa_near is currently only implemented for GPU tensors");
    CHECK_INPUT(box.empty() || box.size() == 6);
    if (box.empty()) {
        const auto sweep = [screening](const nfft_hip_ewald_problem *p, const float *points, const float *xr, const int32_t *start,
                                       const int64_t *index, float *z, float *f, void *ws, int64_t ws_bytes, void *stream) {
            return nfft_hip_ewald_yukawa_near(p, points, xr, start, index, screening, z, f, ws, ws_bytes, stream);
        };
        return ewald_near_op(sweep, pos, x, opt_batch, alpha, r_cut, with_field);
    }
    const auto sweep = [screening](const nfft_hip_ewald_box_problem *p, const float *points, const float *xr, const int32_t *start,
                                   const int64_t *index, float *z, float *f, void *ws, int64_t ws_bytes, void *stream) {
        return nfft_hip_ewald_yukawa_near_box(p, points, xr, start, index, screening, z, f, ws, ws_bytes, stream);
    };
    return ewald_near_box_op(sweep, pos, x, opt_batch, box, alpha, r_cut, with_field);
}

// [B, 7, *cols] float64 as nfft_ewald_virial_near with the same pair weights (w and mg = -w'(r) / r); the far part is
// nfft_ewald_dispersion_virial_far with the splitting's two grids
at::Tensor nfft_ewald_yukawa_virial_near(at::Tensor pos, at::Tensor x, c10::optional<at::Tensor> opt_batch, std::vector<double> box,
                                         double alpha, double r_cut, double screening)
{
    TORCH_CHECK(x.is_cuda(), "torch_nfft._nfft_ewald_yukawa_virial_near is currently only implemented for GPU tensors");
    const auto reduce = [screening](const nfft_hip_ewald_box_problem *p, const float *points, const float *xr, const int32_t *start,
                                    double *out, void *ws, int64_t ws_bytes, void *stream) {
        return nfft_hip_ewald_yukawa_virial_near(p, points, xr, start, screening, out, ws, ws_bytes, stream);
    };
    return virial_near_op(reduce, pos, x, opt_batch, box, alpha, r_cut);
}

// ---- bonded-pair exclusions of the Coulomb and dispersion Ewald sums (not in the reference) ------
// The list's CSR arrays as the native calls take them, checked against the points
struct ExclInput { at::Tensor row_start, col, weight; };
ExclInput check_excl(const at::Tensor &row_start, const at::Tensor &col, const at::Tensor &weight, const at::Tensor &pos, int64_t n)
{
    CHECK_INPUT(row_start.scalar_type() == at::kInt && col.scalar_type() == at::kInt && weight.scalar_type() == at::kFloat);
    CHECK_INPUT(row_start.dim() == 1 && col.dim() == 1 && weight.dim() == 1);
    CHECK_INPUT(row_start.numel() == n + 1 && weight.numel() == col.numel());
    CHECK_INPUT(row_start.device() == pos.device() && col.device() == pos.device() && weight.device() == pos.device());
    return {row_start.contiguous(), col.contiguous(), weight.contiguous()};
}

nfft_hip_ewald_excl_problem excl_problem(const Points &p, int64_t Cr, int64_t entries, const std::vector<double> &box, double alpha,
                                         int64_t kind, bool with_field)
{
    CHECK_INPUT(box.empty() || box.size() == 6);
    CHECK_INPUT(kind == NFFT_HIP_EXCL_COULOMB || kind == NFFT_HIP_EXCL_DISPERSION);
    static const double unit[6] = {1.0, 0.0, 1.0, 0.0, 0.0, 1.0};
    nfft_hip_ewald_excl_problem q;
    q.kind = (int32_t)kind;
    q.with_field = with_field ? 1 : 0;
    q.num_points = p.n;
    q.num_columns = Cr;
    q.num_entries = entries;
    q.batch_size = p.B;
    q.alpha = alpha;
    for (int e = 0; e < 6; ++e) q.box[e] = box.empty() ? unit[e] : box[e];
    return q;
}

// x's rows [n, row] float32 in the caller's order (complex values: real and imaginary parts as columns)
at::Tensor real_rows_in_place(const at::Tensor &x, bool real_input, int64_t n, int64_t row)
{
    const at::Tensor xc = x.contiguous();
    return (real_input ? xc : at::view_as_real(xc)).reshape({n, row}).contiguous();
}

// (z, f): what the listed pairs take out of (phi, E) of the Coulomb sum (kind 0) or (psi, G) of the dispersion sum (kind 1),
// z[i] = sum_{k in row i} weight[k] K0(r) x[col[k]] and f[i, a] = sum_k weight[k] K1(r) d[a] x[col[k]], x's type and shapes
// as for nfft_ewald_near.  box: no numbers for the unit torus, six for the box of nfft_ewald_near_box (pos FRACTIONAL).  The
// positions are reduced with torus_reduce, as the sweeps' cell order reduces them: the image carries the same bits.
std::tuple<at::Tensor, at::Tensor> nfft_ewald_excl(at::Tensor pos, at::Tensor x, c10::optional<at::Tensor> opt_batch,
                                                   at::Tensor row_start, at::Tensor col, at::Tensor weight,
                                                   std::vector<double> box, double alpha, int64_t kind, bool with_field)
{
    TORCH_CHECK(x.is_cuda(), "torch_nfft._nfft_ewald_excl is currently only implemented for GPU tensors");
    const EwaldInput in = check_ewald(pos, x, opt_batch, with_field);
    const Points &p = in.p;
    const ExclInput ex = check_excl(row_start, col, weight, pos, p.n);
    const nfft_hip_ewald_excl_problem q = excl_problem(p, in.cx.Cr(), ex.col.numel(), box, alpha, kind, with_field);
    if (p.n == 0 || in.cx.C == 0 || q.num_entries == 0)
        return {at::zeros(in.z_shape, x.options()), at::zeros(in.f_shape, x.options())};  // no launch
    c10::DeviceGuard guard(x.device());
    const at::Tensor red = torus_reduce(p.pos).contiguous();
    const at::Tensor xr = real_rows_in_place(x, in.cx.real_input, p.n, q.num_columns);
    const at::TensorOptions opts = x.options().dtype(at::kFloat);
    at::Tensor z = at::empty({p.n, q.num_columns}, opts);
    at::Tensor f = with_field ? at::empty({p.n, 3 * q.num_columns}, opts) : at::empty({0}, x.options());
    check_rc((box.empty() ? nfft_hip_ewald_excl : nfft_hip_ewald_excl_box)(
        &q, red.data_ptr<float>(), xr.data_ptr<float>(), ex.row_start.data_ptr<int32_t>(), ex.col.data_ptr<int32_t>(),
        ex.weight.data_ptr<float>(), z.data_ptr<float>(), with_field ? f.data_ptr<float>() : nullptr, stream_of(x)));
    return ewald_result(in, z, f, with_field);
}

// [B, 7, *cols] float64: the listed pairs' share of nfft_ewald_virial_near (kind 0) or nfft_ewald_dispersion_virial_near
// (kind 1), each pair once, in their order; real x only; box: six numbers (the unit cube: 1, 0, 1, 0, 0, 1), pos FRACTIONAL
at::Tensor nfft_ewald_excl_virial(at::Tensor pos, at::Tensor x, c10::optional<at::Tensor> opt_batch, at::Tensor row_start,
                                  at::Tensor col, at::Tensor weight, std::vector<double> box, double alpha, int64_t kind)
{
    TORCH_CHECK(x.is_cuda(), "torch_nfft._nfft_ewald_excl_virial is currently only implemented for GPU tensors");
    const EwaldInput in = check_ewald(pos, x, opt_batch, false);
    const Points &p = in.p;
    CHECK_INPUT(box.size() == 6);
    CHECK_INPUT(in.cx.real_input);  // (the energy is bilinear: real values only)
    const ExclInput ex = check_excl(row_start, col, weight, pos, p.n);
    const int64_t C = in.cx.C;
    const std::vector<int64_t> shape = in.cx.shape({p.B, 7});
    const nfft_hip_ewald_excl_problem q = excl_problem(p, C, ex.col.numel(), box, alpha, kind, false);
    const int64_t ws_bytes = nfft_hip_ewald_excl_virial_workspace_bytes(&q);
    if (ws_bytes < 0) check_rc(NFFT_HIP_EINVAL);
    const at::TensorOptions opts = x.options().dtype(at::kDouble);
    if (p.n == 0 || C == 0 || q.num_entries == 0) return at::zeros(shape, opts);  // no launch
    c10::DeviceGuard guard(x.device());
    const at::Tensor red = torus_reduce(p.pos).contiguous();
    const at::Tensor xr = real_rows_in_place(x, true, p.n, C);
    at::Tensor set_start;
    if (p.batch.defined())
        set_start = at::searchsorted(p.batch, at::arange(p.B + 1, p.batch.options()), /*out_int32=*/true).contiguous();
    at::Tensor out = at::empty({p.B, 7, C}, opts);
    at::Tensor ws = byte_buffer(ws_bytes, x);
    check_rc(nfft_hip_ewald_excl_virial(&q, red.data_ptr<float>(), xr.data_ptr<float>(), ex.row_start.data_ptr<int32_t>(),
                                        ex.col.data_ptr<int32_t>(), ex.weight.data_ptr<float>(),
                                        set_start.defined() ? set_start.data_ptr<int32_t>() : nullptr, out.data_ptr<double>(),
                                        ws.data_ptr(), ws_bytes, stream_of(x)));
    return out.reshape(shape);
}

// ---- bonded-pair exclusions of the Lennard-Jones + Coulomb step (not in the reference) ----------
struct LjExclInput {
    Points p;
    ExclInput ex;
    at::Tensor wl;
    nfft_hip_ewald_box_problem q;
};
LjExclInput check_lj_excl(const at::Tensor &pos, const at::Tensor &xs, const c10::optional<at::Tensor> &opt_batch,
                          const at::Tensor &row_start, const at::Tensor &col, const at::Tensor &weight_coulomb,
                          const at::Tensor &weight_lj, const std::vector<double> &box, double alpha_coulomb, double r_cut)
{
    const Points p = check_points(pos, opt_batch, "batch");
    CHECK_INPUT(p.dim == 3);
    CHECK_INPUT(xs.scalar_type() == at::kFloat && xs.dim() == 2 && xs.size(0) == p.n && xs.size(1) == 3);
    CHECK_INPUT(xs.device() == pos.device());
    CHECK_INPUT(box.size() == 6);
    const ExclInput ex = check_excl(row_start, col, weight_coulomb, pos, p.n);
    CHECK_INPUT(weight_lj.scalar_type() == at::kFloat && weight_lj.dim() == 1 && weight_lj.numel() == ex.col.numel());
    CHECK_INPUT(weight_lj.device() == pos.device());
    return {p, ex, weight_lj.contiguous(), ewald_box_problem(p, 1, true, box, alpha_coulomb, r_cut)};
}

// (f, eight) of nfft_ewald_lj_step_near with the terms of the listed pairs scaled by 1 - weight before they are added: the
// list is ExclusionList's CSR matrix over the points in the caller's order with the two weights 1 - s^C and 1 - s^L
std::tuple<at::Tensor, at::Tensor> nfft_ewald_lj_excl_near(at::Tensor pos, at::Tensor xs, c10::optional<at::Tensor> opt_batch,
                                                           at::Tensor row_start, at::Tensor col, at::Tensor weight_coulomb,
                                                           at::Tensor weight_lj, std::vector<double> box, double alpha_coulomb,
                                                           double alpha_dispersion, double r_cut)
{
    TORCH_CHECK(xs.is_cuda(), "torch_nfft._nfft_ewald_lj_excl_near is currently only implemented for GPU tensors");
    const LjExclInput in = check_lj_excl(pos, xs, opt_batch, row_start, col, weight_coulomb, weight_lj, box, alpha_coulomb, r_cut);
    const Points &p = in.p;
    const int64_t ws_bytes = nfft_hip_ewald_lj_excl_near_workspace_bytes(&in.q, alpha_dispersion);
    if (ws_bytes < 0) check_rc(NFFT_HIP_EINVAL);
    // (zeros: a point whose coordinates are not numbers has no cell and is not written)
    at::Tensor f = at::zeros({p.n, 3}, xs.options());
    at::Tensor out = at::zeros({p.B, 8}, xs.options().dtype(at::kDouble));
    if (p.n == 0) return {f, out};  // no launch
    c10::DeviceGuard guard(xs.device());
    const CellOrder o = torus_cell_order(p, in.q.cells);
    const at::Tensor xr = real_rows(xs, true, p.n, 3, o.order);
    at::Tensor ws = byte_buffer(ws_bytes, xs);
    const bool any = in.ex.col.numel() > 0;
    check_rc(nfft_hip_ewald_lj_excl_near(&in.q, alpha_dispersion, in.ex.col.numel(), o.pos.data_ptr<float>(), xr.data_ptr<float>(),
                                         o.start.data_ptr<int32_t>(), o.order.data_ptr<int64_t>(),
                                         in.ex.row_start.data_ptr<int32_t>(), any ? in.ex.col.data_ptr<int32_t>() : nullptr,
                                         any ? in.ex.weight.data_ptr<float>() : nullptr, any ? in.wl.data_ptr<float>() : nullptr,
                                         f.data_ptr<float>(), out.data_ptr<double>(), ws.data_ptr(), ws_bytes, stream_of(xs)));
    return {f, out};
}

// (f, eight) to ADD to those of nfft_ewald_lj_excl_near: minus the listed pairs' smooth share (r < r_cut) or their whole
// Coulomb and dispersion terms (r >= r_cut), on the positions reduced with torus_reduce as the walk's cell order reduces them
std::tuple<at::Tensor, at::Tensor> nfft_ewald_lj_excl_list(at::Tensor pos, at::Tensor xs, c10::optional<at::Tensor> opt_batch,
                                                           at::Tensor row_start, at::Tensor col, at::Tensor weight_coulomb,
                                                           at::Tensor weight_lj, std::vector<double> box, double alpha_coulomb,
                                                           double alpha_dispersion, double r_cut)
{
    TORCH_CHECK(xs.is_cuda(), "torch_nfft._nfft_ewald_lj_excl_list is currently only implemented for GPU tensors");
    const LjExclInput in = check_lj_excl(pos, xs, opt_batch, row_start, col, weight_coulomb, weight_lj, box, alpha_coulomb, r_cut);
    const Points &p = in.p;
    const int64_t ws_bytes = nfft_hip_ewald_lj_excl_list_workspace_bytes(&in.q, alpha_dispersion);
    if (ws_bytes < 0) check_rc(NFFT_HIP_EINVAL);
    at::Tensor f = at::zeros({p.n, 3}, xs.options());
    at::Tensor out = at::zeros({p.B, 8}, xs.options().dtype(at::kDouble));
    if (p.n == 0 || in.ex.col.numel() == 0) return {f, out};  // no launch
    c10::DeviceGuard guard(xs.device());
    const at::Tensor red = torus_reduce(p.pos).contiguous();
    const at::Tensor xr = xs.contiguous();
    at::Tensor set_start;
    if (p.batch.defined())
        set_start = at::searchsorted(p.batch, at::arange(p.B + 1, p.batch.options()), /*out_int32=*/true).contiguous();
    at::Tensor ws = byte_buffer(ws_bytes, xs);
    check_rc(nfft_hip_ewald_lj_excl_list(&in.q, alpha_dispersion, in.ex.col.numel(), red.data_ptr<float>(), xr.data_ptr<float>(),
                                         in.ex.row_start.data_ptr<int32_t>(), in.ex.col.data_ptr<int32_t>(),
                                         in.ex.weight.data_ptr<float>(), in.wl.data_ptr<float>(),
                                         set_start.defined() ? set_start.data_ptr<int32_t>() : nullptr, f.data_ptr<float>(),
                                         out.data_ptr<double>(), ws.data_ptr(), ws_bytes, stream_of(xs)));
    return {f, out};
}

// ---- the pair walks with a type-pair table (not in the reference; DESIGN.md sections 7t and 7u) ---------------------------
typedef int table_near_entry(const nfft_hip_ewald_box_problem *, double, int64_t, int64_t, const float *, const float *,
                             const int32_t *, const float *, const int32_t *, const int64_t *, const int32_t *, const int32_t *,
                             const float *, const float *, float *, double *, void *, int64_t, void *);

// (f, eight) of `entry` for xs [n, 2] = (q, c), types [n] int32 and table [T, T, width] float32.  The four list tensors are
// ExclusionList's, all given or none: with them the listed pairs' terms are scaled as by nfft_ewald_lj_excl_near.  realign:
// the bytes to which a table that is a view into a larger tensor is cloned (1: taken as it comes)
std::tuple<at::Tensor, at::Tensor> ewald_table_near(const char *name, int64_t width, uintptr_t realign, table_near_entry *entry,
                                                    const at::Tensor &pos, const at::Tensor &xs, const at::Tensor &types,
                                                    const at::Tensor &table, const c10::optional<at::Tensor> &opt_batch,
                                                    const c10::optional<at::Tensor> &row_start, const c10::optional<at::Tensor> &col,
                                                    const c10::optional<at::Tensor> &weight_coulomb,
                                                    const c10::optional<at::Tensor> &weight_lj, const std::vector<double> &box,
                                                    double alpha_coulomb, double alpha_dispersion, double r_cut)
{
    TORCH_CHECK(xs.is_cuda(), "torch_nfft.", name, " is currently only implemented for GPU tensors");
    const Points p = check_points(pos, opt_batch, "batch");
    CHECK_INPUT(p.dim == 3);
    CHECK_INPUT(xs.scalar_type() == at::kFloat && xs.dim() == 2 && xs.size(0) == p.n && xs.size(1) == 2);
    CHECK_INPUT(types.scalar_type() == at::kInt && types.dim() == 1 && types.size(0) == p.n);
    CHECK_INPUT(table.scalar_type() == at::kFloat && table.dim() == 3 && table.size(0) == table.size(1) && table.size(2) == width);
    CHECK_INPUT(table.size(0) >= 1 && table.size(0) <= 32);
    CHECK_INPUT(xs.device() == pos.device() && types.device() == pos.device() && table.device() == pos.device());
    CHECK_INPUT(box.size() == 6);
    const bool masked = row_start.has_value();
    CHECK_INPUT(col.has_value() == masked && weight_coulomb.has_value() == masked && weight_lj.has_value() == masked);
    ExclInput ex;
    at::Tensor wl;
    if (masked) {
        ex = check_excl(*row_start, *col, *weight_coulomb, pos, p.n);
        CHECK_INPUT(weight_lj->scalar_type() == at::kFloat && weight_lj->dim() == 1 && weight_lj->numel() == ex.col.numel());
        CHECK_INPUT(weight_lj->device() == pos.device());
        wl = weight_lj->contiguous();
    }
    const nfft_hip_ewald_box_problem q = ewald_box_problem(p, 1, true, box, alpha_coulomb, r_cut);
    const int64_t ws_bytes = nfft_hip_ewald_lj_table_near_workspace_bytes(&q, alpha_dispersion);  // (one for every step walk)
    if (ws_bytes < 0) check_rc(NFFT_HIP_EINVAL);
    // (zeros: a point whose coordinates are not numbers has no cell and is not written)
    at::Tensor f = at::zeros({p.n, 3}, xs.options());
    at::Tensor out = at::zeros({p.B, 8}, xs.options().dtype(at::kDouble));
    if (p.n == 0) return {f, out};  // no launch
    c10::DeviceGuard guard(xs.device());
    const CellOrder o = torus_cell_order(p, q.cells);
    const at::Tensor xr = real_rows(xs, true, p.n, 2, o.order);
    const at::Tensor tr = types.index_select(0, o.order);
    at::Tensor tab = table.contiguous();
    if ((uintptr_t)tab.data_ptr() & (realign - 1)) tab = tab.clone();  // (an entry moves as one load)
    at::Tensor ws = byte_buffer(ws_bytes, xs);
    const int64_t entries = masked ? ex.col.numel() : 0;
    const bool any = entries > 0;
    check_rc(entry(&q, alpha_dispersion, tab.size(0), entries, o.pos.data_ptr<float>(), xr.data_ptr<float>(), tr.data_ptr<int32_t>(),
                   tab.data_ptr<float>(), o.start.data_ptr<int32_t>(), o.order.data_ptr<int64_t>(),
                   masked ? ex.row_start.data_ptr<int32_t>() : nullptr, any ? ex.col.data_ptr<int32_t>() : nullptr,
                   any ? ex.weight.data_ptr<float>() : nullptr, any ? wl.data_ptr<float>() : nullptr, f.data_ptr<float>(),
                   out.data_ptr<double>(), ws.data_ptr(), ws_bytes, stream_of(xs)));
    return {f, out};
}

// table = (C12, dC6): the pair's repulsion and what its C6 has above c_i c_j come from the table entry of the two types
std::tuple<at::Tensor, at::Tensor> nfft_ewald_lj_table_near(at::Tensor pos, at::Tensor xs, at::Tensor types, at::Tensor table,
                                                            c10::optional<at::Tensor> opt_batch,
                                                            c10::optional<at::Tensor> row_start, c10::optional<at::Tensor> col,
                                                            c10::optional<at::Tensor> weight_coulomb,
                                                            c10::optional<at::Tensor> weight_lj, std::vector<double> box,
                                                            double alpha_coulomb, double alpha_dispersion, double r_cut)
{
    return ewald_table_near("_nfft_ewald_lj_table_near", 2, 1, nfft_hip_ewald_lj_table_near, pos, xs, types, table, opt_batch,
                            row_start, col, weight_coulomb, weight_lj, box, alpha_coulomb, alpha_dispersion, r_cut);
}

// table = (A, B, dC6, C8): the pair energy of two types within r_cut is A e^(-B r) - dC6 / r^6 - C8 / r^8 beside the Ewald
// weights of (q, c); an entry moves as one 16-byte load
std::tuple<at::Tensor, at::Tensor> nfft_ewald_bmh_table_near(at::Tensor pos, at::Tensor xs, at::Tensor types, at::Tensor table,
                                                             c10::optional<at::Tensor> opt_batch,
                                                             c10::optional<at::Tensor> row_start, c10::optional<at::Tensor> col,
                                                             c10::optional<at::Tensor> weight_coulomb,
                                                             c10::optional<at::Tensor> weight_lj, std::vector<double> box,
                                                             double alpha_coulomb, double alpha_dispersion, double r_cut)
{
    return ewald_table_near("_nfft_ewald_bmh_table_near", 4, 16, nfft_hip_ewald_bmh_table_near, pos, xs, types, table, opt_batch,
                            row_start, col, weight_coulomb, weight_lj, box, alpha_coulomb, alpha_dispersion, r_cut);
}

// coefficient operators (csrc/core.cpp:124-171; drivers core_cuda.cu:855-1064): outputs live on the current device
at::TensorOptions current_device_options(at::ScalarType dtype)
{
    int dev = 0;
    TORCH_CHECK(hipGetDevice(&dev) == hipSuccess, "hipGetDevice failed");
    return at::TensorOptions().device(c10::Device(c10::kCUDA, (c10::DeviceIndex)dev)).dtype(dtype);
}

std::vector<int64_t> cube(int64_t N, int64_t dim)
{
    CHECK_INPUT(dim >= 1 && dim <= 3 && N >= 2);
    return std::vector<int64_t>((size_t)dim, N);
}

at::Tensor coeffs_workspace(int64_t N, int64_t dim, const at::Tensor &like, int64_t &nbytes)
{
    nbytes = nfft_hip_coeffs_workspace_bytes(N, (int32_t)dim);
    return workspace_or_raise(nbytes, like);
}

at::Tensor gaussian_analytic_coeffs(double sigma, int64_t N, int64_t dim)
{
    at::Tensor out = at::empty(cube(N, dim), current_device_options(at::kFloat));
    check_rc(nfft_hip_gaussian_analytic_coeffs(sigma, N, (int32_t)dim, out.data_ptr<float>(), stream_of(out)));
    return out;
}

at::Tensor gaussian_interpolated_coeffs(double sigma, int64_t N, int64_t dim, int64_t p, double eps)
{
    TORCH_CHECK(p <= 0, "Gaussian interpolated coeffs are currently only implemented for p<=0");    // core_cuda.cu:890
    TORCH_CHECK(eps == 0.0, "Gaussian interpolated coeffs are currently only implemented for eps=0");  // :891
    at::Tensor out = at::empty(cube(N, dim), current_device_options(at::kComplexFloat));
    int64_t nbytes = 0;
    at::Tensor ws = coeffs_workspace(N, dim, out, nbytes);
    check_rc(nfft_hip_gaussian_interpolated_coeffs(sigma, N, (int32_t)dim, p, eps, out.data_ptr(), ws.data_ptr(), nbytes,
                                                   stream_of(out)));
    return out;
}

at::Tensor interpolation_grid(int64_t N, int64_t dim)
{
    std::vector<int64_t> shape = cube(N, dim);
    shape.push_back(dim);
    at::Tensor out = at::empty(shape, current_device_options(at::kFloat));
    check_rc(nfft_hip_interpolation_grid(N, (int32_t)dim, 0, out.data_ptr<float>(), stream_of(out)));
    return out;
}

at::Tensor radial_interpolation_grid(int64_t N, int64_t dim)
{
    at::Tensor out = at::empty(cube(N, dim), current_device_options(at::kFloat));
    check_rc(nfft_hip_interpolation_grid(N, (int32_t)dim, 1, out.data_ptr<float>(), stream_of(out)));
    return out;
}

at::Tensor interpolated_kernel_coeffs(at::Tensor grid_values)
{
    TORCH_CHECK(grid_values.is_cuda(),
                "torch_nfft.interpolated_kernel_coeffs is currently only implemented for GPU tensors");
    const int64_t dim = grid_values.dim();
    CHECK_INPUT(dim >= 1 && dim <= 3);
    const int64_t N = grid_values.size(0);
    for (int64_t d = 1; d < dim; ++d) CHECK_INPUT(grid_values.size(d) == N);
    const bool real = real_dtype(grid_values);
    const at::Tensor vals = grid_values.contiguous();
    c10::DeviceGuard guard(vals.device());
    at::Tensor out = at::empty(cube(N, dim), vals.options().dtype(at::kComplexFloat));
    int64_t nbytes = 0;
    at::Tensor ws = coeffs_workspace(N, dim, out, nbytes);
    check_rc(nfft_hip_interpolated_kernel_coeffs(vals.data_ptr(), real ? 0 : 1, N, (int32_t)dim, out.data_ptr(),
                                                 ws.data_ptr(), nbytes, stream_of(out)));
    return out;
}

} // namespace

// Same eight schemas as the reference's RegisterOperators block (csrc/core.cpp:176-184); every caller is positional
// (torch_nfft/nfft.py:14-86, coeffs.py:11-27), so naming the arguments changes nothing for them.
TORCH_LIBRARY(torch_nfft, m)
{
    m.def("nfft_adjoint(Tensor pos, Tensor x, Tensor? batch, int N, int m, int real_output) -> Tensor", &nfft_adjoint);
    m.def("nfft_forward(Tensor pos, Tensor x, Tensor? batch, int m, int real_output) -> Tensor", &nfft_forward);
    m.def("nfft_fastsum(Tensor sources, Tensor targets, Tensor x, Tensor coeffs, Tensor? source_batch, "
          "Tensor? target_batch, int m) -> Tensor", &nfft_fastsum);
    m.def("gaussian_analytic_coeffs(float sigma, int N, int dim) -> Tensor", &gaussian_analytic_coeffs);
    m.def("gaussian_interpolated_coeffs(float sigma, int N, int dim, int p, float eps) -> Tensor",
          &gaussian_interpolated_coeffs);
    m.def("interpolation_grid(int N, int dim) -> Tensor", &interpolation_grid);
    m.def("radial_interpolation_grid(int N, int dim) -> Tensor", &radial_interpolation_grid);
    m.def("interpolated_kernel_coeffs(Tensor grid_values) -> Tensor", &interpolated_kernel_coeffs);
    // not in the reference: control of the point-plan cache (torch_nfft_amd.ops.plan_cache_*)
    m.def("_plan_cache(int action) -> int", &plan_cache_control);
    // not in the reference: device-side fault reports (torch_nfft_amd.ops.check_status)
    m.def("_check_status(int synchronize) -> int", &check_status);
    // not in the reference: gradient of nfft_forward with respect to the points (autograd of both transforms)
    m.def("_nfft_forward_grad_points(Tensor pos, Tensor x, Tensor? batch, int m, int real_output, Tensor w) -> Tensor",
          &nfft_forward_grad_points);
    // not in the reference: its backward, for second derivatives of both transforms
    m.def("_nfft_forward_grad_points_backward(Tensor pos, Tensor xhat, Tensor? batch, int m, int real_output, Tensor w, "
          "Tensor v, int need_xhat, int need_w, int need_pos) -> (Tensor, Tensor, Tensor)",
          &nfft_forward_grad_points_backward);
    // not in the reference: gradient of nfft_fastsum with respect to the points (autograd of nfft_fastsum)
    m.def("_nfft_fastsum_band(Tensor sources, Tensor targets, Tensor x, Tensor coeffs, Tensor? source_batch, "
          "Tensor? target_batch, int m) -> (Tensor, Tensor)", &nfft_fastsum_band);
    m.def("_nfft_fastsum_backward(Tensor sources, Tensor targets, Tensor x, Tensor dy, Tensor coeffs, Tensor? band, "
          "Tensor? source_batch, Tensor? target_batch, int m, int need_x, int need_sources, int need_targets) "
          "-> (Tensor, Tensor, Tensor)", &nfft_fastsum_backward);
    // not in the reference: the Toeplitz normal operator A^H W A (nfft_toeplitz_kernel / nfft_normal / nfft_inverse)
    m.def("_nfft_toeplitz_kernel(Tensor t) -> Tensor", &nfft_toeplitz_kernel);
    m.def("_nfft_normal(Tensor kernel, Tensor x) -> Tensor", &nfft_normal);
    // not in the reference: the near-field pair sum of the fast summation for singular kernels (nfft_fastsum_nearfield)
    m.def("_nfft_nearfield(Tensor sources, Tensor targets, Tensor x, Tensor? source_batch, Tensor? target_batch, "
          "int kernel, float c, float eps_I, float[] poly) -> Tensor", &nfft_nearfield);
    // ... and its gradient at the targets / the transpose of that (nfft_fastsum_nearfield_gradient)
    m.def("_nfft_nearfield_gradient(Tensor sources, Tensor targets, Tensor x, Tensor? source_batch, Tensor? target_batch, "
          "int kernel, float c, float eps_I, float[] poly, bool transpose) -> Tensor", &nfft_nearfield_gradient);
    // ... and the gradient of the near-field sum with respect to its points, contracted with dy (point_gradients=True)
    m.def("_nfft_nearfield_point_gradient(Tensor sources, Tensor targets, Tensor x, Tensor dy, Tensor? source_batch, "
          "Tensor? target_batch, int kernel, float c, float eps_I, float[] poly, bool need_sources, bool need_targets) "
          "-> (Tensor, Tensor)", &nfft_nearfield_point_gradient);
    // not in the reference: the wrapped pair sum erfc(alpha r) / r of the Ewald sum and its field (nfft_ewald)
    m.def("_nfft_ewald_near(Tensor pos, Tensor x, Tensor? batch, float alpha, float r_cut, bool with_field) "
          "-> (Tensor, Tensor)", &nfft_ewald_near);
    // not in the reference: the same pair sum in an orthorhombic or triclinic box, on fractional positions
    m.def("_nfft_ewald_near_box(Tensor pos, Tensor x, Tensor? batch, float[] box, float alpha, float r_cut, bool with_field) "
          "-> (Tensor, Tensor)", &nfft_ewald_near_box);
    // not in the reference: the wrapped pair sum of the dispersion Ewald sum 1/r^6 and its field (nfft_ewald_dispersion)
    m.def("_nfft_ewald_dispersion_near(Tensor pos, Tensor x, Tensor? batch, float alpha, float r_cut, bool with_field) "
          "-> (Tensor, Tensor)", &nfft_ewald_dispersion_near);
    m.def("_nfft_ewald_dispersion_near_box(Tensor pos, Tensor x, Tensor? batch, float[] box, float alpha, float r_cut, "
          "bool with_field) -> (Tensor, Tensor)", &nfft_ewald_dispersion_near_box);
    // not in the reference: the pair and the spectral reduction of the Ewald sum's virial tensor (nfft_ewald_virial)
    m.def("_nfft_ewald_virial_near(Tensor pos, Tensor x, Tensor? batch, float[] box, float alpha, float r_cut) -> Tensor",
          &nfft_ewald_virial_near);
    m.def("_nfft_ewald_virial_far(Tensor band, Tensor coeffs, float[] box, float alpha) -> Tensor", &nfft_ewald_virial_far);
    // not in the reference: the field sweep and the two reductions above in one pair walk and one spectral pass (nfft_ewald_step)
    m.def("_nfft_ewald_step_near(Tensor pos, Tensor x, Tensor? batch, float[] box, float alpha, float r_cut) "
          "-> (Tensor, Tensor, Tensor)", &nfft_ewald_step_near);
    m.def("_nfft_ewald_step_spectral(Tensor band, Tensor coeffs, float[] box, float alpha) -> (Tensor, Tensor)",
          &nfft_ewald_step_spectral);
    // not in the reference: Coulomb, dispersion and r^-12 repulsion in one pair walk and one spectral pass (nfft_ewald_lj_step)
    m.def("_nfft_ewald_lj_step_near(Tensor pos, Tensor xs, Tensor? batch, float[] box, float alpha_coulomb, "
          "float alpha_dispersion, float r_cut) -> (Tensor, Tensor)", &nfft_ewald_lj_step_near);
    m.def("_nfft_ewald_lj_step_spectral(Tensor band, Tensor coeffs_coulomb, Tensor coeffs_dispersion, Tensor strain_dispersion, "
          "float[] box, float alpha_coulomb) -> (Tensor, Tensor)", &nfft_ewald_lj_step_spectral);
    // not in the reference: the same two reductions for the dispersion Ewald sum 1/r^6 (nfft_ewald_dispersion_virial)
    m.def("_nfft_ewald_dispersion_virial_near(Tensor pos, Tensor x, Tensor? batch, float[] box, float alpha, float r_cut) "
          "-> Tensor", &nfft_ewald_dispersion_virial_near);
    m.def("_nfft_ewald_dispersion_virial_far(Tensor band, Tensor coeffs, Tensor strain_coeffs, float[] box) -> Tensor",
          &nfft_ewald_dispersion_virial_far);
    // not in the reference: the pair sweep and the spectral step of the Ewald sum of charges and dipoles (nfft_ewald_dipole)
    m.def("_nfft_ewald_dipole_near(Tensor pos, Tensor xs, Tensor? batch, float[] box, float alpha, float r_cut, int order) "
          "-> Tensor", &nfft_ewald_dipole_near);
    m.def("_nfft_ewald_dipole_spectral(Tensor band, Tensor coeffs, float[] box, int order) -> Tensor",
          &nfft_ewald_dipole_spectral);
    // not in the reference: the pair sweep and the spectral step of the periodic Stokeslet sum (nfft_ewald_stokeslet)
    m.def("_nfft_ewald_stokeslet_near(Tensor pos, Tensor f, Tensor? batch, float[] box, float alpha, float r_cut, int order) "
          "-> Tensor", &nfft_ewald_stokeslet_near);
    m.def("_nfft_ewald_stokeslet_spectral(Tensor band, Tensor coeffs, float[] box, int order) -> Tensor",
          &nfft_ewald_stokeslet_spectral);
    // not in the reference: the pair sweep of the periodic Rotne-Prager-Yamakawa sum (nfft_ewald_rpy)
    m.def("_nfft_ewald_rpy_near(Tensor pos, Tensor f, Tensor? batch, float[] box, float alpha, float r_cut, float radius, "
          "int order) -> Tensor", &nfft_ewald_rpy_near);
    // not in the reference: the pair sweep and the pair reduction of the screened Coulomb (Yukawa) Ewald sum (nfft_ewald_yukawa)
    m.def("_nfft_ewald_yukawa_near(Tensor pos, Tensor x, Tensor? batch, float[] box, float alpha, float r_cut, float screening, "
          "bool with_field) -> (Tensor, Tensor)", &nfft_ewald_yukawa_near);
    m.def("_nfft_ewald_yukawa_virial_near(Tensor pos, Tensor x, Tensor? batch, float[] box, float alpha, float r_cut, "
          "float screening) -> Tensor", &nfft_ewald_yukawa_virial_near);
    // not in the reference: what a list of bonded pairs takes out of the Coulomb and dispersion Ewald sums and their virials
    // not in the reference: the Lennard-Jones + Coulomb step with bonded-pair exclusions (nfft_ewald_lj_excl_step)
    m.def("_nfft_ewald_lj_excl_near(Tensor pos, Tensor xs, Tensor? batch, Tensor row_start, Tensor col, Tensor weight_coulomb, "
          "Tensor weight_lj, float[] box, float alpha_coulomb, float alpha_dispersion, float r_cut) -> (Tensor, Tensor)",
          &nfft_ewald_lj_excl_near);
    m.def("_nfft_ewald_lj_excl_list(Tensor pos, Tensor xs, Tensor? batch, Tensor row_start, Tensor col, Tensor weight_coulomb, "
          "Tensor weight_lj, float[] box, float alpha_coulomb, float alpha_dispersion, float r_cut) -> (Tensor, Tensor)",
          &nfft_ewald_lj_excl_list);
    // not in the reference: the pair walk of the same step with a type-pair table (nfft_ewald_lj_table_step)
    m.def("_nfft_ewald_lj_table_near(Tensor pos, Tensor xs, Tensor types, Tensor table, Tensor? batch, Tensor? row_start, "
          "Tensor? col, Tensor? weight_coulomb, Tensor? weight_lj, float[] box, float alpha_coulomb, float alpha_dispersion, "
          "float r_cut) -> (Tensor, Tensor)", &nfft_ewald_lj_table_near);
    // not in the reference: the pair walk of the Buckingham / Born-Mayer-Huggins step (nfft_ewald_bmh_table_step)
    m.def("_nfft_ewald_bmh_table_near(Tensor pos, Tensor xs, Tensor types, Tensor table, Tensor? batch, Tensor? row_start, "
          "Tensor? col, Tensor? weight_coulomb, Tensor? weight_lj, float[] box, float alpha_coulomb, float alpha_dispersion, "
          "float r_cut) -> (Tensor, Tensor)", &nfft_ewald_bmh_table_near);
    m.def("_nfft_ewald_excl(Tensor pos, Tensor x, Tensor? batch, Tensor row_start, Tensor col, Tensor weight, float[] box, "
          "float alpha, int kind, bool with_field) -> (Tensor, Tensor)", &nfft_ewald_excl);
    m.def("_nfft_ewald_excl_virial(Tensor pos, Tensor x, Tensor? batch, Tensor row_start, Tensor col, Tensor weight, "
          "float[] box, float alpha, int kind) -> Tensor", &nfft_ewald_excl_virial);
}
