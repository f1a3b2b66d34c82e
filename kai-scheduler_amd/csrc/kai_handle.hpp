// kai_handle.hpp — the handle behind the C ABI (struct kai_core) and what every entry point of kai_core.hip shares: the error macros, the buffers that live with the
// handle (HandleBuf), the session's slab allocator with its upload / fill helpers, the pinned staging of the snapshot's own arrays (UploadStage), the context builder's arena on them (DevArena), free_session.  First of kai_core.hip's own headers.
#pragma once
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <map>
#include <mutex>
#include <thread>

#include "kai_host_prep.hpp"
#include "kai_ctx_build.hpp"
#include "kai_kernels.hpp"
#include "kai_batch_kernels.hpp"
#include "kai_batch_driver.hpp"
#include "kai_victim_shard.hpp"
#include "kai_delta.hpp"
#include "kai_best_nodes.hpp"
#include "kai_ordered_nodes.hpp"
#include "kai_ops_apply.hpp"
#include "kai_stmt.hpp"
#include "kai_stmt_place.hpp"
#include "kai_stale_gangs.hpp"
#include "kai_job_order.hpp"
#include "kai_subset_nodes.hpp"

using namespace kai;

// A buffer of its own that lives with the handle (never part of the slab bookkeeping): pinned host memory or device memory, allocated on first use and regrown on demand.
// grow(): nothing when `need` fits; otherwise the old allocation goes and `want` bytes come (the caller's growth rule) and *grew says so: what depends on the buffer's
// content is the caller's to reset.  A failed allocation leaves the buffer empty.  kai_core::handle_bufs() lists every one of them for kai_core_destroy.
struct HandleBuf {
    const bool pinned; unsigned char* p = nullptr; size_t bytes = 0;
    explicit HandleBuf(bool pinned_) : pinned(pinned_) {}
    void release() { if (p) (void)(pinned ? hipHostFree(p) : hipFree(p)); p = nullptr; bytes = 0; }
    hipError_t grow(size_t need, size_t want, bool* grew = nullptr) {
        if (grew) *grew = need > bytes;
        if (need <= bytes) return hipSuccess;
        release();
        void* q = nullptr; const hipError_t e = pinned ? hipHostMalloc(&q, want, hipHostMallocDefault) : hipMalloc(&q, want);
        if (e == hipSuccess) { p = static_cast<unsigned char*>(q); bytes = want; } else if (grew) *grew = false;
        return e;
    }
};

struct kai_core {
    kai_config cfg{}; int device = -1; hipStream_t stream = nullptr; hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::string err = "ok"; bool open = false;
    KaiCtx ctx{};
    KaiCtx* d_ctx = nullptr;  // HBM copy of ctx for the persistent kernel
    int fast_ok0 = 0;  // the snapshot's verdict on the staged job path (restored by kai_session_reset)
    bool solver_ready = false;  // scratch of the victim search allocated (first reclaim / preempt / consolidation of the session)
    std::vector<void*> bufs; std::vector<size_t> buf_bytes;  // session HBM: a few large slabs, sub-allocated (one contiguous range ⇒ few TLB entries for the latency-bound engine)
    std::vector<std::pair<void*, size_t>> spare;  // slabs of closed sessions, reused by the next open
    bool index_stale = false;  // the last action ran on the bucket fill, which keeps the sets current but not the class index (sum1_key / sum1_node): rebuilt before the next action reads it
    HandleBuf rep_buf{false};  // the victim actions' replica memory: its own allocation (never part of the slab bookkeeping), kept between sessions while it is large enough
    HandleBuf pin_buf{true};  // pinned host staging for the operations handed to the caller (grows, lives with the handle)
    char* slab = nullptr; size_t slab_left = 0;
    size_t post_open_max = 0;  // largest slab a request made after kai_session_open needed in this session (trim rule of the next open)
    OpenAux aux;  // the open's arrays that are no part of the context (kai_ctx_build.hpp): arguments of the session-open kernels, k_drain, k_best_node
    int n_levels = 0; std::vector<int32_t> h_lvl_off; int n_heights = 0;  // fair-share levels (aux.lvl_off on the host), heights of the queue tree
    int32_t *d_status0 = nullptr, *d_node0 = nullptr; QShare* d_shares0 = nullptr;  // HBM-resident initial state for kai_session_reset
    std::vector<int32_t> perm;  // engine node index (= name rank) → caller's node index
    kai_action_stats stats{};
    HostPrep::BatchShape shape;  // batch path of the allocate action (kai_batch.hpp)
    int world = 1, rank = 0, shard_k = 0; kai_allgather_fn ag_fn = nullptr; void* ag_user = nullptr;  // node-axis sharding over the GPUs of one node (kai_shard_attach)
    void* rccl_comm = nullptr;  // the library's own communicator (kai_shard_attach_rccl): the exchange is an ncclAllGather on `stream`, no host round trip
    bool shared = false; int32_t next_group0 = 0;  // shared GPUs in the session; the first group id a cycle may open (kai_session_reset)
    hipEvent_t bev[4] = {nullptr, nullptr, nullptr, nullptr};
    // rounds without the host (kai_batch_driver.hpp): per slot the round's phase events (plan start, fill start, fill end, apply end), the event behind its RoundCtl copy, the pinned copy
    hipEvent_t rev[KB_ROUND_SLOTS][5] = {}; HandleBuf rpin{true}; bool rev_ready = false;
    double batch_plan_ms = 0, batch_fill_ms = 0, batch_apply_ms = 0;
    // victim actions on several workgroups (kai_engine_solver.inc solve_partial_multi): every array a KaiCtx field points to, so that each workgroup gets a replica
    struct AllocRec { size_t field_off; char* base; size_t bytes; };
    std::vector<AllocRec> allocs; char* sv_base = nullptr; size_t sv_bytes = 0; char* xr_base = nullptr; size_t xr_bytes = 0;
    int mw_world = 0; char* rep_mem = nullptr; size_t rep_stride = 0; KaiCtx* d_ctxs = nullptr; MultiCtx* d_mw = nullptr; void* d_segs = nullptr; int n_segs = 0;
    ScanGrid* d_sg = nullptr;  // the scan grid's table (allocate action on the sequential engine, kai_kernels.hpp)
    // victim actions of a node-sharded group: the waves' outcomes exchanged over the ranks (kai_victim_shard.hpp) — the caller's all-gather on HOST memory (kai_shard_attach_host)
    // or the library's own RCCL communicator on xstream; the mailbox the running kernel rings, pinned staging for the copies in and out of MultiCtx
    kai_allgather_fn xag_fn = nullptr; void* xag_user = nullptr;
    XMail* mail = nullptr; XMail* d_mail = nullptr; hipStream_t xstream = nullptr;
    HandleBuf xpin{true}, xd_send{false}, xd_recv{false};
    XShardHost xs;
    std::vector<MultiCtx> mw_host;  // staging of the victim actions' shared block (one per handle: handles of several ranks may run on threads of one process)
    // kai_session_open's host preparation, kept with the handle: a scheduler opens a session per cycle, and arrays that keep their memory are not mapped and page-faulted
    // in again every cycle (config 5: ~150 MB of host memory stays with the handle; build() rewrites every element it hands out)
    HostPrep prep; SharedPods sp;
    // pinned host staging for the snapshot's own arrays (kai_session_open, UploadStage): grows, lives with the handle
    HandleBuf up_pin{true};
    // kai_session_update (kai_delta.hpp): what the open derives from pod status / node / group and node flags / allocatable, kept so that a delta adjusts it
    // (HostPrep keeps the class operands, the exact-sum counts and the nodes' rows in engine order)
    bool idx_forced_off = false, fast_forced_off = false;  // the open's shared-GPU / MIG rules on the class index and the staged job path
    bool legacy_on = false; std::vector<int32_t> legacy_cnt;  // per engine node: active legacy MIG tasks (only when the snapshot has such a pod)
    bool gm_guard = false;  // shared-GPU requests + node_gpu_memory: the cluster's one GPU memory size is found among the nodes that have GPUs
    std::vector<int64_t> h_gpu_mem;  // node_gpu_memory in engine order (what n_gpu_mem holds)
    std::map<int32_t, int32_t> new_groups;  // shared-GPU group ids >= KAI_NEW_GROUP in the snapshot and how many pods carry them (next_group0)
    std::vector<std::vector<std::pair<uint32_t, int32_t>>> np_lists; std::vector<uint32_t> np_uid; size_t np_cap = 0;  // shared GPUs: each node's active pods as (UID rank, pod); every pod's UID rank
    decltype(KaiCtx::bt) bt_pools{}; bool bt_alloc = false; int bt_C = 0;  // the batch path's pools of this session (bound for bt_C classes)
    int cls_cap = 0;  // classes the session's cls / sum1_key / sum1_node arrays hold
    uint32_t* d_rank = nullptr; int32_t* d_pkey = nullptr; int32_t* d_remap = nullptr; size_t remap_cap = 0;  // first update of a session: name ranks, pods' request keys, key -> class
    HandleBuf dl_pin{true}, dl_dev{false};  // the delta's staging: pinned and device, grows, lives with the handle
    // kai_best_nodes and kai_ordered_nodes (kai_best_nodes.hpp, kai_ordered_nodes.hpp; one pair for both): pinned staging and device scratch, grow, live with the handle; whether the scratch holds this session's permutation
    HandleBuf bn_pin{true}, bn_dev{false}; bool bn_perm_ok = false; int cus = 0;  // (compute units of the device: device_cus)
    // kai_ops_apply (kai_ops_apply.hpp): pinned staging and device scratch, grow, live with the handle; pods the scratch's per-pod arrays hold; caller's node index -> name rank (of this session's permutation)
    HandleBuf oa_pin{true}, oa_dev{false}; size_t oa_pod_cap = 0; std::vector<int32_t> oa_rank; bool oa_rank_ok = false;
    // kai_stale_gang_eviction (kai_stale_gangs.hpp): pinned staging and device scratch, grow, live with the handle; jobs and pod-grid workgroups the scratch's arrays hold
    HandleBuf sg_pin{true}, sg_dev{false}; size_t sg_job_cap = 0, sg_wg_cap = 0;
    // kai_job_order (kai_job_order.hpp): pinned staging and device scratch (the call's outputs, the tree tables, the plan's pools), grow, live with the handle
    HandleBuf jo_pin{true}, jo_dev{false};
    // kai_subset_nodes (kai_subset_nodes.hpp): pinned staging, device scratch and the emitted sets' own buffer, grow, live with the handle; whether the scratch holds this session's
    // tables (both node permutations, the open's children table); the session's topologies: raw records a query can have, the most levels of one (found with the first call)
    HandleBuf sn_pin{true}, sn_dev{false}, sn_out{false}; bool sn_tab_ok = false, sn_shape_ok = false; int sn_stride = 1, sn_levels = 0;
    // kai_stmt_* (kai_stmt.hpp): the open Statement — the log's length and one byte per record (its kai_op kind, ST_REC_WIDE: the chip-wide kernels may undo / commit it);
    // its own device memory (stamps and verdict: sized at kai_stmt_begin, so that it does not grow while the Statement is open), the committed operations' device buffer and
    // pinned staging (grown by the commit)
    bool st_open = false; std::vector<uint8_t> st_rec; HandleBuf st_pin{true}, st_dev{false}, st_out{false}; size_t st_pod_cap = 0;
    // kai_stmt_place (kai_stmt_place.hpp): pinned staging and device scratch, grow, live with the handle; whether the scratch holds this session's permutation
    HandleBuf sp_pin{true}, sp_dev{false}; bool sp_perm_ok = false;
    std::vector<HandleBuf*> handle_bufs() { return {&rep_buf, &dl_pin, &dl_dev, &bn_pin, &bn_dev, &oa_pin, &oa_dev, &st_pin, &st_dev, &st_out, &sp_pin, &sp_dev, &sg_pin, &sg_dev, &jo_pin, &jo_dev, &sn_pin, &sn_dev, &sn_out, &pin_buf, &up_pin, &xpin, &xd_send, &xd_recv, &rpin}; }  // every one: kai_core_destroy
};

// leave the function with a step's status unless it is KAI_OK; a HIP call's error becomes KAI_ERR_HIP with the call's text in kai_last_error
#define KAI_TRY(x) do { const int rc_ = (x); if (rc_) return rc_; } while (0)
#define HIP_TRY(core, expr) KAI_TRY(hip_status((core), (expr), #expr))
inline int hip_status(kai_core* core, hipError_t e, const char* what) { if (e == hipSuccess) return KAI_OK; core->err = std::string(what) + ": " + hipGetErrorString(e); return KAI_ERR_HIP; }

namespace {

int fail(kai_core* core, int code, const char* msg) { core->err = msg; return code; }
// HandleBuf::grow for the callers that fail with the allocation (up_pin and rep_buf fall back instead: they call grow themselves)
int reserve(kai_core* core, HandleBuf& b, size_t need, size_t want, bool* grew = nullptr) { return hip_status(core, b.grow(need, want, grew), b.pinned ? "hipHostMalloc" : "hipMalloc"); }
double ms_between(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }
int device_cus(kai_core* core) {  // compute units of the handle's device, or 64 when the runtime does not say; asked once
    if (core->cus <= 0 && (hipDeviceGetAttribute(&core->cus, hipDeviceAttributeMultiprocessorCount, core->device) != hipSuccess || core->cus <= 0)) core->cus = 64;
    return core->cus;
}
template <class T> int dalloc(kai_core* core, T** out, size_t n) {
    size_t bytes = (std::max<size_t>(n, 1) * sizeof(T) + 255) & ~(size_t)255;
    if (bytes > core->slab_left) {
        size_t want = std::max<size_t>(bytes, (size_t)256 << 20);  // 256 MiB slabs (2 MiB-aligned by the driver)
        if (core->open && want > core->post_open_max) core->post_open_max = want;  // (what the end-of-open trim of the NEXT session keeps a slab for)
        void* p = nullptr;
        // a slab of the previous session first: a scheduler opens a session per cycle (scheduler.go:112-138), and hipFree + hipMalloc of a few 256 MiB
        // slabs per cycle would be milliseconds of every one of them
        // (the smallest one that is large enough; what an open leaves unused is released at its end, trim_spare)
        { size_t best = core->spare.size();
          for (size_t i = 0; i < core->spare.size(); i++) if (core->spare[i].second >= want && (best == core->spare.size() || core->spare[i].second < core->spare[best].second)) best = i;
          if (best != core->spare.size()) { p = core->spare[best].first; want = core->spare[best].second; core->spare.erase(core->spare.begin() + (long)best); } }
        if (!p) HIP_TRY(core, hipMalloc(&p, want));
        core->bufs.push_back(p); core->buf_bytes.push_back(want);
        core->slab = static_cast<char*>(p); core->slab_left = want;
    }
    *out = reinterpret_cast<T*>(core->slab);
    core->slab += bytes; core->slab_left -= bytes;
    return KAI_OK;
}
// KaiCtx fields are address-space-qualified pointers in the device pass (kai_engine.hpp KAI_GP): assign them through casts
#define KAI_VP(x) ((void*)(x))
template <class F> int dalloc_f(kai_core* core, F& field, size_t n) {
    char* p = nullptr;
    int rc = dalloc(core, &p, std::max<size_t>(n, 1) * sizeof(*field));
    if (rc) return rc;
    field = (F)p;
    { const char* fp = reinterpret_cast<const char*>(&field); const char* c0 = reinterpret_cast<const char*>(&core->ctx);  // a field of the session context: its array is part of every replica
      if (fp >= c0 && fp + sizeof(void*) <= c0 + sizeof(KaiCtx)) core->allocs.push_back({(size_t)(fp - c0), p, std::max<size_t>(n, 1) * sizeof(*field)}); }
    return KAI_OK;
}
template <class F> int dfill_f(kai_core* core, F& field, size_t n, int byte) {  // the array allocated and every byte of it set on the device (0xFF: -1 in every element)
    KAI_TRY(dalloc_f(core, field, n));
    HIP_TRY(core, hipMemsetAsync(KAI_VP(field), byte, std::max<size_t>(n, 1) * sizeof(*field), core->stream));
    return KAI_OK;
}
template <class F> int dzero_f(kai_core* core, F& field, size_t n) { return dfill_f(core, field, n, 0); }
template <class F, class T> int dupload_f(kai_core* core, F& field, const T* host, size_t n) {
    static_assert(sizeof(*field) == sizeof(T), "element size");
    int rc = dalloc_f(core, field, n);
    if (rc) return rc;
    if (n) HIP_TRY(core, hipMemcpyAsync(KAI_VP(field), host, n * sizeof(T), hipMemcpyHostToDevice, core->stream));
    else HIP_TRY(core, hipMemsetAsync(KAI_VP(field), 0, sizeof(T), core->stream));  // (an empty array is one element nobody reads: zeros rather than what the slab held before)
    return KAI_OK;
}
template <class F, class S> int dcopy_f(kai_core* core, F& field, S src, size_t n) {  // the array allocated and filled from device memory
    static_assert(sizeof(*field) == sizeof(*src), "element size");
    KAI_TRY(dalloc_f(core, field, n));
    if (n) HIP_TRY(core, hipMemcpyAsync(KAI_VP(field), KAI_VP(src), n * sizeof(*field), hipMemcpyDeviceToDevice, core->stream));
    return KAI_OK;
}
// The snapshot's own arrays (nothing the host preparation derives) go up FIRST and from pinned memory: add() allocates the device array, flush() copies the host arrays into the
// handle's pinned staging buffer on the host's cores and enqueues one DMA per array — which then runs while kai_session_open's host preparation (milliseconds of loops over the same
// pods and jobs) keeps the cores busy.  hipMemcpyAsync from the caller's pageable arrays, as every other upload of the open is made, stages through the runtime's own bounce buffers on
// the calling thread and returns when the data has left the host: ~27 GB/s and nothing else happens meanwhile.  Below 4 MB (nearly every session of the test suites) and with
// KAI_OPEN_NO_STAGING the arrays are sent that way, in the same order to the same places.
struct UploadStage {
    kai_core* core; struct Seg { void* dst; const void* src; size_t bytes, off; }; std::vector<Seg> segs; size_t total = 0;
    template <class F, class T> int add(F& field, const T* host, size_t n) {
        static_assert(sizeof(*field) == sizeof(T), "element size");
        int rc = dalloc_f(core, field, n); if (rc) return rc;
        if (n) { segs.push_back({KAI_VP(field), host, n * sizeof(T), total}); total += (n * sizeof(T) + 255) & ~(size_t)255; }
        else HIP_TRY(core, hipMemsetAsync(KAI_VP(field), 0, sizeof(T), core->stream));
        return KAI_OK;
    }
    int flush() {
        bool pinned = total >= ((size_t)4 << 20) && !std::getenv("KAI_OPEN_NO_STAGING");
        if (pinned && core->up_pin.grow(total, total + total / 4) != hipSuccess) { pinned = false; (void)hipGetLastError(); }  // (no pinned memory to be had: the plain way)
        if (pinned) {
            char* pin = reinterpret_cast<char*>(core->up_pin.p);
            parallel_chunks(total, [&](int, size_t a, size_t b) {  // byte range [a, b) of the staging buffer: the pieces of the arrays that fall into it
                for (const Seg& g : segs) { const size_t lo = std::max(a, g.off), hi = std::min(b, g.off + g.bytes); if (lo < hi) std::memcpy(pin + lo, static_cast<const char*>(g.src) + (lo - g.off), hi - lo); }
            }, (size_t)1 << 20);
            for (const Seg& g : segs) HIP_TRY(core, hipMemcpyAsync(g.dst, pin + g.off, g.bytes, hipMemcpyHostToDevice, core->stream));
        } else {
            for (const Seg& g : segs) HIP_TRY(core, hipMemcpyAsync(g.dst, g.src, g.bytes, hipMemcpyHostToDevice, core->stream));
        }
        segs.clear(); total = 0;
        return KAI_OK;
    }
};
// kai_ctx_build.hpp's arena on the session's slabs: the helpers above, the first failure kept
struct DevArena {
    kai_core* core; UploadStage up{core}; int rc = KAI_OK;
    template <class F> void alloc(F& field, size_t n) { if (!rc) rc = dalloc_f(core, field, n); }
    template <class F> void fill(F& field, size_t n, int byte) { if (!rc) rc = dfill_f(core, field, n, byte); }
    template <class F> void zero(F& field, size_t n) { fill(field, n, 0); }
    template <class F, class T> void upload(F& field, const T* host, size_t n) { if (!rc) rc = dupload_f(core, field, host, n); }
    template <class F, class T> void stage(F& field, const T* host, size_t n) { if (!rc) rc = up.add(field, host, n); }
    int flush() { if (!rc) rc = up.flush(); return rc; }
    template <class F, class S> void copy_of(F& field, S src, size_t n) { if (!rc) rc = dcopy_f(core, field, src, n); }
    int status() const { return rc; }
};
void free_session(kai_core* core, bool release = false) {
    // the slabs stay with the handle for the next session (dalloc takes them back); kai_core_destroy releases them
    if (core->bufs.size() != core->buf_bytes.size()) { for (void* p : core->bufs) (void)hipFree(p); core->bufs.clear(); core->buf_bytes.clear(); }  // (every slab carries its size: dalloc is the only writer of both; anything else is a bug — release rather than recycle under a wrong size)
    for (size_t i = 0; i < core->bufs.size(); i++) core->spare.push_back({core->bufs[i], core->buf_bytes[i]});
    core->bufs.clear(); core->buf_bytes.clear(); core->slab = nullptr; core->slab_left = 0;
    if (release) { for (auto& sp : core->spare) (void)hipFree(sp.first); core->spare.clear(); }
    core->d_rank = nullptr; core->d_pkey = nullptr; core->d_remap = nullptr; core->remap_cap = 0; core->bt_alloc = false;
    core->allocs.clear(); core->sv_base = nullptr; core->xr_base = nullptr; core->mw_world = 0; core->rep_mem = nullptr; core->d_ctxs = nullptr; core->d_mw = nullptr; core->d_segs = nullptr; core->d_sg = nullptr;
    core->open = false; core->st_open = false;
}
// nothing leaves an entry point by an exception: the status and the message instead
template <class F> int no_throw(kai_core* core, const std::string& what, F&& f) {
    try { return f(); }
    catch (const std::bad_alloc&) { core->err = what + ": out of host memory"; return KAI_ERR_NO_MEMORY; }
    catch (const std::exception& e) { core->err = what + ": " + e.what(); return KAI_ERR_INVALID_ARG; }
    catch (...) { core->err = what + ": unknown exception"; return KAI_ERR_INVALID_ARG; }
}
// a failure after the session began to change: the stream drained (staged copies read the handle's pinned buffers), the slabs back with the handle, the message kept
void close_failed(kai_core* core) { const std::string why = core->err; if (core->stream) (void)hipStreamSynchronize(core->stream); free_session(core); core->err = why; }
// the batch path's pools and tables of this session (kai_batch.hpp), from the slabs; kept with the handle so that a later update binds them again without allocating
int bind_batch_pools(kai_core* core) {
    KaiCtx& c = core->ctx;
    const int rcb = batch_bind(c, core->prep,
        [&](size_t bytes) -> void* { char* p = nullptr; if (dalloc(core, &p, bytes)) return nullptr; if (hipMemsetAsync(p, 0, bytes, core->stream) != hipSuccess) return nullptr; return p; },
        [&](void* d, const void* h, size_t n) -> int { return hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, core->stream) == hipSuccess ? 0 : (int)KAI_ERR_HIP; },
        core->world, core->rank, core->shard_k);
    if (rcb) return fail(core, rcb, "batch path buffers");
    core->bt_pools = c.bt; core->bt_alloc = c.bt.enabled != 0; core->bt_C = c.C;
    return KAI_OK;
}
}  // namespace
