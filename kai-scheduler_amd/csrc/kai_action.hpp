// kai_action.hpp — kai_action_execute's host side: the batch path's launcher (DevLauncher), the exchange of a node-sharded group's victim actions (DevXIo, xshard_*), the victim actions' replicas (k_replicate, prepare_multi), the solver's scratch, the action in its steps.
#pragma once
#include "kai_rccl.hpp"
namespace {
// The dynamic-LDS ceiling of a kernel (hipFuncAttributeMaxDynamicSharedMemorySize) belongs to the process and the device, not to a handle: a second handle with a smaller cluster
// must not lower it under the first handle's next launch.  So the mark is kept per device for the whole process and only ever rises.  which: 0 k_fill_buckets, 1 k_fill_counts, 2 k_fill_levels, 3 / 4 the spread instantiations of the latter two.
bool fill_dyn_raise(int device, int which, const void* kernel, size_t dyn) {
    static std::mutex mu; static std::map<int, size_t> mark[5];
    std::lock_guard<std::mutex> lock(mu);
    size_t& m = mark[which][device];
    if (dyn <= m) return true;
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn) != hipSuccess) return false;
    m = dyn; return true;
}
// the batch path's kernels on the session's stream (kai_batch_driver.hpp's Launcher)
struct DevLauncher {
    kai_core* core; int rc = 0; unsigned fill_attr_mask = 0; size_t fill_attr_dyn = 0; bool timed = false; unsigned timed_slots = 0;  // (timed: the round recorded its phase events; per slot in the rounds without the host)
    hipEvent_t* pev = nullptr;  // the phase events the next round records into: the session's four (loop on the host) or a slot's (rounds without the host)
    hipEvent_t ev(int i) { return pev ? pev[i] : core->bev[i]; }
    void static_rank(int g, int b, const KaiCtx& c) { hipLaunchKernelGGL(k_batch_static_rank, dim3(g), dim3(b), 0, core->stream, c); }
    void static_check(int g, int b, const KaiCtx& c) { hipLaunchKernelGGL(k_batch_static_check, dim3(g), dim3(b), 0, core->stream, c); }
    void qualify(int g, int b, const KaiCtx& c) { hipLaunchKernelGGL(k_batch_qualify, dim3(g), dim3(b), 0, core->stream, c); }
    void nrec(int g, int b, const KaiCtx& c) { hipLaunchKernelGGL(k_batch_nrec, dim3(g), dim3(b), 0, core->stream, c); }
    void plan_setup(int g, int b, const KaiCtx& c, RoundParams rp) { (void)hipEventRecord(ev(0), core->stream); hipLaunchKernelGGL(k_plan_setup, dim3(g), dim3(b), 0, core->stream, c, rp); }
    void plan_leaf(int g, int b, const KaiCtx& c, RoundParams rp) { hipLaunchKernelGGL(k_plan_leaf, dim3(g), dim3(b), 0, core->stream, c, rp); }
    void plan_rank(int g, int b, const KaiCtx& c, RoundParams rp) { hipLaunchKernelGGL(k_plan_rank, dim3(g), dim3(b), 0, core->stream, c, rp); }
    void plan_gather(int g, int b, const KaiCtx& c, RoundParams rp) { hipLaunchKernelGGL(k_plan_gather, dim3(g), dim3(b), 0, core->stream, c, rp); }
    void plan_scan(int g, int b, const KaiCtx& c, RoundParams rp) { hipLaunchKernelGGL(k_plan_scan, dim3(g), dim3(b), 0, core->stream, c, rp); }
    void seg_sum(int g, int b, const KaiCtx& c, RoundParams rp, int segs) { hipLaunchKernelGGL(k_seg_sum, dim3(g), dim3(b), 0, core->stream, c, rp, segs); }
    void seg_gate(int g, int b, const KaiCtx& c, RoundParams rp, int segs) { hipLaunchKernelGGL(k_seg_gate, dim3(g), dim3(b), 0, core->stream, c, rp, segs); }
    void seg_keys(int g, int b, const KaiCtx& c, RoundParams rp, int segs) { hipLaunchKernelGGL(k_seg_keys, dim3(g), dim3(b), 0, core->stream, c, rp, segs); }
    void seg_max(int g, int b, const KaiCtx& c, RoundParams rp, int segs) { hipLaunchKernelGGL(k_seg_max, dim3(g), dim3(b), 0, core->stream, c, rp, segs); }
    void plan_emit(int g, int b, const KaiCtx& c) { hipLaunchKernelGGL(k_plan_emit, dim3(g), dim3(b), 0, core->stream, c); }
    void class_capacity(int g, int b, const KaiCtx& c, int buckets, int levels) { hipLaunchKernelGGL(k_class_capacity, dim3(g), dim3(b), 0, core->stream, c, buckets, levels); }
    template <int MODE, bool SPEC, bool L1L> void fill_launch(int g, int b, size_t dyn, const KaiCtx& c, RoundParams rp) {
        const unsigned vbit = 1u << ((MODE == FM_SHARDED ? 4 : 0) + (SPEC ? 2 : 0) + (L1L ? 1 : 0));  // once per variant and action: the dynamic-LDS ceiling of the kernel
        if (!(fill_attr_mask & vbit) || dyn > fill_attr_dyn) { if (hipFuncSetAttribute(reinterpret_cast<const void*>(k_fill<MODE, SPEC, L1L>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn) != hipSuccess) rc = KAI_ERR_HIP; fill_attr_mask |= vbit; fill_attr_dyn = std::max(fill_attr_dyn, dyn); }
        hipLaunchKernelGGL((k_fill<MODE, SPEC, L1L>), dim3(g), dim3(b), dyn, core->stream, c, rp);
    }
    void fill(int g, int b, size_t dyn, const KaiCtx& c, RoundParams rp, int l1) {
        if (rp.mode == 0 || (rp.mode == 2 && rp.start == 0)) (void)hipEventRecord(ev(1), core->stream);  // a sharded round: from its first virtual fill …
        const bool spec = (c.plugins & KB_KEY_PLUGINS) == KB_KEY_PLUGINS && c.R == 4, sh = rp.mode == 2;
        if (sh) { if (spec) { if (l1) fill_launch<FM_SHARDED, true, true>(g, b, dyn, c, rp); else fill_launch<FM_SHARDED, true, false>(g, b, dyn, c, rp); }
                  else { if (l1) fill_launch<FM_SHARDED, false, true>(g, b, dyn, c, rp); else fill_launch<FM_SHARDED, false, false>(g, b, dyn, c, rp); } }
        else { if (spec) { if (l1) fill_launch<FM_PLAIN, true, true>(g, b, dyn, c, rp); else fill_launch<FM_PLAIN, true, false>(g, b, dyn, c, rp); }
               else { if (l1) fill_launch<FM_PLAIN, false, true>(g, b, dyn, c, rp); else fill_launch<FM_PLAIN, false, false>(g, b, dyn, c, rp); } }
        if (rp.mode != 1) (void)hipEventRecord(ev(2), core->stream);                                       // … to its last (exchanges included)
    }
    void bucket_build(int g, int b, const KaiCtx& c) { hipLaunchKernelGGL(k_bucket_build, dim3(g), dim3(b), 0, core->stream, c); }
    // the set-based fills (kai_fill_counts.hpp, kai_fill_levels.hpp, kai_fill_buckets.hpp); which: fill_dyn_raise's mark.  (The GPU strategy is a compile-time parameter of the first two kernels' bodies: two instantiations.)
    template <class K> void fill_sets(K kernel, int which, int g, int b, size_t dyn, const KaiCtx& c, RoundParams rp, BucketParams bp) {
        if (!fill_dyn_raise(core->device, which, reinterpret_cast<const void*>(kernel), dyn)) rc = KAI_ERR_HIP;
        if (rp.mode == 0) (void)hipEventRecord(ev(1), core->stream);
        hipLaunchKernelGGL(kernel, dim3(g), dim3(b), dyn, core->stream, c, rp, bp);
        if (rp.mode != 1) (void)hipEventRecord(ev(2), core->stream);
    }
    void fill_counts(int g, int b, size_t dyn, const KaiCtx& c, RoundParams rp, BucketParams bp) { const bool sp = c.gpu_strategy == KAI_SPREAD; fill_sets(sp ? k_fill_counts_spread : k_fill_counts, sp ? 3 : 1, g, b, dyn, c, rp, bp); }
    void fill_levels(int g, int b, size_t dyn, const KaiCtx& c, RoundParams rp, BucketParams bp) { const bool sp = c.gpu_strategy == KAI_SPREAD; fill_sets(sp ? k_fill_levels_spread : k_fill_levels, sp ? 4 : 2, g, b, dyn, c, rp, bp); }
    void fill_buckets(int g, int b, size_t dyn, const KaiCtx& c, RoundParams rp, BucketParams bp) { fill_sets(k_fill_buckets, 0, g, b, dyn, c, rp, bp); }
    void apply_jobs(int g, int b, const KaiCtx& c, int64_t ops_base, int64_t stmt_base) { hipLaunchKernelGGL(k_apply_jobs, dim3(g), dim3(b), 0, core->stream, c, (long long)ops_base, (long long)stmt_base); }
    void apply_nodes(int g, int b, const KaiCtx& c) { hipLaunchKernelGGL(k_apply_nodes, dim3(g), dim3(b), 0, core->stream, c); (void)hipEventRecord(ev(3), core->stream); timed = true; }
    void index_from_recs(int g, int b, const KaiCtx& c, const NodeRec* recs, int n_recs, uint64_t* l1k, int32_t* l1n, int nb, int blk0, int blk1) { hipLaunchKernelGGL(k_index_from_recs, dim3(g), dim3(b), 0, core->stream, c, recs, n_recs, l1k, l1n, nb, blk0, blk1); }
    void shard_mask_nrec(int g, int b, const KaiCtx& c) { hipLaunchKernelGGL(k_shard_mask_nrec, dim3(g), dim3(b), 0, core->stream, c); }
    void shard_keys(int g, int b, const KaiCtx& c) { hipLaunchKernelGGL(k_shard_keys, dim3(g), dim3(b), 0, core->stream, c); }
    void shard_select(int g, int b, const KaiCtx& c) { hipLaunchKernelGGL(k_shard_select, dim3(g), dim3(b), 0, core->stream, c); }
    void shard_compact(int g, int b, const KaiCtx& c) { hipLaunchKernelGGL(k_shard_compact, dim3(g), dim3(b), 0, core->stream, c); }
    void shard_vbuild(int g, int b, const KaiCtx& c) { hipLaunchKernelGGL(k_shard_vbuild, dim3(g), dim3(b), 0, core->stream, c); }
    void shard_scatter(int g, int b, const KaiCtx& c, int total) { hipLaunchKernelGGL(k_shard_scatter, dim3(g), dim3(b), 0, core->stream, c, total); }
    // the group's all-gather is the caller's (torch.distributed over RCCL / xGMI in the Python mirror): the library hands over its device buffers
    int allgather(const void* send, void* recv, int64_t bytes) {
        if (core->rccl_comm) {  // the library's own communicator: stream-ordered with the kernels on either side, nothing to wait for on the host
            const int rc = rccl_api()->AllGather(send, recv, (size_t)bytes, /*ncclUint8*/ 1, core->rccl_comm, core->stream);
            return rc ? rccl_fail(core, "ncclAllGather", rc) : KAI_OK;
        }
        if (!core->ag_fn) { core->err = "node-sharded group without kai_shard_attach"; return KAI_ERR_COMM; }
        if (hipStreamSynchronize(core->stream) != hipSuccess) return KAI_ERR_HIP;
        if (core->ag_fn(core->ag_user, send, recv, bytes) != 0) { core->err = "the caller's all-gather failed"; return KAI_ERR_COMM; }
        return KAI_OK;
    }
    int read(void* dst, const void* src, size_t n) {
        hipError_t e1 = n ? hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, core->stream) : hipSuccess, e2 = hipStreamSynchronize(core->stream), e3 = hipGetLastError();
        if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) { core->err = std::string("batch path: ") + hipGetErrorString(e1 != hipSuccess ? e1 : e2 != hipSuccess ? e2 : e3); return KAI_ERR_HIP; }
        if (rc) return rc;
        if (timed) { add_phase_times(core->bev); timed = false; }
        return KAI_OK;
    }
    void add_phase_times(hipEvent_t* e) {  // a round's phases, from the events recorded around them
        float a = 0, f = 0, p = 0;
        if (hipEventElapsedTime(&p, e[0], e[1]) == hipSuccess && hipEventElapsedTime(&f, e[1], e[2]) == hipSuccess && hipEventElapsedTime(&a, e[2], e[3]) == hipSuccess) { core->batch_plan_ms += p; core->batch_fill_ms += f; core->batch_apply_ms += a; }
        else (void)hipGetLastError();  // an event that was not recorded this round: not an error of the path
    }
    // ---- rounds without the host: the loop's state on the device, its copies in pinned memory
    void round_init(const KaiCtx& c, int remaining, int H0, int policy, int64_t ops_base, int64_t stmt_base) { hipLaunchKernelGGL(k_round_init, dim3(1), dim3(64), 0, core->stream, c, remaining, H0, policy, (long long)ops_base, (long long)stmt_base); }
    void round_next(const KaiCtx& c) { hipLaunchKernelGGL(k_round_next, dim3(1), dim3(64), 0, core->stream, c); }
    void round_finish(const KaiCtx& c) { hipLaunchKernelGGL(k_round_finish, dim3(1), dim3(64), 0, core->stream, c); pev = nullptr; }
    bool round_ready() {
        if (core->rev_ready) return true;
        for (auto& slot : core->rev) for (hipEvent_t& e : slot) if (!e && hipEventCreate(&e) != hipSuccess) return false;
        if (core->rpin.grow((size_t)KB_ROUND_SLOTS * 256, (size_t)KB_ROUND_SLOTS * 256) != hipSuccess) return false;
        static_assert(sizeof(RoundCtl) <= 256, "a pinned slot holds one RoundCtl");
        return core->rev_ready = true;
    }
    void round_begin(int slot) { if (round_ready()) pev = core->rev[slot]; }
    int round_post(int slot, const void* src, size_t n) {  // the state behind round `slot`, stream-ordered into the slot's pinned copy
        if (!round_ready()) { core->err = "batch path: no events / pinned memory for the round loop"; return KAI_ERR_HIP; }
        if (hipMemcpyAsync(core->rpin.p + (size_t)slot * 256, src, n, hipMemcpyDeviceToHost, core->stream) != hipSuccess || hipEventRecord(core->rev[slot][4], core->stream) != hipSuccess) { core->err = "batch path: the round's state copy failed"; return KAI_ERR_HIP; }
        if (timed) { timed_slots |= 1u << slot; timed = false; }
        return KAI_OK;
    }
    int round_wait(int slot, void* dst, size_t n) {  // waits for that copy — not for the stream: the next round is already behind it
        hipError_t e1 = hipEventSynchronize(core->rev[slot][4]), e2 = hipGetLastError();
        if (e1 != hipSuccess || e2 != hipSuccess) { core->err = std::string("batch path: ") + hipGetErrorString(e1 != hipSuccess ? e1 : e2); return KAI_ERR_HIP; }
        if (rc) return rc;
        std::memcpy(dst, core->rpin.p + (size_t)slot * 256, n);
        if (timed_slots & (1u << slot)) { add_phase_times(core->rev[slot]); timed_slots &= ~(1u << slot); }
        return KAI_OK;
    }
    int write(void* dst, const void* src, size_t n) { return hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, core->stream) == hipSuccess ? KAI_OK : KAI_ERR_HIP; }
    int zero(void* dst, size_t n) { return hipMemsetAsync(dst, 0, n, core->stream) == hipSuccess ? KAI_OK : KAI_ERR_HIP; }  // (a copy from pageable host memory is staged and waited for; a memset is a launch)
};
// ---- victim actions of a node-sharded group: the host side of a wave's exchange (kai_victim_shard.hpp XShardHost) against the device
struct DevXIo {
    kai_core* core;
    // pinned layout: [0,32) MultiCtx header | res (cap x 4) | cnt (cap x 64) | scalars
    int pull(int32_t* hdr, int32_t* res, int64_t* cnt, int b, int cap) {
        MultiCtx* M = core->d_mw; unsigned char* p = core->xpin.p;
        if (hipMemcpyAsync(p, M, 32, hipMemcpyDeviceToHost, core->xstream) != hipSuccess) return KAI_ERR_HIP;
        if (hipMemcpyAsync(p + 64, &M->res[b][0], (size_t)cap * 4, hipMemcpyDeviceToHost, core->xstream) != hipSuccess) return KAI_ERR_HIP;
        if (hipMemcpyAsync(p + 64 + (size_t)KAI_MW_WAVE * 4, &M->cnt[b][0][0], (size_t)cap * 8 * KAI_MW_CNT, hipMemcpyDeviceToHost, core->xstream) != hipSuccess) return KAI_ERR_HIP;
        if (hipStreamSynchronize(core->xstream) != hipSuccess) return KAI_ERR_HIP;
        std::memcpy(hdr, p, 32); std::memcpy(res, p + 64, (size_t)cap * 4); std::memcpy(cnt, p + 64 + (size_t)KAI_MW_WAVE * 4, (size_t)cap * 8 * KAI_MW_CNT);
        return 0;
    }
    int push(int b, const int32_t* res, const int64_t* cnt, int cap, int hit, int xrun, int fault) {
        MultiCtx* M = core->d_mw; unsigned char* p = core->xpin.p;
        std::memcpy(p + 64, res, (size_t)cap * 4); std::memcpy(p + 64 + (size_t)KAI_MW_WAVE * 4, cnt, (size_t)cap * 8 * KAI_MW_CNT);
        int32_t* sc = reinterpret_cast<int32_t*>(p + 32); sc[0] = hit; sc[1] = xrun; sc[2] = 1;
        if (hipMemcpyAsync(&M->res[b][0], p + 64, (size_t)cap * 4, hipMemcpyHostToDevice, core->xstream) != hipSuccess) return KAI_ERR_HIP;
        if (hipMemcpyAsync(&M->cnt[b][0][0], p + 64 + (size_t)KAI_MW_WAVE * 4, (size_t)cap * 8 * KAI_MW_CNT, hipMemcpyHostToDevice, core->xstream) != hipSuccess) return KAI_ERR_HIP;
        if (hipMemcpyAsync(&M->hit[b], &sc[0], 4, hipMemcpyHostToDevice, core->xstream) != hipSuccess) return KAI_ERR_HIP;
        if (hipMemcpyAsync(&M->xrun[b], &sc[1], 4, hipMemcpyHostToDevice, core->xstream) != hipSuccess) return KAI_ERR_HIP;
        if (fault && hipMemcpyAsync(&M->fault, &sc[2], 4, hipMemcpyHostToDevice, core->xstream) != hipSuccess) return KAI_ERR_HIP;
        return hipStreamSynchronize(core->xstream) == hipSuccess ? 0 : (int)KAI_ERR_HIP;
    }
    int raise_fault() { int32_t* sc = reinterpret_cast<int32_t*>(core->xpin.p + 32); sc[2] = 1; (void)hipMemcpyAsync(&core->d_mw->fault, &sc[2], 4, hipMemcpyHostToDevice, core->xstream); return hipStreamSynchronize(core->xstream) == hipSuccess ? 0 : (int)KAI_ERR_HIP; }
    int allgather(const void* send, void* recv, int64_t bytes) {
        if (core->xag_fn) return core->xag_fn(core->xag_user, send, recv, bytes) == 0 ? 0 : (int)KAI_ERR_COMM;
        if (!core->rccl_comm || (size_t)bytes * core->world > core->xd_recv.bytes) return KAI_ERR_COMM;
        if (hipMemcpyAsync(core->xd_send.p, send, (size_t)bytes, hipMemcpyHostToDevice, core->xstream) != hipSuccess) return KAI_ERR_HIP;
        if (rccl_api()->AllGather(core->xd_send.p, core->xd_recv.p, (size_t)bytes, /*ncclUint8*/ 1, core->rccl_comm, core->xstream)) return KAI_ERR_COMM;
        if (hipMemcpyAsync(recv, core->xd_recv.p, (size_t)bytes * core->world, hipMemcpyDeviceToHost, core->xstream) != hipSuccess) return KAI_ERR_HIP;
        return hipStreamSynchronize(core->xstream) == hipSuccess ? 0 : (int)KAI_ERR_HIP;
    }
};
// mailbox, second stream, staging: once per handle
int xshard_setup(kai_core* core) {
    if (!core->xstream) HIP_TRY(core, hipStreamCreateWithFlags(&core->xstream, hipStreamNonBlocking));
    if (!core->mail) {
        void* m = nullptr; HIP_TRY(core, hipHostMalloc(&m, 4096, hipHostMallocCoherent | hipHostMallocMapped));
        core->mail = static_cast<XMail*>(m); std::memset(m, 0, 4096);
        void* d = nullptr; HIP_TRY(core, hipHostGetDevicePointer(&d, m, 0)); core->d_mail = static_cast<XMail*>(d);
    }
    { const size_t want = 64 + (size_t)KAI_MW_WAVE * 4 + (size_t)KAI_MW_WAVE * 8 * KAI_MW_CNT; KAI_TRY(reserve(core, core->xpin, want, want)); }
    if (core->rccl_comm && !core->xag_fn && !core->xd_send.p) {
        const size_t one = xw_msg_bytes(KAI_MW_WAVE, 1);
        KAI_TRY(reserve(core, core->xd_send, one, one)); KAI_TRY(reserve(core, core->xd_recv, one * (size_t)core->world, one * (size_t)core->world));
    }
    return KAI_OK;
}
// while the action's kernel runs: answer the mailbox (one exchange per wave) until the stream is idle
int xshard_serve(kai_core* core) {
    DevXIo io{core}; int32_t served = 0; long idle = 0;
    for (;;) {
        const int32_t req = __atomic_load_n(&core->mail->req, __ATOMIC_ACQUIRE);
        if (req != served) {
            const int b = __atomic_load_n(&core->mail->buf, __ATOMIC_ACQUIRE) & 1;
            if (core->xs.wave(io, b)) (void)io.raise_fault();  // the engines give up at the barrier behind the answer
            served = req; __atomic_store_n(&core->mail->resp, served, __ATOMIC_RELEASE); idle = 0;
            continue;
        }
        if ((++idle & 63) == 0) {
            const hipError_t q = hipStreamQuery(core->stream);
            if (q == hipSuccess) break;
            if (q != hipErrorNotReady) { core->err = std::string("victim action: ") + hipGetErrorString(q); return KAI_ERR_HIP; }
            if (idle > 4096) std::this_thread::yield();
        }
    }
    return KAI_OK;
}

// ---- victim actions on several workgroups: replicas of the session arrays, one per further workgroup
struct RepSeg { const char* src; unsigned long long dst_off, bytes; };
constexpr size_t REP_CHUNK = (size_t)256 << 10;
__global__ void __launch_bounds__(256) k_replicate(const RepSeg* segs, char* rep_mem, unsigned long long stride) {
    const RepSeg sg = segs[blockIdx.x];
    const uint4* s = reinterpret_cast<const uint4*>(sg.src); uint4* d = reinterpret_cast<uint4*>(rep_mem + (size_t)blockIdx.y * stride + sg.dst_off);
    const size_t n16 = (size_t)sg.bytes / 16;  // (every allocation is a multiple of 256 bytes)
    for (size_t i = threadIdx.x; i < n16; i += blockDim.x) d[i] = s[i];
}
// Builds (first call of a session) and refreshes (every call) the replicas for a victim action on `G` workgroups; G <= 1 or no memory: one workgroup.
int prepare_multi(kai_core* core, int G, int* g_out) {
    *g_out = 1;
    KaiCtx& c = core->ctx;
    c.mw = nullptr; c.mw_rank = 0; c.mw_world = 1;
    if (G <= 1 || core->shared || !core->sv_base) return KAI_OK;  // (with shared GPUs a rolled-back simulation is observable on its node: the simulations of a partial job are not independent)
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    if (core->mw_world != G) {  // the layout of a replica: the registered arrays, the solver's scratch, the shared-GPU residency groups
        if (core->mw_world != 0) return KAI_OK;  // (replicas of another width exist already: keep to one workgroup rather than rebuild)
        size_t total = 0; std::vector<RepSeg> segs;
        auto add = [&](const char* src, size_t bytes) { bytes = up(bytes); for (size_t o = 0; o < bytes; o += REP_CHUNK) segs.push_back({src + o, (unsigned long long)(total + o), (unsigned long long)std::min(REP_CHUNK, bytes - o)}); total += bytes; };
        for (const auto& a : core->allocs) add(a.base, a.bytes);
        add(core->sv_base, core->sv_bytes); add(core->xr_base, core->xr_bytes);
        const size_t need = total * (size_t)(G - 1);
        if (core->rep_buf.grow(need, need) != hipSuccess) {  // (the replicas of the previous session serve again while they are large enough)
            (void)hipGetLastError();
            if (c.mw_xworld > 1) { core->err = "victim action of a node-sharded group: no memory for the replicas (every rank must run the same number of engines)"; return KAI_ERR_HIP; }
            return KAI_OK;
        }
        core->rep_mem = reinterpret_cast<char*>(core->rep_buf.p); core->rep_stride = total;
        RepSeg* dsegs = nullptr; KaiCtx* dctx = nullptr; MultiCtx* dmw = nullptr;
        int rc = dalloc(core, &dsegs, segs.size()); if (rc) return rc;
        rc = dalloc(core, &dctx, (size_t)G); if (rc) return rc;
        rc = dalloc(core, &dmw, (size_t)1); if (rc) return rc;
        HIP_TRY(core, hipMemcpyAsync(dsegs, segs.data(), segs.size() * sizeof(RepSeg), hipMemcpyHostToDevice, core->stream));
        HIP_TRY(core, hipStreamSynchronize(core->stream));  // segs dies with this scope
        core->d_segs = dsegs; core->n_segs = (int)segs.size(); core->d_ctxs = dctx; core->d_mw = dmw; core->mw_world = G;
    }
    // this action's contexts: replica w = the session's context with every array pointer moved into replica w's memory
    std::vector<KaiCtx> ctxs((size_t)G, c);
    for (int w = 0; w < G; w++) {
        KaiCtx& cw = ctxs[w];
        cw.mw = core->d_mw; cw.mw_rank = w; cw.mw_world = G;
        if (w == 0) continue;
        char* rb = core->rep_mem + (size_t)(w - 1) * core->rep_stride; size_t off = 0;
        for (const auto& a : core->allocs) { *reinterpret_cast<char**>(reinterpret_cast<char*>(&cw) + a.field_off) = rb + off; off += up(a.bytes); }
        solver_scratch_bind(cw.sv, rb + off, c.N, c.P, c.S, c.J, c.Q, c.W, c.D + c.T, c.TL, c.G); off += up(core->sv_bytes);
        cw.sv.xr_group = reinterpret_cast<int32_t*>(rb + off); off += up(core->xr_bytes);
        cw.bt.enabled = 0;  // (the batch path's pools are not replicated; a victim action never reads them)
    }
    HIP_TRY(core, hipMemcpyAsync(core->d_ctxs, ctxs.data(), (size_t)G * sizeof(KaiCtx), hipMemcpyHostToDevice, core->stream));
    if (core->mw_host.empty()) core->mw_host.resize(1);
    MultiCtx& m0 = core->mw_host[0]; std::memset(&m0, 0, sizeof m0); m0.world = G; m0.hit[0] = m0.hit[1] = 0x7fffffff;
    HIP_TRY(core, hipMemcpyAsync(core->d_mw, &m0, sizeof(MultiCtx), hipMemcpyHostToDevice, core->stream));
    hipLaunchKernelGGL(k_replicate, dim3(core->n_segs, G - 1), dim3(256), 0, core->stream, (const RepSeg*)core->d_segs, core->rep_mem, (unsigned long long)core->rep_stride);
    HIP_TRY(core, hipGetLastError());
    HIP_TRY(core, hipStreamSynchronize(core->stream));  // ctxs / m0 die with this scope
    *g_out = G;
    return KAI_OK;
}
// scratch of the victim search (and of kai_ops_apply's engine walk, which needs its second-residency table), kept for the rest of the session
int solver_ensure(kai_core* core) {
    if (core->solver_ready) return KAI_OK;
    KaiCtx& c = core->ctx;
    char* base = nullptr; size_t bytes = solver_scratch_bytes(c.N, c.P, c.S, c.J, c.Q, c.W, c.D + c.T, c.TL, c.G);
    int rc0 = dalloc(core, &base, bytes); if (rc0) return rc0;
    HIP_TRY(core, hipMemsetAsync(base, 0, bytes, core->stream));
    solver_scratch_bind(c.sv, base, c.N, c.P, c.S, c.J, c.Q, c.W, c.D + c.T, c.TL, c.G);
    core->sv_base = base; core->sv_bytes = bytes;
    HIP_TRY(core, hipMemsetAsync(c.sv.xr_key, 0xFF, sizeof(int64_t) * ((size_t)c.sv.xr_mask + 1), core->stream));  // empty residency table
    { int32_t* xg = nullptr; int rcx = dalloc(core, &xg, (size_t)c.sv.xr_mask + 1); if (rcx) return rcx; c.sv.xr_group = xg; core->xr_base = (char*)xg; core->xr_bytes = ((size_t)c.sv.xr_mask + 1) * 4; }
    core->solver_ready = true;
    return KAI_OK;
}

// ---- kai_action_execute in its steps.  What they share: the action, the batch path's verdict, the widths the engine's kernel ran on, the engine's scalars as read back
struct ActionRun { int action; bool victim; BatchStats bs; int g_run = 1, scan_wgs = 1; bool xsh = false; EngineState st{}; };

// a victim action runs on several workgroups, each on a replica of the session arrays made right here (after k_job_init / k_leaf_init on the stream)
int victim_setup(kai_core* core, size_t dyn, ActionRun& r) {
    KaiCtx& c = core->ctx;
    int want = 32; if (const char* e = std::getenv("KAI_VICTIM_WGS")) want = std::atoi(e);  // (measured on C4: 32 workgroups — four replicas per XCD, hot in its L2 — beat 64 and more, whose waves are no shorter)
    const int cus = device_cus(core);
    want = std::max(1, std::min(std::min(want, (int)KAI_MW_MAX), cus));  // every workgroup must be resident: they meet at a grid barrier
    { int per_cu = 0;  // ... as the runtime's occupancy calculation sees it for this kernel, its workgroup size and its dynamic LDS (not only one per compute unit)
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(k_action<true, false>), WG, dyn) == hipSuccess && per_cu > 0) want = std::min(want, per_cu * cus);
      else (void)hipGetLastError(); }
    // a node-sharded group with an exchange for it deals the waves out over its ranks (kai_victim_shard.hpp); every rank takes the same decision here
    r.xsh = core->world > 1 && (core->xag_fn || core->rccl_comm) && !core->shared && want > 1 && (core->mw_world == 0 || core->mw_world == want) && !std::getenv("KAI_VICTIM_REPLICATED");
    if (r.xsh) {
        if (int rcx = xshard_setup(core)) return rcx;
        int cap = xw_default_cap(core->world, want); if (const char* e = std::getenv("KAI_VICTIM_XCAP")) { const int v = std::atoi(e); if (v > 0) cap = std::max(core->world, std::min(v, (int)KAI_MW_WAVE)); }
        c.mw_xworld = core->world; c.mw_xrank = core->rank; c.mw_xcap = cap; c.mw_mail = core->d_mail;
        core->xs.begin(core->world, core->rank, cap);
        __atomic_store_n(&core->mail->req, 0, __ATOMIC_RELEASE); __atomic_store_n(&core->mail->resp, 0, __ATOMIC_RELEASE);
    }
    int rcm = prepare_multi(core, want, &r.g_run);
    c.mw_xworld = 0; c.mw_xrank = 0; c.mw_xcap = 0; c.mw_mail = nullptr;  // (the host copy is what every other kernel of the session gets by value)
    if (rcm) return rcm;
    if (r.xsh && r.g_run <= 1) r.xsh = false;  // (one engine: the action runs replicated; the conditions are the same on every rank — a failed allocation is an error above)
    return KAI_OK;
}
// the allocate action of a large cluster: helper workgroups beside the engine's take the passes over the nodes (ScanGrid, kai_kernels.hpp)
int scan_grid_setup(kai_core* core, ActionRun& r) {
    KaiCtx& c = core->ctx;
    int want = c.N >= 4096 ? 32 : c.N >= 1024 ? 16 : 1; if (const char* e = std::getenv("KAI_SCAN_WGS")) want = std::atoi(e);  // (measured on the mixed config 5 and on config 3 with fractions: 16 .. 32 workgroups are the fastest, 64 and more pay for the table they all watch; from about a thousand nodes a pass on the grid beats one on this workgroup alone: 1 500 nodes 355 -> 303 ms, 2 500: 707 -> 517, 3 500: 1 143 -> 725 per cycle of config 3 with fractions)
    want = std::max(1, std::min(std::min(want, (int)KAI_SG_MAX), device_cus(core) / 2));  // every workgroup must be resident (the control lane waits for the helpers); half the chip leaves room for a neighbour
    if (want <= 1) return KAI_OK;
    if (!core->d_sg) { ScanGrid* g = nullptr; KAI_TRY(dalloc(core, &g, (size_t)1)); core->d_sg = g; }
    HIP_TRY(core, hipMemsetAsync(core->d_sg, 0, sizeof(ScanGrid), core->stream));
    c.sg = core->d_sg; c.sg_wgs = want; c.sg_per = (((c.N + want - 1) / want + 63) / 64) * 64;
    HIP_TRY(core, hipMemcpyAsync(core->d_ctx, &core->ctx, sizeof(KaiCtx), hipMemcpyHostToDevice, core->stream));
    HIP_TRY(core, hipStreamSynchronize(core->stream));
    c.sg = nullptr; c.sg_wgs = 0; c.sg_per = 0;  // (the host copy is what every other kernel of the session gets by value)
    r.scan_wgs = want;
    return KAI_OK;
}
// the sequential engine (k_action): every action the batch path did not run
int action_engine(kai_core* core, ActionRun& r) {
    KaiCtx& c = core->ctx; const bool victim = r.victim;
    if (core->world > 1) {
        // A node-sharded group shards the batch path's fill.  Every other action — sub-group trees, topology, elastic jobs, the victim actions — runs REPLICATED: every rank
        // holds the whole session (only the fill's index is sharded), runs the same engine on it and commits the same operations; nothing is exchanged and nothing gets
        // faster, but a cycle that mixes both kinds of action (BASELINE config 4: allocate, consolidation, reclaim) runs on the group with the one-rank results.
        // The sharded fill left a class index of the own slice only: rebuild it over all nodes first.
        OpenLauncher ol{core}; index_drive(ol, c);
    }
    // dynamic LDS: upper levels of the class index, plus the job-order tree when it fits beside them (160 KiB per CU)
    size_t idx_b = lds_index_bytes(c.C, c.NSB), tree_b = lds_tree_bytes(c.Q);
    const size_t budget = 160 * 1024 - 16384;  // static LDS of the kernel (mailbox, context, engine scalars, frame: 6.8 KB, llvm-readelf .group_segment_fixed_size) + margin
    int tree_in_lds = (idx_b + tree_b <= budget && !std::getenv("KAI_TREE_IN_HBM")) ? 1 : 0;
    size_t dyn = idx_b + (tree_in_lds ? tree_b : 0);
    KAI_TRY(victim ? victim_setup(core, dyn, r) : scan_grid_setup(core, r));
    auto launch = [&](auto kernel) -> int {
        HIP_TRY(core, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
        hipLaunchKernelGGL(kernel, dim3(victim ? r.g_run : r.scan_wgs), dim3(WG), dyn, core->stream, r.g_run > 1 ? (const KaiCtx*)core->d_ctxs : (const KaiCtx*)core->d_ctx, r.action, tree_in_lds, victim ? 1 : r.scan_wgs);
        return KAI_OK;
    };
    KAI_TRY(victim ? launch(k_action<true, false>) : tree_in_lds ? launch(k_action<false, true>) : launch(k_action<false, false>));
    if (r.xsh) { HIP_TRY(core, hipGetLastError()); if (int rcs = xshard_serve(core)) return rcs; }  // the kernel is running: carry its waves' exchanges until it ends
    return KAI_OK;
}
// kai_action_stats from the engine's scalars and the batch path's counters (what reserved[] holds: include/kai_core.h)
int action_stats(kai_core* core, ActionRun& r, float ms) {
    const EngineState& st = r.st; const BatchStats& bs = r.bs; const bool victim = r.victim;
    double upload = core->stats.upload_ms;
    std::memset(&core->stats, 0, sizeof(core->stats));
    core->stats.upload_ms = upload; core->stats.kernel_ms = ms; core->stats.decisions = st.decisions; core->stats.node_scans = st.node_scans;
    core->stats.nodes_scanned = st.nodes_scanned; core->stats.jobs_attempted = st.jobs_attempted; core->stats.jobs_committed = st.jobs_committed; core->stats.rollbacks = st.rollbacks;
    core->stats.reserved[0] = st.index_queries; core->stats.reserved[1] = st.index_refreshes; core->stats.reserved[2] = victim ? st.scenarios : st.drained_jobs; core->stats.reserved[3] = victim ? st.simulations : st.drained_decisions;
    // reserved[4] = plan/fill rounds of the batch path (0 = the sequential engine ran the action); batch path: [5] fill-wave cycles, [6] mispredicted jobs,
    // [7] plan / fill / apply time in microseconds, 21 bits each; sequential engine: [5..7] control-lane cycles allocate / commit+discard / total
    if (bs.ran) {
        core->stats.reserved[4] = bs.rounds; core->stats.reserved[5] = bs.fill_cycles; core->stats.reserved[6] = bs.mismatches;
        auto us = [](double ms) { int64_t v = (int64_t)(ms * 1000.0); return v < 0 ? (int64_t)0 : v > 0x1fffff ? (int64_t)0x1fffff : v; };
        core->stats.reserved[7] = (us(core->batch_plan_ms) << 42) | (us(core->batch_fill_ms) << 21) | us(core->batch_apply_ms);
        core->stats.reserved[1] = (bs.block_loads & ((1ll << 48) - 1)) | ((int64_t)(bs.buckets ? 1 : 0) << 62) | ((int64_t)(bs.buckets >= 2 ? 1 : 0) << 61) | ((int64_t)(bs.buckets == 3 ? 1 : 0) << 60) | ((int64_t)(bs.dev_loop ? 1 : 0) << 59); /* bit 59: the round loop's state lived on the device (rounds without the host), bit 62: the fill ran on the sets by free devices (kai_fill_buckets.hpp), bit 61: behind a counting machine (kai_fill_counts.hpp), bit 60: with a wavefront per level (kai_fill_levels.hpp) */ core->stats.reserved[0] = core->world > 1 ? bs.exchanges : core->stats.reserved[0];
        if (std::getenv("KAI_PROF")) std::fprintf(stderr, "kai batch%s: rounds %lld mismatches %lld planned %lld max_h %d | fill cycles %lld load %lld update %lld rescan %lld | block loads %lld rescans %lld %lld %lld | plan %.3f ms fill %.3f ms apply %.3f ms\n",
            bs.buckets ? " (bucket fill)" : "", (long long)bs.rounds, (long long)bs.mismatches, (long long)bs.planned, bs.max_h, (long long)bs.fill_cycles, (long long)bs.fill_load, (long long)bs.fill_update, (long long)bs.fill_rescan,
            (long long)bs.block_loads, (long long)bs.rescans1, (long long)bs.rescans2, (long long)bs.rescans3, core->batch_plan_ms, core->batch_fill_ms, core->batch_apply_ms);
    } else { core->stats.reserved[4] = 0; core->stats.reserved[5] = st.prof[2]; core->stats.reserved[6] = st.prof[3]; core->stats.reserved[7] = st.prof[7]; }
    if (!victim && !bs.ran && r.scan_wgs > 1) {  // sequential allocate with a scan grid: bits 48.. of [1] = workgroups that took the passes over the nodes (the engine's + the helpers that signed on)
        int32_t nreg = 0; HIP_TRY(core, hipMemcpyAsync(&nreg, &core->d_sg->n_reg, sizeof nreg, hipMemcpyDeviceToHost, core->stream)); HIP_TRY(core, hipStreamSynchronize(core->stream));
        core->stats.reserved[1] |= (int64_t)(nreg + 1) << 48;
        if (std::getenv("KAI_PROF")) std::fprintf(stderr, "kai scan grid: %d workgroups launched, %d helpers signed on\n", r.scan_wgs, nreg);
    }
    if (r.xsh) {  // the action's closing message (every rank sends exactly one; skipped once another rank's was seen): a fault anywhere is everybody's
        DevXIo io{core}; int32_t mfault = 0;
        HIP_TRY(core, hipMemcpyAsync(&mfault, &core->d_mw->fault, 4, hipMemcpyDeviceToHost, core->stream)); HIP_TRY(core, hipStreamSynchronize(core->stream));
        const int rcf = core->xs.finish(io, (st.fault || mfault) ? 1 : 0);
        core->stats.reserved[7] = core->xs.exchanges;  // collectives of this action
        if (rcf && !st.fault) return fail(core, rcf, "victim action of a node-sharded group: another rank ended it with a fault");
    }
    if (victim) {  // victim actions: [1] workgroups the action ran on, [5] waves, [6] simulations run (speculative ones included) << 32 | simulations the reference's order reached; a group that dealt the waves out over its ranks: [7] collectives
        core->stats.reserved[1] = r.g_run;
        if (r.g_run > 1) {
            if (core->mw_host.empty()) core->mw_host.resize(1);
            MultiCtx& m = core->mw_host[0]; HIP_TRY(core, hipMemcpyAsync(&m, core->d_mw, sizeof(MultiCtx), hipMemcpyDeviceToHost, core->stream)); HIP_TRY(core, hipStreamSynchronize(core->stream));
            core->stats.reserved[5] = m.waves; core->stats.reserved[6] = (m.sims_run << 32) | (m.sims_used & 0xffffffffll);
            if (std::getenv("KAI_PROF")) std::fprintf(stderr, "kai victim: %d workgroups, waves %lld, simulations run %lld / counted %lld, replays %lld, fault %d\n", r.g_run, (long long)m.waves, (long long)m.sims_run, (long long)m.sims_used, (long long)m.replays, m.fault);
        }
    }
    return KAI_OK;
}
// the operations to the caller, the nodes as the caller's indices
int action_ops_out(kai_core* core, int64_t out_len, kai_op* ops_out, int64_t ops_cap) {
    if (out_len > ops_cap) return fail(core, KAI_ERR_CAPACITY, "kai_action_execute: ops_cap too small");
    // through the handle's own pinned buffer: a copy of some MB straight into the caller's pageable memory makes the runtime pin and unpin that memory around
    // the transfer, and the unpinning lands in a later call (measured: 22 ms in every other kai_session_reset of the C5 bench, profiles/r04e_*)
    const size_t bytes = (size_t)out_len * sizeof(kai_op);
    KAI_TRY(reserve(core, core->pin_buf, bytes, std::max<size_t>(bytes + bytes / 2, (size_t)1 << 20)));
    if (out_len) HIP_TRY(core, hipMemcpyAsync(core->pin_buf.p, KAI_VP(core->ctx.out_ops), bytes, hipMemcpyDeviceToHost, core->stream));
    HIP_TRY(core, hipStreamSynchronize(core->stream));
    const kai_op* src = reinterpret_cast<const kai_op*>(core->pin_buf.p);
    const int32_t* perm = core->perm.data();
    parallel_chunks((size_t)out_len, [&](int, size_t i0, size_t i1) { for (size_t i = i0; i < i1; i++) { kai_op o = src[i]; if (o.node >= 0) o.node = perm[o.node]; ops_out[i] = o; } });  // name rank → caller's index (config 5: 150 k operations, 4.8 MB)
    return KAI_OK;
}

int action_execute(kai_core* core, int action, kai_op* ops_out, int64_t ops_cap, int64_t* n_ops) {
    const auto ta0 = std::chrono::steady_clock::now();
    KaiCtx& c = core->ctx;
    ActionRun r{action, action != KAI_ACTION_ALLOCATE}; const bool victim = r.victim; EngineState& st = r.st;
    if (victim) KAI_TRY(solver_ensure(core));
    // the context sent, the per-action scalars reset (the proportion totals kept), the class index rebuilt if the last action left it stale, the jobs' and leaves' state
    { int d = core->cfg.queue_depth[action]; c.queue_depth = d > 0 ? d : 0; c.action = action; }
    HIP_TRY(core, hipMemcpyAsync(core->d_ctx, &core->ctx, sizeof(KaiCtx), hipMemcpyHostToDevice, core->stream));
    HIP_TRY(core, hipMemcpyAsync(&st, KAI_VP(c.st), sizeof(st), hipMemcpyDeviceToHost, core->stream));
    HIP_TRY(core, hipStreamSynchronize(core->stream));
    double total[3] = {st.total[0], st.total[1], st.total[2]};
    st = EngineState{}; st.total[0] = total[0]; st.total[1] = total[1]; st.total[2] = total[2];
    HIP_TRY(core, hipMemcpyAsync(KAI_VP(c.st), &st, sizeof(st), hipMemcpyHostToDevice, core->stream));
    HIP_TRY(core, hipEventRecord(core->ev0, core->stream));
    OpenLauncher ol{core};
    action_init_drive(ol, c, core->index_stale);
    core->batch_plan_ms = core->batch_fill_ms = core->batch_apply_ms = 0;
    if (!victim) {  // the batch path (plan / fill / apply rounds, kai_batch.hpp) when the action qualifies
        DevLauncher dl{core};
        int rcb = batch_allocate(dl, c, core->shape, r.bs);
        if (rcb) { if (core->err == "ok") core->err = "batch path failed"; return rcb; }
        if (r.bs.ran && r.bs.buckets) core->index_stale = true;
        if (r.bs.ran && !r.bs.st_on_device) {
            EngineState sb{};
            HIP_TRY(core, hipMemcpyAsync(&sb, KAI_VP(c.st), sizeof(sb), hipMemcpyDeviceToHost, core->stream));
            HIP_TRY(core, hipStreamSynchronize(core->stream));
            sb.decisions += r.bs.decisions; sb.jobs_attempted += r.bs.attempted; sb.jobs_committed += r.bs.committed; sb.rollbacks += r.bs.rollbacks; sb.out_len += r.bs.ops; sb.stmts += r.bs.committed;
            sb.index_queries += r.bs.decisions; sb.drain_pending = r.bs.drain;
            HIP_TRY(core, hipMemcpyAsync(KAI_VP(c.st), &sb, sizeof(sb), hipMemcpyHostToDevice, core->stream));
        }
    }
    const auto ta1 = std::chrono::steady_clock::now();
    if (!r.bs.ran) KAI_TRY(action_engine(core, r));
    if (!victim) drain_drive(ol, c, core->aux);
    HIP_TRY(core, hipGetLastError());
    HIP_TRY(core, hipEventRecord(core->ev1, core->stream));
    HIP_TRY(core, hipMemcpyAsync(&st, KAI_VP(c.st), sizeof(st), hipMemcpyDeviceToHost, core->stream));
    HIP_TRY(core, hipStreamSynchronize(core->stream));
    float ms = 0; HIP_TRY(core, hipEventElapsedTime(&ms, core->ev0, core->ev1));
    KAI_TRY(action_stats(core, r, ms));
    if (std::getenv("KAI_PROF")) { std::fprintf(stderr, "kai prof:"); for (int i = 0; i < KAI_NPROF; i++) std::fprintf(stderr, " %lld", (long long)st.prof[i]); std::fprintf(stderr, "\n"); }
    if (st.non_allocate_commits) c.fast_ok = 0;  // the staged job path assumes nothing releasing / pipelined in the session (kai_host_prep.hpp); until the next open / reset
    if (st.fault) { char buf[96]; std::snprintf(buf, sizeof buf, "device engine fault code %d (engine source line %d)", st.fault, st.fault_line); core->err = buf; return KAI_ERR_DEVICE_FAULT; }
    *n_ops = st.out_len;
    const auto ta2 = std::chrono::steady_clock::now();
    if (ops_out) KAI_TRY(action_ops_out(core, st.out_len, ops_out, ops_cap));
    if (std::getenv("KAI_PROF")) { const auto ta3 = std::chrono::steady_clock::now(); std::fprintf(stderr, "kai action host clocks: setup + batch path %.2f ms, engine / drain / stats %.2f, operations to the caller %.2f | total %.2f ms\n", ms_between(ta0, ta1), ms_between(ta1, ta2), ms_between(ta2, ta3), ms_between(ta0, ta3)); }
    return KAI_OK;
}
}  // namespace
