// kai_session_open.hpp — kai_session_open's host side around the context builder (kai_ctx_build.hpp), the launcher of kai_open_kernels.hpp's sequences (OpenLauncher), the kernels behind the open and the reset (open_kernels), kai_session_reset's body (reset_state).
#pragma once
#include "kai_handle.hpp"
namespace {
// the session-open, action-init and drain kernels on the session's stream (the Launcher of kai_open_kernels.hpp's sequences)
struct OpenLauncher {
    kai_core* core; hipError_t err = hipSuccess;
    template <class P> void fill32(P p, int byte, size_t n) { const hipError_t e = hipMemsetAsync(KAI_VP(p), byte, n * 4, core->stream); if (err == hipSuccess) err = e; }
    void node_accounting(int g, int b, const KaiCtx& c) { hipLaunchKernelGGL(k_node_accounting, dim3(g), dim3(b), 0, core->stream, c); }
    void pod_accounting_reset(int g, int b, const KaiCtx& c) { hipLaunchKernelGGL(k_pod_accounting_reset, dim3(g), dim3(b), 0, core->stream, c); }
    void node_accounting_shared(int g, int b, const KaiCtx& c, const int32_t* np_off, const int32_t* np_pods) { hipLaunchKernelGGL(k_node_accounting_shared, dim3(g), dim3(b), 0, core->stream, c, np_off, np_pods); }
    void total_nodes(int g, int b, const KaiCtx& c) { hipLaunchKernelGGL(k_total_nodes, dim3(g), dim3(b), 0, core->stream, c); }
    void total_foreign(int g, int b, const KaiCtx& c) { hipLaunchKernelGGL(k_total_foreign, dim3(g), dim3(b), 0, core->stream, c); }
    void job_usage(int g, int b, const KaiCtx& c, double* jsum) { hipLaunchKernelGGL(k_job_usage, dim3(g), dim3(b), 0, core->stream, c, jsum); }
    void leaf_usage(int g, int b, const KaiCtx& c, const double* jsum) { hipLaunchKernelGGL(k_leaf_usage, dim3(g), dim3(b), 0, core->stream, c, jsum); }
    void tree_usage(int g, int b, const KaiCtx& c, const int32_t* h_off, const int32_t* h_nodes, int n_h) { hipLaunchKernelGGL(k_tree_usage, dim3(g), dim3(b), 0, core->stream, c, h_off, h_nodes, n_h); }
    void fair_share_level(int g, int b, const KaiCtx& c, const int32_t* lvl_parents, int first, int count, double* weight, double* rem_amt, uint8_t* rem_has) { hipLaunchKernelGGL(k_fair_share_level, dim3(g), dim3(b), 0, core->stream, c, lvl_parents, first, count, weight, rem_amt, rem_has); }
    void qnode_static(int g, int b, const KaiCtx& c) { hipLaunchKernelGGL(k_qnode_static, dim3(g), dim3(b), 0, core->stream, c); }
    void index_build(int g, int b, const KaiCtx& c) { hipLaunchKernelGGL(k_index_build, dim3(g), dim3(b), 0, core->stream, c); }
    void job_init(int g, int b, const KaiCtx& c) { hipLaunchKernelGGL(k_job_init, dim3(g), dim3(b), 0, core->stream, c); }
    void leaf_init(int g, int b, const KaiCtx& c) { hipLaunchKernelGGL(k_leaf_init, dim3(g), dim3(b), 0, core->stream, c); }
    void drain(int g, int b, const KaiCtx& c, const int32_t* slot_queue) { hipLaunchKernelGGL(k_drain, dim3(g), dim3(b), 0, core->stream, c, slot_queue); }
};
// FNV-1a of every array of the session context, a line per KaiCtx field under `prefix` (KAI_OPEN_DIGEST; tests/test_open_uploads.py, tests/test_gpu_open_digest.py)
int open_digest(kai_core* core, const char* prefix) {
    HIP_TRY(core, hipStreamSynchronize(core->stream));
    for (const kai_core::AllocRec& a : core->allocs) {
        std::vector<unsigned char> h(a.bytes);
        HIP_TRY(core, hipMemcpyAsync(h.data(), a.base, a.bytes, hipMemcpyDeviceToHost, core->stream)); HIP_TRY(core, hipStreamSynchronize(core->stream));
        uint64_t f = 1469598103934665603ull; for (unsigned char x : h) { f ^= x; f *= 1099511628211ull; }
        std::fprintf(stderr, "%s: field %zu bytes %zu fnv %016llx\n", prefix, a.field_off, a.bytes, (unsigned long long)f);
    }
    return KAI_OK;
}
// session-open kernels over the HBM-resident snapshot (used by kai_session_open and kai_session_reset)
int open_kernels(kai_core* core) {
    OpenLauncher l{core};
    open_drive(l, core->ctx, core->aux, OpenShape{core->n_levels, core->h_lvl_off.data(), core->n_heights, core->cfg.plugins, core->shared});
    HIP_TRY(core, l.err); HIP_TRY(core, hipGetLastError());
    core->index_stale = false;
    return KAI_OK;
}
// ---- kai_session_open: session_open_impl below is the checks, the context builder's calls (kai_ctx_build.hpp), the handle's bookkeeping, the baselines and the kernels
// checks: the dimensions, the required arrays, the fallback rules on the pods' flags, the shared-GPU model's own refusals (SharedPods)
int open_checks(kai_core* core, const kai_snapshot_soa* s, bool& any_legacy_mig) {
    const int N = s->n_nodes, P = s->n_pods, S = s->n_podsets, J = s->n_jobs, Q = s->n_queues;
    if (N < 0 || P < 0 || S < 0 || J < 0 || Q < 0) return fail(core, KAI_ERR_INVALID_ARG, "negative dimension");
    if (const char* m = HostPrep::missing_array(s)) return fail(core, KAI_ERR_INVALID_ARG, m);  // (before anything reads the snapshot's arrays; HostPrep::build reports the same)
    if (s->pod_flags) {  // one pass over the pods' flags on the host's cores: the two fallback rules (the first one wins, as when checked one after the other) and whether any pod is a legacy MIG task
        const int K = chunk_count((size_t)P);
        std::vector<unsigned char> seen((size_t)K, 0);
        parallel_chunks((size_t)P, [&](int ci, size_t p0, size_t p1) {
            unsigned char f = 0;
            for (size_t p = p0; p < p1; p++) {
                const uint32_t fl = s->pod_flags[p];
                if (!(fl & (KAI_POD_CPU_FALLBACK | KAI_POD_GPU_UNMODELLED | KAI_POD_LEGACY_MIG))) continue;
                if ((fl & KAI_POD_CPU_FALLBACK) && s->pod_status[p] == KAI_POD_PENDING) f |= 1;
                if ((fl & KAI_POD_GPU_UNMODELLED) && (s->pod_status[p] & KAI_POD_ACTIVE)) f |= 2;
                if (fl & KAI_POD_LEGACY_MIG) f |= 4;
            }
            seen[(size_t)ci] = f;
        });
        unsigned char all = 0; for (unsigned char f : seen) all |= f;
        if (all & 1) return fail(core, KAI_ERR_UNSUPPORTED, "a pending pod is flagged KAI_POD_CPU_FALLBACK: leave its job to the host path");
        if (all & 2) return fail(core, KAI_ERR_UNSUPPORTED, "an active pod holds GPU state the device does not model (gpu-memory / several fractional devices / MIG / DRA): its node's idle GPUs would be overstated");
        any_legacy_mig = all & 4;
    }
    // shared GPUs (ABI v4): fractions of one device.  One GPU memory size for the whole cluster keeps the queue-capacity step node independent.
    SharedPods& sp = core->sp;
    try { if (!sp.build(core->cfg, s)) return fail(core, KAI_ERR_UNSUPPORTED, sp.err.c_str()); }
    catch (const std::bad_alloc&) { throw; }  // (kai_session_open reports it as what it is)
    catch (const std::exception& e) { core->err = std::string("host preparation: ") + e.what(); return KAI_ERR_INVALID_ARG; }
    core->shared = sp.any;
    return KAI_OK;
}
// what the handle keeps beside the context the builder filled (kai_ctx_build.hpp), most of it for kai_session_update
void open_bookkeeping(kai_core* core, const kai_snapshot_soa* s, CtxBuildOut& built) {
    KaiCtx& c = core->ctx; HostPrep& prep = core->prep; const int N = c.N, P = c.P;
    core->n_levels = prep.n_levels; core->h_lvl_off = prep.lvl_off; core->n_heights = prep.n_heights;
    core->solver_ready = false; core->cls_cap = std::max(c.C, 1); core->shape = prep.shape;
    core->fast_ok0 = c.fast_ok; core->idx_forced_off = built.idx_forced_off; core->fast_forced_off = built.fast_forced_off;
    core->next_group0 = built.next_group; core->new_groups.clear();
    for (int32_t g : built.groups) if (g >= KAI_NEW_GROUP) core->new_groups[g]++;
    core->gm_guard = core->shared && s->node_gpu_memory != nullptr;
    core->h_gpu_mem.swap(built.gpu_mem);
    // (kai_session_update edits these lists by the delta: every pod's UID rank, each node's list with the ranks)
    core->np_uid.clear(); core->np_lists.clear(); core->np_cap = built.np_pods.size();
    if (core->shared) {
        core->np_uid.assign(s->pod_uid_rank, s->pod_uid_rank + P); core->np_lists.assign((size_t)N, {});
        for (int n = 0; n < N; n++) for (int k = built.np_off[n]; k < built.np_off[n + 1]; k++) core->np_lists[(size_t)n].push_back({s->pod_uid_rank[built.np_pods[k]], built.np_pods[k]});
    }
}
// the batch path's pools, the initial state kept in HBM for kai_session_reset, the context
int open_baselines(kai_core* core) {
    KaiCtx& c = core->ctx; const int P = c.P, Q = c.Q;
    // batch path of the allocate action (kai_batch.hpp): its pools and tables, when the snapshot admits it
    KAI_TRY(bind_batch_pools(core));
    if (core->shared) c.bt.enabled = 0;
    // keep the initial dynamic state in HBM so that kai_session_reset needs no host traffic
    KAI_TRY(dalloc(core, &core->d_status0, (size_t)P)); KAI_TRY(dalloc(core, &core->d_node0, (size_t)P)); KAI_TRY(dalloc(core, &core->d_shares0, (size_t)std::max(Q, 1) * 3));
    if (P) { HIP_TRY(core, hipMemcpyAsync(core->d_status0, KAI_VP(c.p_status), (size_t)P * 4, hipMemcpyDeviceToDevice, core->stream));
             HIP_TRY(core, hipMemcpyAsync(core->d_node0, KAI_VP(c.p_node), (size_t)P * 4, hipMemcpyDeviceToDevice, core->stream)); }
    HIP_TRY(core, hipMemcpyAsync(core->d_shares0, KAI_VP(c.q_share), (size_t)std::max(Q, 1) * 3 * sizeof(QShare), hipMemcpyDeviceToDevice, core->stream));
    { KaiCtx* t = nullptr; KAI_TRY(dalloc(core, &t, (size_t)1)); core->d_ctx = t; }
    HIP_TRY(core, hipMemcpyAsync(core->d_ctx, &core->ctx, sizeof(KaiCtx), hipMemcpyHostToDevice, core->stream));
    return KAI_OK;
}
// slabs of earlier (larger) sessions this open did not take: keep two for what the session's actions still allocate (solver scratch, batch pools), release the rest
// ... and the smallest one that holds the LARGEST request the last session made after its open (post_open_max: a victim action's replicas, the batch pools) — or that request
// would pay a hipMalloc every cycle and a hipFree at the next trim, which is what keeping slabs is there to avoid
void trim_spare(kai_core* core) {
    if (core->spare.size() > 2) {
        std::sort(core->spare.begin(), core->spare.end(), [](const std::pair<void*, size_t>& a, const std::pair<void*, size_t>& b) { return a.second < b.second; });
        size_t keep_big = core->spare.size();
        for (size_t i = 2; i < core->spare.size(); i++) if (core->post_open_max > 0 && core->spare[i].second >= core->post_open_max) { keep_big = i; break; }
        if (core->post_open_max > 0 && (core->spare[0].second >= core->post_open_max || core->spare[1].second >= core->post_open_max)) keep_big = core->spare.size();  // (one of the two small ones already holds it)
        std::vector<std::pair<void*, size_t>> kept;
        for (size_t i = 0; i < core->spare.size(); i++) { if (i < 2 || i == keep_big) kept.push_back(core->spare[i]); else (void)hipFree(core->spare[i].first); }
        core->spare.swap(kept);
    }
}

int session_open_impl(kai_core* core, const kai_snapshot_soa* s) {
    if (s->abi_version != KAI_ABI_VERSION || s->n_res < 4 || s->n_res > KAI_MAX_RES) return fail(core, KAI_ERR_INVALID_ARG, "bad abi_version / n_res");
    HIP_TRY(core, hipSetDevice(core->device));
    const bool prof_open = std::getenv("KAI_PROF") != nullptr;  // host clocks of the open: where a production cycle's per-cycle cost goes (stderr)
    auto tnow = [] { return std::chrono::steady_clock::now(); };
    const auto t_begin = tnow();
    free_session(core);
    const auto t_freed = tnow();
    bool any_legacy_mig = false;
    KAI_TRY(open_checks(core, s, any_legacy_mig));
    HIP_TRY(core, hipEventRecord(core->ev0, core->stream));
    KaiCtx& c = core->ctx; DevArena arena{core};
    ctx_scalars(c, core->cfg, s);
    const auto t_shared = tnow();
    KAI_TRY(ctx_stage_snapshot(arena, c, s));  // (sent from pinned staging while the host preparation runs: UploadStage)
    // ---- index structures (pure re-orderings / groupings of the input; kai_host_prep.hpp)
    const auto t_staged = tnow();
    HostPrep& prep = core->prep; SharedPods& sp = core->sp;
    prep.shared_pods = sp.any ? &sp : nullptr;
    try { if (prep.build(core->cfg, s, core->err)) return KAI_ERR_INVALID_ARG; }  // (the staged copies read the handle's pinned buffer: kai_session_open drains the stream on every failure)
    catch (const std::bad_alloc&) { throw; }  // (a worker thread's included: kai_parallel.hpp carries it here)
    catch (const std::exception& e) { core->err = std::string("host preparation: ") + e.what(); return KAI_ERR_INVALID_ARG; }
    const auto t_prep = tnow();
    core->legacy_on = any_legacy_mig; core->legacy_cnt.clear();
    if (any_legacy_mig) flag_legacy_mig_nodes(s, prep, core->legacy_cnt);
    core->perm = prep.perm; core->bn_perm_ok = false; core->sp_perm_ok = false; core->oa_rank_ok = false; core->sn_tab_ok = false; core->sn_shape_ok = false;

    // the context's arrays (kai_ctx_build.hpp; the order of its allocations is the session's layout in HBM), then what is the handle's own
    CtxBuildOut built;
    KAI_TRY(ctx_build(arena, c, core->aux, CtxBuildIn{core->cfg, s, prep, sp, std::getenv("KAI_OPEN_FULL_UPLOADS") != nullptr, 1}, built));
    open_bookkeeping(core, s, built);
    KAI_TRY(open_baselines(core));
    const bool digest = std::getenv("KAI_OPEN_DIGEST") != nullptr;  // diagnostic: what the open put into every array of the session context before its first kernel, and what its kernels left
    if (digest) KAI_TRY(open_digest(core, "kai open digest"));
    KAI_TRY(open_kernels(core));
    HIP_TRY(core, hipEventRecord(core->ev1, core->stream));
    const auto t_enq = tnow();
    HIP_TRY(core, hipStreamSynchronize(core->stream));  // prep's host buffers die with this scope
    if (digest) KAI_TRY(open_digest(core, "kai open digest behind the kernels"));
    if (prof_open) std::fprintf(stderr, "kai open: free %.2f ms, checks + shared pods %.2f, the snapshot's arrays staged %.2f, host prep %.2f, allocate + enqueue uploads %.2f, wait %.2f | total %.2f ms\n",
                                ms_between(t_begin, t_freed), ms_between(t_freed, t_shared), ms_between(t_shared, t_staged), ms_between(t_staged, t_prep), ms_between(t_prep, t_enq), ms_between(t_enq, tnow()), ms_between(t_begin, tnow()));
    if (prof_open) std::fprintf(stderr, "kai open: host prep by phase: range checks %.2f, nodes %.2f, pods %.2f, task order %.2f, queues + job lists %.2f, shares + topology %.2f, classes %.2f, batch shape %.2f ms on %d host threads\n",
                                prep.phase_ms[0], prep.phase_ms[1], prep.phase_ms[2], prep.phase_ms[3], prep.phase_ms[4], prep.phase_ms[5], prep.phase_ms[6], prep.phase_ms[7], host_threads());
    float ms = 0; HIP_TRY(core, hipEventElapsedTime(&ms, core->ev0, core->ev1));
    std::memset(&core->stats, 0, sizeof(core->stats));
    core->stats.upload_ms = ms;
    trim_spare(core);
    core->post_open_max = 0;  // (counted from here on: dalloc)
    core->open = true; core->st_open = false; core->err = "ok";
    return KAI_OK;
}
// the session's dynamic state from the HBM-resident snapshot: kai_session_reset, and kai_session_update after its scatter
int reset_state(kai_core* core) {
    KaiCtx& c = core->ctx;
    const size_t RN = (size_t)c.R * c.N;
    HIP_TRY(core, hipEventRecord(core->ev0, core->stream));
    if (RN) { HIP_TRY(core, hipMemcpyAsync(KAI_VP(c.n_idle), KAI_VP(c.n_alloc), RN * 8, hipMemcpyDeviceToDevice, core->stream));
              HIP_TRY(core, hipMemsetAsync(KAI_VP(c.n_rel), 0, RN * 8, core->stream)); HIP_TRY(core, hipMemsetAsync(KAI_VP(c.n_used), 0, RN * 8, core->stream)); }
    if (c.P) { HIP_TRY(core, hipMemcpyAsync(KAI_VP(c.p_status), core->d_status0, (size_t)c.P * 4, hipMemcpyDeviceToDevice, core->stream));
               HIP_TRY(core, hipMemcpyAsync(KAI_VP(c.p_node), core->d_node0, (size_t)c.P * 4, hipMemcpyDeviceToDevice, core->stream)); }
    HIP_TRY(core, hipMemcpyAsync(KAI_VP(c.q_share), core->d_shares0, (size_t)std::max(c.Q, 1) * 3 * sizeof(QShare), hipMemcpyDeviceToDevice, core->stream));
    c.fast_ok = core->fast_ok0; core->st_open = false;  // (an open Statement goes with everything else the reset drops)
    if (c.P) HIP_TRY(core, hipMemcpyAsync(KAI_VP(c.p_group), core->aux.group0, (size_t)c.P * 4, hipMemcpyDeviceToDevice, core->stream));
    HIP_TRY(core, hipMemcpyAsync(KAI_VP(c.next_new_group), &core->next_group0, 4, hipMemcpyHostToDevice, core->stream));
    { const size_t NG = (size_t)std::max(c.N, 1) * KAI_GMAX;
      HIP_TRY(core, hipMemsetAsync(KAI_VP(c.ng_used), 0, NG * 8, core->stream)); HIP_TRY(core, hipMemsetAsync(KAI_VP(c.ng_rel), 0, NG * 8, core->stream)); HIP_TRY(core, hipMemsetAsync(KAI_VP(c.ng_alloc), 0, NG * 8, core->stream));
      HIP_TRY(core, hipMemsetAsync(KAI_VP(c.ng_mark), 0, (size_t)std::max(c.N, 1) * 4, core->stream)); HIP_TRY(core, hipMemsetAsync(KAI_VP(c.ng_has_alloc), 0, (size_t)std::max(c.N, 1) * 4, core->stream)); }
    if (core->solver_ready) HIP_TRY(core, hipMemsetAsync(c.sv.xr_key, 0xFF, sizeof(int64_t) * ((size_t)c.sv.xr_mask + 1), core->stream));
    HIP_TRY(core, hipMemsetAsync(KAI_VP(c.st), 0, sizeof(EngineState), core->stream));
    KAI_TRY(open_kernels(core));
    HIP_TRY(core, hipEventRecord(core->ev1, core->stream));
    HIP_TRY(core, hipStreamSynchronize(core->stream));
    float ms = 0; HIP_TRY(core, hipEventElapsedTime(&ms, core->ev0, core->ev1));
    core->stats.upload_ms = ms;
    return KAI_OK;
}
}  // namespace
