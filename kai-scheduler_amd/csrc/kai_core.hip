// kai_core.hip — C ABI of libkai_core (include/kai_core.h) on top of the gfx950 kernels: the library's one translation unit.  The entry points are here; what they
// share is in the headers included below, in dependency order (the handle, RCCL, the open and the reset, the update, the actions).
//
// Host code here only moves the snapshot into HBM, derives index structures that are pure re-orderings / groupings of the input (kai_host_prep.hpp: nodes in name-rank
// order, CSR children, per-queue job lists, each job's pods in TaskOrderFn order, scan classes), launches the kernels and copies results back.  There is NO CPU
// implementation of the path in this library: without a HIP device every entry point fails with KAI_ERR_NO_DEVICE.
#define KAI_SHARED_GPUS 1  // fractions of one device (ABI v4): group tables per node, gpusharingorder score, FittingGPUs (kai_engine.hpp)
#include "kai_handle.hpp"
#include "kai_rccl.hpp"
#include "kai_session_open.hpp"
#include "kai_session_update.hpp"
#include "kai_action.hpp"

extern "C" {

const char* kai_version(void) { return "kai_core abi 5 gfx950 (HIP; batch plan/fill/apply path, node-axis sharding, device-resident sequential engine, class index)"; }

const char* kai_last_error(kai_core* core) { return core ? core->err.c_str() : "null handle"; }

int kai_core_create(const kai_config* cfg, int n_gpus, const int* gpu_ids, kai_core** out) {
    if (!cfg || !out || cfg->abi_version != KAI_ABI_VERSION || n_gpus < 1) return KAI_ERR_INVALID_ARG;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return KAI_ERR_NO_DEVICE;
    int dev = gpu_ids ? gpu_ids[0] : 0;
    if (dev < 0 || dev >= count) return KAI_ERR_INVALID_ARG;
    kai_core* core = new kai_core();
    core->cfg = *cfg; core->device = dev; core->world = n_gpus;  // n_gpus > 1: this handle is ONE rank of a node-sharded group (kai_shard_attach names the rank)
    if (hipSetDevice(dev) != hipSuccess || hipStreamCreateWithFlags(&core->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&core->ev0) != hipSuccess || hipEventCreate(&core->ev1) != hipSuccess || hipEventCreate(&core->bev[0]) != hipSuccess ||
        hipEventCreate(&core->bev[1]) != hipSuccess || hipEventCreate(&core->bev[2]) != hipSuccess || hipEventCreate(&core->bev[3]) != hipSuccess) {
        delete core;
        return KAI_ERR_HIP;
    }
    *out = core;
    return KAI_OK;
}

int kai_core_destroy(kai_core* core) {
    if (!core) return KAI_ERR_INVALID_ARG;
    (void)hipSetDevice(core->device);
    free_session(core, true);
    if (core->up_pin.p) (void)hipStreamSynchronize(core->stream);  // (a staged copy of the last open may still read it)
    if (core->rccl_comm) { (void)hipStreamSynchronize(core->stream); if (RcclApi* a = rccl_api()) (void)a->CommDestroy(core->rccl_comm); core->rccl_comm = nullptr; }
    for (HandleBuf* b : core->handle_bufs()) b->release();
    if (core->mail) (void)hipHostFree(core->mail);
    if (core->xstream) (void)hipStreamDestroy(core->xstream);
    for (hipEvent_t e : {core->ev0, core->ev1}) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : core->bev) if (e) (void)hipEventDestroy(e);
    for (auto& slot : core->rev) for (hipEvent_t e : slot) if (e) (void)hipEventDestroy(e);
    if (core->stream) (void)hipStreamDestroy(core->stream);
    delete core;
    return KAI_OK;
}

int kai_session_close(kai_core* core) {
    if (!core) return KAI_ERR_INVALID_ARG;
    (void)hipSetDevice(core->device);
    free_session(core);
    return KAI_OK;
}

// Nothing leaves this function by an exception (the host preparation's loops allocate: std::bad_alloc, also from a worker thread — kai_parallel.hpp carries it here — and
// std::system_error from thread creation), and every failure takes ONE way out: the stream is drained — the staged copies read the handle's pinned buffer, which the next open
// writes again — and the slabs this open took go back to the handle, so that a failed open leaves the handle as a closed session does.
int kai_session_open(kai_core* core, const kai_snapshot_soa* s) {
    if (!core || !s) return KAI_ERR_INVALID_ARG;
    const int rc = no_throw(core, "kai_session_open", [&] { return session_open_impl(core, s); });
    if (rc != KAI_OK) close_failed(core);
    return rc;
}

int kai_session_reset(kai_core* core) {
    if (!core) return KAI_ERR_INVALID_ARG;
    if (!core->open) return fail(core, KAI_ERR_STATE, "no open session");
    HIP_TRY(core, hipSetDevice(core->device));
    return reset_state(core);
}

int kai_session_update(kai_core* core, const kai_session_delta* d) {
    if (!core) return KAI_ERR_INVALID_ARG;
    if (!d) return fail(core, KAI_ERR_INVALID_ARG, "kai_session_update: NULL delta");
    return session_update(core, d, nullptr, "kai_session_update");
}

int kai_session_update_rows(kai_core* core, const kai_session_delta* delta, const kai_session_rows* rows) {
    if (!core) return KAI_ERR_INVALID_ARG;
    return session_update(core, delta, rows, "kai_session_update_rows");
}

// The cycle's clock.  Every action sends the context again (kai_action_execute) and builds the replicas' contexts from it (prepare_multi), so the handle's copy is the one
// that counts; the device copy follows for whatever reads it before the next action.
int kai_core_set_now(kai_core* core, int64_t now_ns) {
    if (!core) return KAI_ERR_INVALID_ARG;
    core->cfg.now_ns = now_ns;
    if (!core->open) return KAI_OK;
    core->ctx.now_ns = now_ns;
    HIP_TRY(core, hipSetDevice(core->device));
    HIP_TRY(core, hipMemcpyAsync(core->d_ctx, &core->ctx, sizeof(KaiCtx), hipMemcpyHostToDevice, core->stream));
    HIP_TRY(core, hipStreamSynchronize(core->stream));
    return KAI_OK;
}

int kai_queue_shares(kai_core* core, kai_queue_share* out, int cap) {
    if (!core || !out) return KAI_ERR_INVALID_ARG;
    if (!core->open) return fail(core, KAI_ERR_STATE, "no open session");
    const int Q = core->ctx.Q;
    if (cap < Q) return fail(core, KAI_ERR_CAPACITY, "kai_queue_shares: cap < n_queues");
    HIP_TRY(core, hipSetDevice(core->device));
    std::vector<QShare> h((size_t)std::max(Q, 1) * 3);
    HIP_TRY(core, hipMemcpyAsync(h.data(), KAI_VP(core->ctx.q_share), (size_t)Q * 3 * sizeof(QShare), hipMemcpyDeviceToHost, core->stream));
    HIP_TRY(core, hipStreamSynchronize(core->stream));
    for (int q = 0; q < Q; q++) for (int k = 0; k < 3; k++) {
        const QShare& x = h[(size_t)q * 3 + k];
        out[q].fair_share[k] = x.fair; out[q].allocated[k] = x.allocated; out[q].allocated_non_preemptible[k] = x.allocated_np;
        out[q].request[k] = x.request; out[q].deserved[k] = x.deserved; out[q].max_allowed[k] = x.max_allowed;
    }
    return KAI_OK;
}

int kai_action_execute(kai_core* core, int action, kai_op* ops_out, int64_t ops_cap, int64_t* n_ops) {
    if (!core || !n_ops) return KAI_ERR_INVALID_ARG;
    if (!core->open) return fail(core, KAI_ERR_STATE, "no open session");
    if (action < KAI_ACTION_ALLOCATE || action > KAI_ACTION_PREEMPT) return fail(core, KAI_ERR_INVALID_ARG, "unknown action");
    if (core->st_open) return fail(core, KAI_ERR_STATE, "kai_action_execute: a Statement is open (kai_stmt_commit or kai_stmt_discard first)");
    if (action != KAI_ACTION_ALLOCATE && core->cfg.use_scheduling_signatures && !core->ctx.j_signature && core->ctx.J > 0) return fail(core, KAI_ERR_UNSUPPORTED, "use_scheduling_signatures needs kai_snapshot_soa.job_signature (actions/common/minimal_job_comparison.go)");
    HIP_TRY(core, hipSetDevice(core->device));
    return action_execute(core, action, ops_out, ops_cap, n_ops);
}

int kai_best_node(kai_core* core, int32_t pod_idx, const uint32_t* nodeset_bitmap, int pipeline_only, int32_t* node_idx_out, int* is_pipeline_out) {
    if (!core || !node_idx_out) return KAI_ERR_INVALID_ARG;
    if (!core->open) return fail(core, KAI_ERR_STATE, "no open session");
    if (pod_idx < 0 || pod_idx >= core->ctx.P) return fail(core, KAI_ERR_INVALID_ARG, "pod index out of range");
    HIP_TRY(core, hipSetDevice(core->device));
    uint32_t* d_bits = nullptr;
    if (nodeset_bitmap) {  // caller's node indices → engine order (name rank), then to HBM for this call
        const int N = core->ctx.N, W = (N + 31) / 32;
        std::vector<uint32_t> bits((size_t)std::max(W, 1), 0u);
        for (int i = 0; i < N; i++) { int o = core->perm[i]; if ((nodeset_bitmap[o >> 5] >> (o & 31)) & 1u) bits[i >> 5] |= 1u << (i & 31); }
        HIP_TRY(core, hipMalloc(reinterpret_cast<void**>(&d_bits), bits.size() * 4));
        HIP_TRY(core, hipMemcpyAsync(d_bits, bits.data(), bits.size() * 4, hipMemcpyHostToDevice, core->stream));
        HIP_TRY(core, hipStreamSynchronize(core->stream));
    }
    hipLaunchKernelGGL(k_best_node, dim3(1), dim3(WG), 16, core->stream, core->ctx, (int)pod_idx, pipeline_only, core->aux.best_out, (const uint32_t*)d_bits);
    HIP_TRY(core, hipGetLastError());
    int32_t h[2] = {-1, 0};
    HIP_TRY(core, hipMemcpyAsync(h, core->aux.best_out, sizeof h, hipMemcpyDeviceToHost, core->stream));
    HIP_TRY(core, hipStreamSynchronize(core->stream));
    if (d_bits) (void)hipFree(d_bits);
    *node_idx_out = h[0] >= 0 ? core->perm[h[0]] : -1;
    if (is_pipeline_out) *is_pipeline_out = h[1];
    return KAI_OK;
}

// What kai_best_nodes, kai_ordered_nodes and kai_ordered_nodes_scored refuse alike, in one pass and before the first device call.  *empty: an accepted call without queries
// (KAI_OK, nothing to do).  n_score_rows >= 0: the queries are kai_scored_query (the same layout): the fourth word names a score row, -1 = none, instead of being a pad.
static int bn_check(kai_core* core, const char* who, const kai_node_query* queries, int32_t n_queries, const uint32_t* nodeset_bitmaps, int32_t n_nodesets, bool out_null, bool* empty, int32_t n_score_rows = -1) {
    auto no = [&](int code, const char* why) { core->err = std::string(who) + ": " + why; return code; };
    *empty = false;
    if (n_queries < 0 || n_nodesets < 0) return no(KAI_ERR_INVALID_ARG, "a negative count");
    if (n_queries > 0 && (!queries || out_null)) return no(KAI_ERR_INVALID_ARG, "queries / out is NULL");
    if (n_nodesets > 0 && !nodeset_bitmaps) return no(KAI_ERR_INVALID_ARG, "nodeset_bitmaps is NULL");
    if (core->world > 1) return no(KAI_ERR_UNSUPPORTED, "a handle of a sharded group");
    if (!core->open) return fail(core, KAI_ERR_STATE, "no open session");
    if (n_queries == 0) { *empty = true; return KAI_OK; }
    const int P = core->ctx.P, S = n_nodesets;
    for (int i = 0; i < n_queries; i++) {
        const kai_node_query& q = queries[i];
        if (q.pod < 0 || q.pod >= P) return no(KAI_ERR_INVALID_ARG, "pod index out of range");
        if (q.nodeset < -1 || q.nodeset >= S) return no(KAI_ERR_INVALID_ARG, "nodeset outside -1 .. n_nodesets-1");
        if (q.flags & ~KAI_QUERY_PIPELINE_ONLY) return no(KAI_ERR_INVALID_ARG, "unknown flag bits");
        if (n_score_rows < 0 ? q.pad != 0 : (q.pad < -1 || q.pad >= n_score_rows)) return no(KAI_ERR_INVALID_ARG, n_score_rows < 0 ? "pad is not zero" : "scores outside -1 .. n_score_rows-1");
    }
    return KAI_OK;
}

// The part of a call the two share: the handle's scratch (dev_bytes) and staging ([what is sent][down_bytes of answers]) grown on demand — the only allocations, none once the
// handle is warm —, ONE staging upload and the launches of k_bn_prep and k_bn_range.  The permutation lies at offset 0 of the scratch whichever of the two calls sized it.
static int bn_stage(kai_core* core, const BnLayout& L, size_t dev_bytes, size_t down_bytes, const kai_node_query* queries, const uint32_t* nodeset_bitmaps, int M, int S, int W, BnArgs& a,
                    const void* extra0 = nullptr, size_t extra0_bytes = 0, const void* extra1 = nullptr, size_t extra1_bytes = 0) {
    const int N = core->ctx.N;
    bool grew = false;
    KAI_TRY(reserve(core, core->bn_dev, dev_bytes, std::max<size_t>(dev_bytes + dev_bytes / 2, (size_t)1 << 16), &grew));
    if (grew) core->bn_perm_ok = false;  // (the new scratch does not hold the permutation)
    const size_t pin_need = L.up_end + down_bytes + 16;
    KAI_TRY(reserve(core, core->bn_pin, pin_need, std::max<size_t>(pin_need + pin_need / 2, (size_t)1 << 16)));
    // ---- one staging upload: [queries | rows | zeroed need flags], behind the permutation when the scratch does not hold this session's yet
    unsigned char* h = core->bn_pin.p; unsigned char* d = core->bn_dev.p;
    const size_t up0 = core->bn_perm_ok ? L.queries : L.perm;
    if (!core->bn_perm_ok && N > 0) std::memcpy(h + L.perm, core->perm.data(), (size_t)N * 4);
    std::memcpy(h + L.queries, queries, (size_t)M * sizeof(kai_node_query));
    if (S > 0 && W > 0) std::memcpy(h + L.rows_in, nodeset_bitmaps, (size_t)S * W * 4);
    std::memset(h + L.need, 0, L.up_end - L.need);
    if (extra0_bytes) std::memcpy(h + L.extra, extra0, extra0_bytes);  // (what a scored call sends on top: [score rows | deciles], in the same copy)
    if (extra1_bytes) std::memcpy(h + L.extra + ((extra0_bytes + 15) & ~(size_t)15), extra1, extra1_bytes);
    HIP_TRY(core, hipMemcpyAsync(d + up0, h + up0, L.up_end - up0, hipMemcpyHostToDevice, core->stream));
    core->bn_perm_ok = true;
    a = BnArgs{};
    a.M = M; a.S = S; a.W = W;
    a.queries = (KAI_GP(const kai_node_query))(d + L.queries); a.rows_in = (KAI_GP(const uint32_t))(d + L.rows_in); a.perm = (KAI_GP(const int32_t))(d + L.perm);
    a.rows = (KAI_GP(uint32_t))(d + L.rows); a.need = (KAI_GP(int32_t))(d + L.need); a.range = (KAI_GP(double))(d + L.range);
    a.prep = (KAI_GP(BnQuery))(d + L.prep); a.out = (KAI_GP(kai_node_answer))(d + L.out);
    const size_t prep_items = std::max<size_t>((size_t)M, (size_t)S * W);
    hipLaunchKernelGGL(k_bn_prep, dim3((unsigned)((prep_items + KAI_BN_WG - 1) / KAI_BN_WG)), dim3(KAI_BN_WG), 0, core->stream, core->ctx, a);
    HIP_TRY(core, hipGetLastError());
    const bool binpack = (core->ctx.plugins & KAI_PLUGIN_NODEPLACEMENT) && (core->ctx.gpu_strategy == KAI_BINPACK || core->ctx.cpu_strategy == KAI_BINPACK);
    if (binpack) {  // NodePreOrderFn exists with a bin-pack strategy only; workgroups of pairs no query needs leave at once
        hipLaunchKernelGGL(k_bn_range, dim3((unsigned)(2 * (S + 1))), dim3(KAI_BN_WG), 0, core->stream, core->ctx, a);
        HIP_TRY(core, hipGetLastError());
    }
    return KAI_OK;
}

int kai_best_nodes(kai_core* core, const kai_node_query* queries, int32_t n_queries, const uint32_t* nodeset_bitmaps, int32_t n_nodesets, kai_node_answer* out) {
    // every refusal before the first device call; `out` is written only after the answers came back
    if (!core) return KAI_ERR_INVALID_ARG;
    bool empty = false;
    KAI_TRY(bn_check(core, "kai_best_nodes", queries, n_queries, nodeset_bitmaps, n_nodesets, !out, &empty));
    if (empty) return KAI_OK;
    const int N = core->ctx.N, M = n_queries, S = n_nodesets, W = (N + 31) / 32;
    HIP_TRY(core, hipSetDevice(core->device));
    const BnLayout L(N, M, S, W);
    const int cus = device_cus(core);
    BnArgs a;
    KAI_TRY(bn_stage(core, L, L.end, (size_t)M * sizeof(kai_node_answer), queries, nodeset_bitmaps, M, S, W, a));  // the upload and two of the three launches
    const int grid = std::min(M, cus * KAI_BN_WGS_PER_CU);
    hipLaunchKernelGGL(k_bn_scan, dim3((unsigned)grid), dim3(KAI_BN_WG), 0, core->stream, core->ctx, a);
    HIP_TRY(core, hipGetLastError());
    // ---- one download, one synchronise
    unsigned char* h_out = core->bn_pin.p + L.up_end;
    HIP_TRY(core, hipMemcpyAsync(h_out, core->bn_dev.p + L.out, (size_t)M * sizeof(kai_node_answer), hipMemcpyDeviceToHost, core->stream));
    HIP_TRY(core, hipStreamSynchronize(core->stream));
    std::memcpy(out, h_out, (size_t)M * sizeof(kai_node_answer));
    return KAI_OK;
}

int kai_ordered_nodes(kai_core* core, const kai_node_query* queries, int32_t n_queries, const uint32_t* nodeset_bitmaps, int32_t n_nodesets, int32_t k,
                      kai_node_answer* out, int32_t* n_out) {
    // every refusal before the first device call; `out` and `n_out` are written only after the lists came back
    if (!core) return KAI_ERR_INVALID_ARG;
    if (k < 1 || k > KAI_ORDERED_MAX_K) return fail(core, KAI_ERR_INVALID_ARG, "kai_ordered_nodes: k outside 1 .. KAI_ORDERED_MAX_K");
    bool empty = false;
    KAI_TRY(bn_check(core, "kai_ordered_nodes", queries, n_queries, nodeset_bitmaps, n_nodesets, !out || !n_out, &empty));
    if (empty) return KAI_OK;
    if ((int64_t)n_queries * k > ((int64_t)1 << 27)) return fail(core, KAI_ERR_CAPACITY, "kai_ordered_nodes: n_queries * k above 2^27");
    const int N = core->ctx.N, M = n_queries, S = n_nodesets, W = (N + 31) / 32;
    HIP_TRY(core, hipSetDevice(core->device));
    const OnLayout L(N, M, S, W, k);
    const int cus = device_cus(core);
    BnArgs a;
    KAI_TRY(bn_stage(core, L, L.on_end, L.down_bytes(M, k), queries, nodeset_bitmaps, M, S, W, a));  // the upload and two of the three launches
    OnArgs o{};
    o.k = k; o.out = (KAI_GP(kai_node_answer))(core->bn_dev.p + L.lists); o.n_out = (KAI_GP(int32_t))(core->bn_dev.p + L.n_out);
    const int grid = std::min(M, cus * KAI_BN_WGS_PER_CU);
    hipLaunchKernelGGL(k_on_scan, dim3((unsigned)grid), dim3(KAI_BN_WG), 0, core->stream, core->ctx, a, o);
    HIP_TRY(core, hipGetLastError());
    // ---- one download ([the lists | their lengths]), one synchronise
    unsigned char* h_out = core->bn_pin.p + L.up_end;
    HIP_TRY(core, hipMemcpyAsync(h_out, core->bn_dev.p + L.lists, L.down_bytes(M, k), hipMemcpyDeviceToHost, core->stream));
    HIP_TRY(core, hipStreamSynchronize(core->stream));
    std::memcpy(out, h_out, (size_t)M * k * sizeof(kai_node_answer));
    std::memcpy(n_out, h_out + (L.n_out - L.lists), (size_t)M * 4);
    return KAI_OK;
}

int kai_ordered_nodes_scored(kai_core* core, const kai_scored_query* queries, int32_t n_queries, const uint32_t* nodeset_bitmaps, int32_t n_nodesets,
                             const kai_topo_score_row* score_rows, const uint8_t* deciles, int32_t n_score_rows, int32_t k, kai_node_answer* out, int32_t* n_out) {
    // every refusal before the first device call; `out` and `n_out` are written only after the lists came back
    if (!core) return KAI_ERR_INVALID_ARG;
    if (k < 1 || k > KAI_ORDERED_MAX_K) return fail(core, KAI_ERR_INVALID_ARG, "kai_ordered_nodes_scored: k outside 1 .. KAI_ORDERED_MAX_K");
    if (n_score_rows < 0) return fail(core, KAI_ERR_INVALID_ARG, "kai_ordered_nodes_scored: a negative n_score_rows");
    if (n_score_rows > 0 && (!score_rows || !deciles)) return fail(core, KAI_ERR_INVALID_ARG, "kai_ordered_nodes_scored: score_rows / deciles is NULL");
    bool empty = false;
    const kai_node_query* nq = reinterpret_cast<const kai_node_query*>(queries);  // (the same layout: kai_ordered_nodes.hpp asserts it)
    KAI_TRY(bn_check(core, "kai_ordered_nodes_scored", nq, n_queries, nodeset_bitmaps, n_nodesets, !out || !n_out, &empty, n_score_rows));
    const int D = core->ctx.D, TL = core->ctx.TL;
    for (int s = 0; s < n_score_rows; s++) {  // one host pass over the rows
        if (score_rows[s].level_row < KAI_TOPO_SCORES_EMPTY || score_rows[s].level_row >= TL) return fail(core, KAI_ERR_INVALID_ARG, "kai_ordered_nodes_scored: a level_row outside -2 .. n_topo_levels-1");
        const uint8_t* row = deciles + (size_t)s * D;
        for (int d = 0; d < D; d++) if (row[d] > 10 && row[d] != KAI_TOPO_NO_SCORE) return fail(core, KAI_ERR_INVALID_ARG, "kai_ordered_nodes_scored: a decile that is neither <= 10 nor 255");
    }
    if (empty) return KAI_OK;
    if ((int64_t)n_queries * k > ((int64_t)1 << 27)) return fail(core, KAI_ERR_CAPACITY, "kai_ordered_nodes_scored: n_queries * k above 2^27");
    if ((int64_t)n_score_rows * (D + 8) > ((int64_t)1 << 30)) return fail(core, KAI_ERR_CAPACITY, "kai_ordered_nodes_scored: n_score_rows x (n_domains + 8) above 2^30");
    const int N = core->ctx.N, M = n_queries, S = n_nodesets, W = (N + 31) / 32;
    HIP_TRY(core, hipSetDevice(core->device));
    const size_t row_bytes = (size_t)n_score_rows * sizeof(kai_topo_score_row), dec_bytes = (size_t)n_score_rows * D, dec_off = (row_bytes + 15) & ~(size_t)15;
    const OnLayout L(N, M, S, W, k, dec_off + dec_bytes);
    const int cus = device_cus(core);
    BnArgs a;
    KAI_TRY(bn_stage(core, L, L.on_end, L.down_bytes(M, k), nq, nodeset_bitmaps, M, S, W, a, score_rows, row_bytes, deciles, dec_bytes));  // the upload and two of the three launches
    OnArgs o{};
    o.k = k; o.out = (KAI_GP(kai_node_answer))(core->bn_dev.p + L.lists); o.n_out = (KAI_GP(int32_t))(core->bn_dev.p + L.n_out);
    OnScoreArgs sa{};
    sa.D = D; sa.rows = (KAI_GP(const kai_topo_score_row))(core->bn_dev.p + L.extra); sa.deciles = (KAI_GP(const uint8_t))(core->bn_dev.p + L.extra + dec_off);
    const int grid = std::min(M, cus * KAI_BN_WGS_PER_CU);
    hipLaunchKernelGGL(k_on_scan_scored, dim3((unsigned)grid), dim3(KAI_BN_WG), 0, core->stream, core->ctx, a, o, sa);
    HIP_TRY(core, hipGetLastError());
    // ---- one download ([the lists | their lengths]), one synchronise
    unsigned char* h_out = core->bn_pin.p + L.up_end;
    HIP_TRY(core, hipMemcpyAsync(h_out, core->bn_dev.p + L.lists, L.down_bytes(M, k), hipMemcpyDeviceToHost, core->stream));
    HIP_TRY(core, hipStreamSynchronize(core->stream));
    std::memcpy(out, h_out, (size_t)M * k * sizeof(kai_node_answer));
    std::memcpy(n_out, h_out + (L.n_out - L.lists), (size_t)M * 4);
    return KAI_OK;
}

// kai_ops_apply's kernels and its verdict's download for oa_drive (kai_ops_apply.hpp); pin: where the verdict lands in the handle's staging
struct OaLauncher {
    kai_core* core; unsigned char* pin;
    void check(int g, int b, const KaiCtx& c, const OaArgs& a) { hipLaunchKernelGGL(k_oa_check, dim3((unsigned)g), dim3((unsigned)b), 0, core->stream, c, a); }
    void wide(int g, int b, const KaiCtx& c, const OaArgs& a) { hipLaunchKernelGGL(k_oa_wide, dim3((unsigned)g), dim3((unsigned)b), 0, core->stream, c, a); }
    int engine(const KaiCtx&, const OaArgs& a) {
        if (!(a.flags & KAI_APPLY_CHECK_ONLY)) { const int rcs = solver_ensure(core); if (rcs) return rcs; }  // (binds core->ctx.sv: the context is read after it)
        hipLaunchKernelGGL(k_oa_engine, dim3(1), dim3(64), 0, core->stream, core->ctx, a);
        return KAI_OK;
    }
    int read_head(OaHead& hv, const OaArgs& a) {
        HIP_TRY(core, hipGetLastError());
        HIP_TRY(core, hipMemcpyAsync(pin, (const void*)a.head, sizeof(OaHead), hipMemcpyDeviceToHost, core->stream));
        HIP_TRY(core, hipStreamSynchronize(core->stream));
        std::memcpy(&hv, pin, sizeof(OaHead));
        return KAI_OK;
    }
};

// kai_ops_apply's device scratch for n operations of the open session (OaLayout(core->oa_pod_cap, n) afterwards): grows on demand, no allocation once the handle is warm
static int oa_reserve_scratch(kai_core* core, int n) {
    const int P = core->ctx.P;
    const size_t pod_cap = std::max(std::max<size_t>((size_t)P + (size_t)P / 4, 1024), core->oa_pod_cap);
    const OaLayout G(pod_cap, (int64_t)n + n / 2 + 1024);  // the enlarged capacities: what a growth allocates
    bool grew = false;  // (per-pod arrays that no longer hold the session's pods force the growth whatever the bytes)
    KAI_TRY(reserve(core, core->oa_dev, (size_t)P > core->oa_pod_cap ? SIZE_MAX : OaLayout(core->oa_pod_cap, n).end, G.end, &grew));
    if (grew) { core->oa_pod_cap = pod_cap; HIP_TRY(core, hipMemsetAsync(core->oa_dev.p, 0, G.head, core->stream)); }  // the per-pod arrays: zero between calls (the kernels clean what they touch)
    return KAI_OK;
}

int kai_ops_apply(kai_core* core, const kai_op* ops, int64_t n_ops, uint32_t flags, kai_apply_result* result) {
    // every host-decidable refusal before the first device call; `result` always leaves with a defined content
    kai_apply_result res; res.first_bad = -1; res.path = KAI_APPLY_PATH_NONE; res.statements = 0;
    if (result) *result = res;
    if (!core) return KAI_ERR_INVALID_ARG;
    if (n_ops < 0) return fail(core, KAI_ERR_INVALID_ARG, "kai_ops_apply: a negative count");
    if (flags & ~(KAI_APPLY_CHECK_ONLY | KAI_APPLY_ENGINE_PATH)) return fail(core, KAI_ERR_INVALID_ARG, "kai_ops_apply: unknown flag bits");
    if (n_ops > 0 && !ops) return fail(core, KAI_ERR_INVALID_ARG, "kai_ops_apply: ops is NULL");
    if (core->world > 1) return fail(core, KAI_ERR_UNSUPPORTED, "kai_ops_apply: a handle of a sharded group");
    if (!core->open) return fail(core, KAI_ERR_STATE, "no open session");
    if (core->shared) return fail(core, KAI_ERR_UNSUPPORTED, "kai_ops_apply: a session with shared-GPU requests (kai_op carries no GPU group)");
    if (core->st_open) return fail(core, KAI_ERR_STATE, "kai_ops_apply: a Statement is open (kai_stmt_commit or kai_stmt_discard first)");
    if (n_ops == 0) return KAI_OK;
    if (n_ops > (int64_t)0x7fffffff - 16) return fail(core, KAI_ERR_CAPACITY, "kai_ops_apply: more than 2^31 - 16 operations");
    KaiCtx& c = core->ctx;
    const int N = c.N, P = c.P, n = (int)n_ops;
    bool non_alloc = false; int statements = 1;
    for (int i = 0; i < n; i++) {  // O(n): what no device is needed for
        const kai_op& o = ops[i];
        const char* why = nullptr;
        if (o.kind < KAI_OP_ALLOCATE || o.kind > KAI_OP_EVICT) why = "kai_ops_apply: kind outside 0..2";
        else if (o.pod < 0 || o.pod >= P) why = "kai_ops_apply: pod index out of range";
        else if (o.node < 0 || o.node >= N) why = "kai_ops_apply: node index out of range";
        else if (o.pad != 0) why = "kai_ops_apply: pad is not zero";
        else if (i > 0 && o.stmt < ops[i - 1].stmt) why = "kai_ops_apply: stmt decreases";
        if (why) { if (result) result->first_bad = i; return fail(core, KAI_ERR_INVALID_ARG, why); }
        if (o.kind != KAI_OP_ALLOCATE) non_alloc = true;
        if (i > 0 && o.stmt != ops[i - 1].stmt) statements++;
    }
    res.statements = statements;
    HIP_TRY(core, hipSetDevice(core->device));
    // ---- the handle's scratch and staging: grow on demand, no allocation once the handle is warm
    KAI_TRY(oa_reserve_scratch(core, n));
    const OaLayout L(core->oa_pod_cap, n);
    const size_t up_bytes = L.end - L.head, pin_need = up_bytes + sizeof(OaHead);  // [head | ops][the verdict]
    KAI_TRY(reserve(core, core->oa_pin, pin_need, std::max<size_t>(pin_need + pin_need / 2, (size_t)1 << 16)));
    if (!core->oa_rank_ok) { core->oa_rank.assign((size_t)std::max(N, 1), 0); for (int i = 0; i < N; i++) core->oa_rank[(size_t)core->perm[i]] = i; core->oa_rank_ok = true; }
    // ---- one staging upload: [head | ops], the nodes as name ranks
    unsigned char* h = core->oa_pin.p; unsigned char* d = core->oa_dev.p;
    OaHead* hh = reinterpret_cast<OaHead*>(h); std::memset(hh, 0, sizeof(OaHead)); hh->bad = KAI_OA_NONE;
    {   kai_op* dst = reinterpret_cast<kai_op*>(h + sizeof(OaHead)); const int32_t* rank = core->oa_rank.data();
        parallel_chunks((size_t)n, [&](int, size_t i0, size_t i1) { for (size_t i = i0; i < i1; i++) { kai_op o = ops[i]; o.node = rank[o.node]; dst[i] = o; } }); }
    HIP_TRY(core, hipMemcpyAsync(d + L.head, h, up_bytes, hipMemcpyHostToDevice, core->stream));
    OaArgs a{};
    a.n = n; a.flags = flags | (oa_wide_session(c) ? 0u : KAI_OA_NOT_WIDE); a.use_islot = oa_use_islot(c);
    a.ops = (KAI_GP(const kai_op))(d + L.ops); a.head = (KAI_GP(OaHead))(d + L.head);
    a.stamp = (KAI_GP(int32_t))(d + L.stamp); a.sh_status = (KAI_GP(int32_t))(d + L.sh_status); a.sh_node = (KAI_GP(int32_t))(d + L.sh_node);
    // ---- the check and the chip-wide apply, one small download, one synchronise; the engine walk and a second download where the batch needs it (oa_drive)
    OaLauncher launcher{core, h + up_bytes};
    OaHead hv{}; int path = KAI_APPLY_PATH_NONE;
    const int rcd = oa_drive(launcher, core->ctx, a, KAI_OA_WG, hv, path);
    if (rcd == KAI_ERR_STATE) {
        if (result) result->first_bad = hv.bad;
        return fail(core, KAI_ERR_STATE, "kai_ops_apply: an operation's precondition fails (ALLOCATE: a Pending pod; PIPELINE: Pending or Releasing; EVICT: a pod on op.node)");
    }
    if (rcd == KAI_ERR_DEVICE_FAULT) { char buf[160]; std::snprintf(buf, sizeof buf, "kai_ops_apply: device engine fault code %d (engine source line %d), path %d reported %d", hv.fault, hv.fault_line, path, hv.applied); core->err = buf; return rcd; }
    if (rcd) return rcd;
    res.path = path;
    if (!(flags & KAI_APPLY_CHECK_ONLY)) {
        core->index_stale = true;           // neither path keeps the class index (sum1_key / sum1_node): rebuilt before the next action reads it
        if (non_alloc) c.fast_ok = 0;       // something is releasing / pipelined in the session from here on, as after an action that committed such operations
    }
    if (result) *result = res;
    return KAI_OK;
}

// kai_stmt_*'s kernels for st_apply_drive / st_range_drive (kai_stmt.hpp), on top of the apply's launcher (the check kernel and the verdict's download are kai_ops_apply's)
struct StLauncher : OaLauncher {
    static dim3 g(int n) { return dim3((unsigned)n); }
    void apply(int n, int b, const KaiCtx& c, const StArgs& s) { hipLaunchKernelGGL(k_st_apply, g(n), g(b), 0, core->stream, c, s); }
    void undo(int n, int b, const KaiCtx& c, const StArgs& s) { hipLaunchKernelGGL(k_st_undo, g(n), g(b), 0, core->stream, c, s); }
    void commit(int n, int b, const KaiCtx& c, const StArgs& s) { hipLaunchKernelGGL(k_st_commit, g(n), g(b), 0, core->stream, c, s); }
    int engine(const KaiCtx&, const StArgs& s) {
        if (!(s.a.flags & KAI_APPLY_CHECK_ONLY)) { const int rcs = solver_ensure(core); if (rcs) return rcs; }  // (binds core->ctx.sv: the context is read after it)
        hipLaunchKernelGGL(k_st_engine, dim3(1), dim3(64), 0, core->stream, core->ctx, s);
        return KAI_OK;
    }
};
enum : uint8_t { ST_REC_KIND = 3, ST_REC_WIDE = 4 };  // kai_core::st_rec

// what every kai_stmt_* call refuses before anything else; open_wanted: the call needs an open Statement (begin: none)
static int st_entry(kai_core* core, const char* what, bool open_wanted, kai_stmt_result* result) {
    if (result) { result->first_bad = -1; result->log_len = core && core->st_open ? (int64_t)core->st_rec.size() : 0; result->path = KAI_APPLY_PATH_NONE; result->pad = 0; }
    if (!core) return KAI_ERR_INVALID_ARG;
    auto say = [&](int code, const char* why) { core->err = std::string(what) + ": " + why; return code; };
    if (core->world > 1) return say(KAI_ERR_UNSUPPORTED, "a handle of a sharded group");
    if (!core->open) return fail(core, KAI_ERR_STATE, "no open session");
    if (core->shared) return say(KAI_ERR_UNSUPPORTED, "a session with shared-GPU requests (kai_op carries no GPU group)");
    if (open_wanted && !core->st_open) return say(KAI_ERR_STATE, "no open Statement (kai_stmt_begin)");
    if (!open_wanted && core->st_open) return say(KAI_ERR_STATE, "a Statement is open already");
    return KAI_OK;
}
// the arguments every call's kernels share: the Statement's stamps and verdict, the log as the host counts it
static StArgs st_args(kai_core* core, int mode) {
    const StLayout L(core->st_pod_cap); unsigned char* d = core->st_dev.p;
    StArgs s{};
    s.a.flags = oa_wide_session(core->ctx) ? 0u : KAI_OA_NOT_WIDE; s.a.use_islot = oa_use_islot(core->ctx);
    s.a.head = (KAI_GP(OaHead))(d + L.head); s.a.stamp = (KAI_GP(int32_t))(d + L.stamp);
    s.len = (int32_t)core->st_rec.size(); s.mode = mode;
    return s;
}
static int st_device_fault(kai_core* core, const char* what, const OaHead& hv) {
    char buf[200]; std::snprintf(buf, sizeof buf, "%s: device engine fault code %d (engine source line %d), path reported %d; the Statement is closed", what, hv.fault, hv.fault_line, hv.applied);
    core->err = buf; core->st_open = false; return KAI_ERR_DEVICE_FAULT;
}
// any other failure behind the first launch (a HIP error, the solver scratch): the stamps and the log on the device may no longer be what the host counted — the Statement
// is closed, the call's own status and message stay
static int st_lost(kai_core* core, int rc) { core->st_open = false; core->err += "; the Statement is closed"; return rc; }

int kai_stmt_begin(kai_core* core, uint32_t version) {
    KAI_TRY(st_entry(core, "kai_stmt_begin", false, nullptr));
    if (version != KAI_STMT_VERSION) return fail(core, KAI_ERR_INVALID_ARG, "kai_stmt_begin: wrong version");
    KaiCtx& c = core->ctx;
    HIP_TRY(core, hipSetDevice(core->device));
    // the Statement's own memory: the stamps of this session's pods and the verdict.  Grows here and nowhere else
    const size_t P = (size_t)c.P, room = (size_t)st_log_room(c);
    if (P > core->st_pod_cap || !core->st_dev.p) {
        const size_t pod_cap = std::max(std::max<size_t>(P + P / 4, 1024), core->st_pod_cap);
        KAI_TRY(reserve(core, core->st_dev, SIZE_MAX, StLayout(pod_cap).end));
        core->st_pod_cap = pod_cap;
    }
    const StLayout L(core->st_pod_cap);
    KAI_TRY(reserve(core, core->st_pin, 2 * sizeof(OaHead), (size_t)1 << 16));  // [the verdict up | the verdict down | the committed operations: grown by the commit]
    HIP_TRY(core, hipMemsetAsync(core->st_dev.p + L.stamp, 0, std::max<size_t>(P, 1) * 4, core->stream));  // no pod is named yet
    HIP_TRY(core, hipMemsetAsync(KAI_VP(c.st), 0, 2 * sizeof(int32_t), core->stream));                      // EngineState::ops_len, n_undo: the log is empty
    static_assert(offsetof(EngineState, ops_len) == 0 && offsetof(EngineState, n_undo) == 4, "the log's length and its undo count lead EngineState");
    core->st_rec.clear(); core->st_rec.reserve(room);
    core->st_open = true;
    return KAI_OK;
}

int kai_stmt_apply(kai_core* core, const kai_op* ops, int64_t n_ops, uint32_t flags, kai_stmt_result* result) {
    // every host-decidable refusal before the first device call; `result` always leaves with a defined content
    KAI_TRY(st_entry(core, "kai_stmt_apply", true, result));
    if (n_ops < 0) return fail(core, KAI_ERR_INVALID_ARG, "kai_stmt_apply: a negative count");
    if (flags & ~(KAI_APPLY_CHECK_ONLY | KAI_APPLY_ENGINE_PATH)) return fail(core, KAI_ERR_INVALID_ARG, "kai_stmt_apply: unknown flag bits");
    if (n_ops > 0 && !ops) return fail(core, KAI_ERR_INVALID_ARG, "kai_stmt_apply: ops is NULL");
    if (n_ops == 0) return KAI_OK;
    KaiCtx& c = core->ctx;
    const int N = c.N, P = c.P;
    const int64_t len = (int64_t)core->st_rec.size();
    if (len + n_ops > (int64_t)st_log_room(c)) return fail(core, KAI_ERR_CAPACITY, "kai_stmt_apply: the log would exceed its room (ops_cap / 2 = 2 n_pods + 32 records: a rollback pushes one undo record per undone operation)");
    const int n = (int)n_ops;
    for (int i = 0; i < n; i++) {  // O(n): what no device is needed for
        const kai_op& o = ops[i];
        const char* why = nullptr;
        if (o.kind < KAI_OP_ALLOCATE || o.kind > KAI_OP_EVICT) why = "kai_stmt_apply: kind outside 0..2";
        else if (o.pod < 0 || o.pod >= P) why = "kai_stmt_apply: pod index out of range";
        else if (o.node < 0 || o.node >= N) why = "kai_stmt_apply: node index out of range";
        else if (o.pad != 0) why = "kai_stmt_apply: pad is not zero";
        if (why) { if (result) result->first_bad = i; return fail(core, KAI_ERR_INVALID_ARG, why); }
    }
    HIP_TRY(core, hipSetDevice(core->device));
    // ---- kai_ops_apply's scratch and staging for the batch and the shadow (the stamps are the Statement's own: a growth here loses nothing)
    KAI_TRY(oa_reserve_scratch(core, n));
    const OaLayout L(core->oa_pod_cap, n);
    const size_t up_bytes = L.end - L.head, pin_need = up_bytes + sizeof(OaHead);  // [head | ops][the verdict]
    KAI_TRY(reserve(core, core->oa_pin, pin_need, std::max<size_t>(pin_need + pin_need / 2, (size_t)1 << 16)));
    if (!core->oa_rank_ok) { core->oa_rank.assign((size_t)std::max(N, 1), 0); for (int i = 0; i < N; i++) core->oa_rank[(size_t)core->perm[i]] = i; core->oa_rank_ok = true; }
    // ---- one staging upload: [head | ops], the nodes as name ranks
    unsigned char* h = core->oa_pin.p; unsigned char* d = core->oa_dev.p;
    OaHead* hh = reinterpret_cast<OaHead*>(h); std::memset(hh, 0, sizeof(OaHead)); hh->bad = KAI_OA_NONE;
    {   kai_op* dst = reinterpret_cast<kai_op*>(h + sizeof(OaHead)); const int32_t* rank = core->oa_rank.data();
        parallel_chunks((size_t)n, [&](int, size_t i0, size_t i1) { for (size_t i = i0; i < i1; i++) { kai_op o = ops[i]; o.node = rank[o.node]; dst[i] = o; } }); }
    HIP_TRY(core, hipMemcpyAsync(d + L.head, h, up_bytes, hipMemcpyHostToDevice, core->stream));
    StArgs s = st_args(core, KAI_ST_APPLY);
    s.a.n = n; s.a.flags |= flags;
    s.a.ops = (KAI_GP(const kai_op))(d + L.ops); s.a.head = (KAI_GP(OaHead))(d + L.head);
    s.a.sh_status = (KAI_GP(int32_t))(d + L.sh_status); s.a.sh_node = (KAI_GP(int32_t))(d + L.sh_node);
    // ---- the check and the chip-wide apply, one small download, one synchronise; the engine walk and a second download where the batch needs it
    StLauncher launcher{{core, h + up_bytes}};
    OaHead hv{}; int path = KAI_APPLY_PATH_NONE;
    const int rcd = st_apply_drive(launcher, core->ctx, s, KAI_OA_WG, hv, path);
    if (rcd == KAI_ERR_STATE) {
        if (result) result->first_bad = hv.bad;
        return fail(core, KAI_ERR_STATE, "kai_stmt_apply: an operation's precondition fails (ALLOCATE: a Pending pod; PIPELINE: Pending or Releasing; EVICT: a pod on op.node)");
    }
    if (rcd == KAI_ERR_DEVICE_FAULT) return st_device_fault(core, "kai_stmt_apply", hv);
    if (rcd) return st_lost(core, rcd);
    if (!(flags & KAI_APPLY_CHECK_ONLY)) {
        const uint8_t wide = path == KAI_APPLY_PATH_WIDE ? ST_REC_WIDE : 0;
        for (int i = 0; i < n; i++) core->st_rec.push_back((uint8_t)ops[i].kind | wide);
        core->index_stale = true;  // neither path keeps the class index: rebuilt before the next action reads it
    }
    if (result) { result->path = path; result->log_len = (int64_t)core->st_rec.size(); }
    return KAI_OK;
}

int kai_stmt_checkpoint(kai_core* core, int64_t* cp_out) {
    KAI_TRY(st_entry(core, "kai_stmt_checkpoint", true, nullptr));
    if (!cp_out) return fail(core, KAI_ERR_INVALID_ARG, "kai_stmt_checkpoint: cp_out is NULL");
    *cp_out = (int64_t)core->st_rec.size();
    return KAI_OK;
}

// rollback (close = false) and discard (cp = 0, close = true): the records [cp, len) undone, chip-wide where the host knows every one of them `wide`
static int st_rollback(kai_core* core, const char* what, int64_t cp, uint32_t flags, bool close, kai_stmt_result* result) {
    KAI_TRY(st_entry(core, what, true, result));
    auto say = [&](int code, const char* why) { core->err = std::string(what) + ": " + why; return code; };
    if (flags & ~KAI_APPLY_ENGINE_PATH) return say(KAI_ERR_INVALID_ARG, "unknown flag bits");
    const int64_t len = (int64_t)core->st_rec.size();
    if (cp < 0 || cp > len) return say(KAI_ERR_INVALID_ARG, "cp outside 0 .. log_len");
    if (cp == len) { if (close) core->st_open = false; if (result && close) result->log_len = 0; return KAI_OK; }  // nothing to undo: no launch
    bool wide = !(flags & KAI_APPLY_ENGINE_PATH) && oa_wide_session(core->ctx);
    for (int64_t i = cp; i < len && wide; i++) wide = (core->st_rec[(size_t)i] & ST_REC_WIDE) != 0;
    HIP_TRY(core, hipSetDevice(core->device));
    StArgs s = st_args(core, close ? KAI_ST_DISCARD : KAI_ST_ROLLBACK);
    s.cp = (int32_t)cp;
    unsigned char* h = core->st_pin.p;
    OaHead* hh = reinterpret_cast<OaHead*>(h); std::memset(hh, 0, sizeof(OaHead)); hh->bad = KAI_OA_NONE;
    HIP_TRY(core, hipMemcpyAsync((void*)s.a.head, h, sizeof(OaHead), hipMemcpyHostToDevice, core->stream));
    StLauncher launcher{{core, h + sizeof(OaHead)}};
    OaHead hv{}; int path = KAI_APPLY_PATH_NONE;
    const int rcd = st_range_drive(launcher, core->ctx, s, KAI_OA_WG, wide, hv, path);
    if (rcd == KAI_ERR_DEVICE_FAULT) return st_device_fault(core, what, hv);
    if (rcd) return st_lost(core, rcd);
    core->st_rec.resize((size_t)cp);
    core->index_stale = true;
    if (close) core->st_open = false;
    if (result) { result->path = path; result->log_len = cp; }
    return KAI_OK;
}
int kai_stmt_rollback(kai_core* core, int64_t cp, uint32_t flags, kai_stmt_result* result) { return st_rollback(core, "kai_stmt_rollback", cp, flags, false, result); }
int kai_stmt_discard(kai_core* core, uint32_t flags, kai_stmt_result* result) { return st_rollback(core, "kai_stmt_discard", 0, flags, true, result); }

int kai_stmt_commit(kai_core* core, kai_op* ops_out, int64_t ops_cap, int64_t* n_ops, kai_stmt_result* result) {
    KAI_TRY(st_entry(core, "kai_stmt_commit", true, result));
    if (ops_cap < 0 || (ops_cap > 0 && !ops_out)) return fail(core, KAI_ERR_INVALID_ARG, "kai_stmt_commit: a negative capacity, or ops_out is NULL");
    const int64_t len = (int64_t)core->st_rec.size();
    if (ops_out && ops_cap < len) { if (n_ops) *n_ops = len; return fail(core, KAI_ERR_CAPACITY, "kai_stmt_commit: ops_cap is below the number of surviving operations (*n_ops holds it)"); }
    if (n_ops) *n_ops = len;
    if (len == 0) { core->st_open = false; if (result) result->log_len = 0; return KAI_OK; }  // nothing survived: no launch
    KaiCtx& c = core->ctx;
    bool wide = oa_wide_session(c), non_alloc = false;
    for (uint8_t r : core->st_rec) { if (!(r & ST_REC_WIDE)) wide = false; if ((r & ST_REC_KIND) != KAI_OP_ALLOCATE) non_alloc = true; }
    HIP_TRY(core, hipSetDevice(core->device));
    // the committed operations: a device buffer and, where the caller wants them, pinned staging; grow on demand, no allocation once the handle is warm
    const size_t out_bytes = (size_t)len * sizeof(kai_op), pin_need = 2 * sizeof(OaHead) + (ops_out ? out_bytes : 0);
    KAI_TRY(reserve(core, core->st_out, out_bytes, out_bytes + out_bytes / 2 + 1024 * sizeof(kai_op)));
    KAI_TRY(reserve(core, core->st_pin, pin_need, pin_need + pin_need / 2));
    StArgs s = st_args(core, KAI_ST_COMMIT);
    s.out = (KAI_GP(kai_op))core->st_out.p; s.out_cap = len;
    unsigned char* h = core->st_pin.p;
    OaHead* hh = reinterpret_cast<OaHead*>(h); std::memset(hh, 0, sizeof(OaHead)); hh->bad = KAI_OA_NONE;
    HIP_TRY(core, hipMemcpyAsync((void*)s.a.head, h, sizeof(OaHead), hipMemcpyHostToDevice, core->stream));
    StLauncher launcher{{core, h + sizeof(OaHead)}};
    unsigned char* h_ops = h + 2 * sizeof(OaHead);
    OaHead hv{}; int path = KAI_APPLY_PATH_NONE;
    // (the operations ride in front of the verdict on the same stream: read_head's synchronise covers both)
    struct WithOps : StLauncher { unsigned char* h_ops; const StArgs* s; size_t bytes; bool want;
        int read_head(OaHead& hv_, const OaArgs& a) { if (want) HIP_TRY(core, hipMemcpyAsync(h_ops, (const void*)s->out, bytes, hipMemcpyDeviceToHost, core->stream)); return StLauncher::read_head(hv_, a); } };
    WithOps wl{launcher, h_ops, &s, (size_t)len * sizeof(kai_op), ops_out != nullptr};
    const int rcd = st_range_drive(wl, core->ctx, s, KAI_OA_WG, wide, hv, path);
    if (rcd == KAI_ERR_DEVICE_FAULT) return st_device_fault(core, "kai_stmt_commit", hv);
    if (rcd) return st_lost(core, rcd);
    if (ops_out) { const kai_op* src = reinterpret_cast<const kai_op*>(h_ops); const int32_t* perm = core->perm.data();  // name rank -> the caller's node index
        parallel_chunks((size_t)len, [&](int, size_t i0, size_t i1) { for (size_t i = i0; i < i1; i++) { kai_op o = src[i]; o.node = perm[o.node]; ops_out[i] = o; } }); }
    core->index_stale = true;
    if (non_alloc) c.fast_ok = 0;  // something is releasing / pipelined in the session from here on, as after kai_ops_apply of such operations
    core->st_rec.clear(); core->st_open = false;
    if (result) { result->path = path; result->log_len = 0; }
    return KAI_OK;
}

int kai_stmt_place(kai_core* core, const kai_place_params* params, const kai_place_gang* gangs, int32_t n_gangs, const int32_t* tasks, int32_t n_tasks, const int32_t* sets, int32_t n_sets,
                   const uint32_t* nodeset_bitmaps, int32_t n_nodesets, const kai_topo_score_row* score_rows, const uint8_t* deciles, int32_t n_score_rows,
                   kai_place_answer* answers_out, int32_t* fail_at_out, kai_op* ops_out, int64_t ops_cap, int64_t* n_ops, kai_stmt_result* result) {
    // every host-decidable refusal before the first device call; `result` always leaves with a defined content, the outputs are written only after the answers came back
    KAI_TRY(st_entry(core, "kai_stmt_place", true, result));
    auto no = [&](int code, const char* why) { core->err = std::string("kai_stmt_place: ") + why; return code; };
    if (!params || params->version != KAI_PLACE_VERSION) return no(KAI_ERR_INVALID_ARG, "NULL params or a wrong version");
    if (params->flags & ~(KAI_APPLY_ENGINE_PATH | KAI_PLACE_PIPELINE_ONLY)) return no(KAI_ERR_INVALID_ARG, "unknown flag bits");
    if (n_gangs < 0 || n_tasks < 0 || n_sets < 0 || n_nodesets < 0 || n_score_rows < 0 || ops_cap < 0) return no(KAI_ERR_INVALID_ARG, "a negative count or capacity");
    if ((n_gangs > 0 && (!gangs || !answers_out)) || (n_tasks > 0 && (!tasks || !ops_out)) || (n_sets > 0 && !sets) || (n_nodesets > 0 && !nodeset_bitmaps) || (n_score_rows > 0 && (!score_rows || !deciles)))
        return no(KAI_ERR_INVALID_ARG, "a NULL array with a count above 0");
    KaiCtx& c = core->ctx;
    const int N = c.N, P = c.P, D = c.D, TL = c.TL, W = (N + 31) / 32, G = n_gangs, T = n_tasks, S = n_sets, R = n_nodesets;
    int64_t work = 0;
    std::vector<uint8_t> covered((size_t)T, 0);  // a task belongs to one gang: a pod placed by one gang is no longer Pending for the next
    for (int g = 0; g < G; g++) {
        const kai_place_gang& x = gangs[g];
        if (x.pad != 0) return no(KAI_ERR_INVALID_ARG, "pad is not zero");
        if (x.n_tasks < 1 || x.n_sets < 1) return no(KAI_ERR_INVALID_ARG, "a gang with n_tasks < 1 or n_sets < 1");
        if (x.first_task < 0 || (int64_t)x.first_task + x.n_tasks > T || x.first_set < 0 || (int64_t)x.first_set + x.n_sets > S) return no(KAI_ERR_INVALID_ARG, "a gang's range lies outside tasks / sets");
        if (x.scores < -1 || x.scores >= n_score_rows) return no(KAI_ERR_INVALID_ARG, "scores outside -1 .. n_score_rows-1");
        for (int i = 0; i < x.n_tasks; i++) { uint8_t& seen = covered[(size_t)x.first_task + i]; if (seen) return no(KAI_ERR_INVALID_ARG, "two gangs share an entry of tasks"); seen = 1; }
        work += (int64_t)x.n_tasks * x.n_sets;
    }
    for (int i = 0; i < T; i++) if (tasks[i] < 0 || tasks[i] >= P) return no(KAI_ERR_INVALID_ARG, "pod index out of range");
    for (int i = 0; i < S; i++) if (sets[i] < -1 || sets[i] >= R) return no(KAI_ERR_INVALID_ARG, "a set row outside -1 .. n_nodesets-1");
    for (int s = 0; s < n_score_rows; s++) {  // what kai_ordered_nodes_scored refuses in the rows
        if (score_rows[s].level_row < KAI_TOPO_SCORES_EMPTY || score_rows[s].level_row >= TL) return no(KAI_ERR_INVALID_ARG, "a level_row outside -2 .. n_topo_levels-1");
        const uint8_t* row = deciles + (size_t)s * D;
        for (int d = 0; d < D; d++) if (row[d] > 10 && row[d] != KAI_TOPO_NO_SCORE) return no(KAI_ERR_INVALID_ARG, "a decile that is neither <= 10 nor 255");
    }
    {   std::vector<int32_t> sorted(tasks, tasks + T); std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return no(KAI_ERR_INVALID_ARG, "a pod is named twice in tasks"); }
    const int64_t len0 = (int64_t)core->st_rec.size();
    if (len0 + T > (int64_t)st_log_room(c)) return no(KAI_ERR_CAPACITY, "the log would exceed its room (ops_cap / 2 = 2 n_pods + 32 records)");
    if (ops_cap < T) return no(KAI_ERR_CAPACITY, "ops_cap is below n_tasks");
    if (work > KAI_SP_MAX_WORK) return no(KAI_ERR_CAPACITY, "the sum of n_tasks x n_sets over the gangs is above 2^20 (one workgroup walks the chain)");
    if ((int64_t)n_score_rows * (D + 8) > ((int64_t)1 << 30)) return no(KAI_ERR_CAPACITY, "n_score_rows x (n_domains + 8) above 2^30");
    if (n_ops) *n_ops = 0;
    if (G == 0) return KAI_OK;
    // ---- the rows the sets name and their sizes: a popcount of the caller's words over the N nodes (what k_sp_prep writes per row)
    std::vector<int32_t> row_off((size_t)R + 1, 0), used;
    for (int i = 0; i < S; i++) if (sets[i] >= 0 && !row_off[(size_t)sets[i] + 1]) { row_off[(size_t)sets[i] + 1] = 1; used.push_back(sets[i]); }
    int64_t list_len = 0;
    {   const uint32_t last = (N & 31) ? ((1u << (N & 31)) - 1u) : 0xffffffffu;
        std::vector<int32_t> size((size_t)R, 0);
        parallel_chunks(used.size(), [&](int, size_t i0, size_t i1) { for (size_t i = i0; i < i1; i++) {
            const uint32_t* row = nodeset_bitmaps + (size_t)used[i] * W; int n = 0;
            for (int w = 0; w < W; w++) n += __builtin_popcount(w == W - 1 ? row[w] & last : row[w]);
            size[(size_t)used[i]] = n; } });
        for (int r = 0; r < R; r++) { row_off[(size_t)r] = (int32_t)list_len; list_len += size[(size_t)r]; if (list_len > (int64_t)0x7fffffff - 64) return no(KAI_ERR_CAPACITY, "the named node sets hold more than 2^31 nodes"); }
        row_off[(size_t)R] = (int32_t)list_len; }
    HIP_TRY(core, hipSetDevice(core->device));
    // ---- the handle's scratch and staging: grow on demand, no allocation once the handle is warm
    const int n_used = (int)used.size();
    const SpLayout L(N, G, T, S, R, W, n_used, n_score_rows, D, (size_t)list_len);
    bool grew = false;
    KAI_TRY(reserve(core, core->sp_dev, L.end, std::max<size_t>(L.end + L.end / 2, (size_t)1 << 16), &grew));
    if (grew) core->sp_perm_ok = false;  // (the new scratch does not hold the permutation)
    KAI_TRY(reserve(core, core->sp_pin, L.down_end, std::max<size_t>(L.down_end + L.down_end / 2, (size_t)1 << 16)));
    const bool wide_ok = !(params->flags & KAI_APPLY_ENGINE_PATH) && oa_wide_session(c);
    if (!wide_ok) { const int rcs = solver_ensure(core); if (rcs) return rcs; }  // (binds core->ctx.sv: the context is read after it; before the first write)
    // ---- one staging upload, behind the permutation when the scratch does not hold this session's yet
    unsigned char* h = core->sp_pin.p; unsigned char* d = core->sp_dev.p;
    const size_t up0 = core->sp_perm_ok ? L.gangs : L.perm, up_end = L.head + sizeof(SpHead);
    if (!core->sp_perm_ok && N > 0) std::memcpy(h + L.perm, core->perm.data(), (size_t)N * 4);
    std::memcpy(h + L.gangs, gangs, (size_t)G * sizeof(kai_place_gang));
    std::memcpy(h + L.tasks, tasks, (size_t)T * 4);
    std::memcpy(h + L.sets, sets, (size_t)S * 4);
    if (n_used) std::memcpy(h + L.used, used.data(), (size_t)n_used * 4);
    std::memcpy(h + L.row_off, row_off.data(), ((size_t)R + 1) * 4);
    for (int i = 0; i < n_used; i++) std::memcpy(h + L.rows_in + (size_t)i * W * 4, nodeset_bitmaps + (size_t)used[(size_t)i] * W, (size_t)W * 4);  // only the rows the sets name
    if (n_score_rows) { std::memcpy(h + L.score_rows, score_rows, (size_t)n_score_rows * sizeof(kai_topo_score_row)); if (D > 0) std::memcpy(h + L.deciles, deciles, (size_t)n_score_rows * D); }
    SpHead* hh = reinterpret_cast<SpHead*>(h + L.head); std::memset(hh, 0, sizeof(SpHead)); hh->bad = KAI_OA_NONE; hh->len = (int32_t)len0;
    HIP_TRY(core, hipMemcpyAsync(d + up0, h + up0, up_end - up0, hipMemcpyHostToDevice, core->stream));
    core->sp_perm_ok = true;
    SpArgs a{};
    a.G = G; a.T = T; a.S = S; a.R = R; a.W = W; a.n_used = n_used; a.len0 = (int32_t)len0; a.flags = params->flags & KAI_PLACE_PIPELINE_ONLY;
    a.gangs = (KAI_GP(const kai_place_gang))(d + L.gangs); a.tasks = (KAI_GP(const int32_t))(d + L.tasks); a.sets = (KAI_GP(const int32_t))(d + L.sets);
    a.rows_in = (KAI_GP(const uint32_t))(d + L.rows_in); a.perm = (KAI_GP(const int32_t))(d + L.perm); a.used_rows = (KAI_GP(const int32_t))(d + L.used);
    a.row_off = (KAI_GP(const int32_t))(d + L.row_off); a.list = (KAI_GP(int32_t))(d + L.list);
    a.score_rows = (KAI_GP(const kai_topo_score_row))(d + L.score_rows); a.deciles = (KAI_GP(const uint8_t))(d + L.deciles);
    a.head = (KAI_GP(SpHead))(d + L.head); a.stamp = (KAI_GP(int32_t))(core->st_dev.p + StLayout(core->st_pod_cap).stamp);
    a.answers = (KAI_GP(kai_place_answer))(d + L.answers); a.fail_at = (KAI_GP(int32_t))(d + L.fail_at); a.ops = (KAI_GP(kai_op))(d + L.ops);
    // ---- two launches, one download, one synchronise
    // (KAI_PLACE_PROF: every launch between two events and waited for, the milliseconds per kernel printed; tools/stmt_place_timing.py reads the line)
    static const bool prof = std::getenv("KAI_PLACE_PROF") != nullptr;
    float prof_ms[2] = {0, 0};
    auto timed = [&](int k, auto&& launch) {
        if (!prof) { launch(); return; }
        (void)hipEventRecord(core->ev0, core->stream); launch(); (void)hipEventRecord(core->ev1, core->stream); (void)hipEventSynchronize(core->ev1);
        float ms = 0; if (hipEventElapsedTime(&ms, core->ev0, core->ev1) != hipSuccess) { (void)hipGetLastError(); ms = 0; }
        prof_ms[k] += ms;
    };
    const size_t prep_items = std::max<size_t>(std::max<size_t>((size_t)T, (size_t)S), (size_t)n_used * 64);
    timed(0, [&] { hipLaunchKernelGGL(k_sp_prep, dim3((unsigned)((prep_items + KAI_BN_WG - 1) / KAI_BN_WG)), dim3(KAI_BN_WG), 0, core->stream, core->ctx, a); });
    if (wide_ok) timed(1, [&] { hipLaunchKernelGGL(k_sp_place, dim3(1), dim3(KAI_BN_WG), 0, core->stream, core->ctx, a); });
    else timed(1, [&] { hipLaunchKernelGGL(k_sp_place_engine, dim3(1), dim3(64), 0, core->stream, core->ctx, a); });
    SpHead hv{};
    auto read_back = [&]() -> int {
        HIP_TRY(core, hipGetLastError());
        HIP_TRY(core, hipMemcpyAsync(h + L.head, d + L.head, L.down_end - L.head, hipMemcpyDeviceToHost, core->stream));
        HIP_TRY(core, hipStreamSynchronize(core->stream));
        std::memcpy(&hv, h + L.head, sizeof(SpHead));
        return KAI_OK;
    };
    if (int rc = read_back()) return st_lost(core, rc);
    if (prof) std::fprintf(stderr, "kai stmt place: path %d gangs %d | k_sp_prep %.4f k_sp_place %.4f ms\n", wide_ok ? KAI_APPLY_PATH_WIDE : KAI_APPLY_PATH_ENGINE, G, prof_ms[0], prof_ms[1]);
    if (hv.bad != KAI_OA_NONE) {
        if (result) result->first_bad = hv.bad;
        return no(KAI_ERR_STATE, "a pod of tasks is not Pending (result->first_bad is its index in tasks)");
    }
    const bool wide = wide_ok;
    if (hv.fault || (hv.applied && hv.applied != (wide ? KAI_APPLY_PATH_WIDE : KAI_APPLY_PATH_ENGINE)) || hv.len < len0 || hv.len > len0 + T) {
        char buf[200]; std::snprintf(buf, sizeof buf, "kai_stmt_place: device engine fault code %d (engine source line %d), path reported %d; the Statement is closed", hv.fault, hv.fault_line, hv.applied);
        core->err = buf; core->st_open = false; return KAI_ERR_DEVICE_FAULT;
    }
    const int64_t n = (int64_t)hv.len - len0;
    std::memcpy(answers_out, h + L.answers, (size_t)G * sizeof(kai_place_answer));
    if (fail_at_out && S > 0) std::memcpy(fail_at_out, h + L.fail_at, (size_t)S * 4);
    {   const kai_op* src = reinterpret_cast<const kai_op*>(h + L.ops); const int32_t* perm = core->perm.data();  // name rank -> the caller's node index
        const uint8_t mark = wide ? ST_REC_WIDE : 0;
        for (int64_t i = 0; i < n; i++) { kai_op o = src[i]; o.node = perm[o.node]; ops_out[i] = o; core->st_rec.push_back((uint8_t)o.kind | mark); } }
    if (n_ops) *n_ops = n;
    if (hv.wrote) core->index_stale = true;  // neither mode keeps the class index: rebuilt before the next action reads it
    if (result) { result->path = wide ? KAI_APPLY_PATH_WIDE : KAI_APPLY_PATH_ENGINE; result->log_len = (int64_t)core->st_rec.size(); }
    return KAI_OK;
}

// kai_stale_gang_eviction's kernels for sg_drive (kai_stale_gangs.hpp), on top of the apply's launcher; pin: [the counts | the apply's verdict] in the handle's staging
struct SgLauncher : OaLauncher {
    unsigned char* pin_counts;
    SgLauncher(kai_core* core_, unsigned char* pin_) : OaLauncher{core_, pin_ + sizeof(SgHead)}, pin_counts(pin_) {}
    static dim3 g(int n) { return dim3((unsigned)n); }
    void succeeded(int n, int b, const KaiCtx& c, const SgArgs& a) { hipLaunchKernelGGL(k_sg_succeeded, g(n), g(b), 0, core->stream, c, a); }
    void jobs(int n, int b, const KaiCtx& c, const SgArgs& a) { hipLaunchKernelGGL(k_sg_jobs, g(n), g(b), 0, core->stream, c, a); }
    void first(int n, int b, const KaiCtx& c, const SgArgs& a) { hipLaunchKernelGGL(k_sg_first, g(n), g(b), 0, core->stream, c, a); }
    void totals(int n, int b, const KaiCtx& c, const SgArgs& a) { hipLaunchKernelGGL(k_sg_totals, g(n), g(b), 0, core->stream, c, a); }
    void scan(int b, const SgArgs& a) { hipLaunchKernelGGL(k_sg_scan, g(1), g(b), 0, core->stream, a); }
    void emit(int n, int b, const KaiCtx& c, const SgArgs& a) { hipLaunchKernelGGL(k_sg_emit, g(n), g(b), 0, core->stream, c, a); }
    int read_counts(SgHead& hd, const SgArgs& a) {
        HIP_TRY(core, hipGetLastError());
        HIP_TRY(core, hipMemcpyAsync(pin_counts, (const void*)a.head, sizeof(SgHead), hipMemcpyDeviceToHost, core->stream));
        HIP_TRY(core, hipStreamSynchronize(core->stream));
        std::memcpy(&hd, pin_counts, sizeof(SgHead));
        return KAI_OK;
    }
    int reserve_ops(int n, SgArgs& a, OaArgs& oa) {
        KAI_TRY(oa_reserve_scratch(core, n));
        const OaLayout L(core->oa_pod_cap, n); unsigned char* d = core->oa_dev.p;
        a.oa_head = (KAI_GP(OaHead))(d + L.head); a.ops = (KAI_GP(kai_op))(d + L.ops);
        oa.ops = (KAI_GP(const kai_op))(d + L.ops); oa.head = (KAI_GP(OaHead))(d + L.head);
        oa.stamp = (KAI_GP(int32_t))(d + L.stamp); oa.sh_status = (KAI_GP(int32_t))(d + L.sh_status); oa.sh_node = (KAI_GP(int32_t))(d + L.sh_node);
        return KAI_OK;
    }
};

int kai_stale_gang_eviction(kai_core* core, const kai_stale_params* params, int64_t* job_stale_since_ns, uint8_t* job_stale_out,
                            kai_op* ops_out, int64_t ops_cap, int64_t* n_ops, kai_stale_result* result) {
    // every host-decidable refusal before the first device call and before the first write to the caller's arrays
    if (!core) return KAI_ERR_INVALID_ARG;
    if (!params || !job_stale_since_ns || !n_ops) return fail(core, KAI_ERR_INVALID_ARG, "kai_stale_gang_eviction: params / job_stale_since_ns / n_ops is NULL");
    if (params->version != KAI_STALE_VERSION) return fail(core, KAI_ERR_INVALID_ARG, "kai_stale_gang_eviction: wrong params version");
    if (params->flags & ~KAI_STALE_DRY_RUN) return fail(core, KAI_ERR_INVALID_ARG, "kai_stale_gang_eviction: unknown flag bits");
    if (ops_cap < 0 || (ops_cap > 0 && !ops_out)) return fail(core, KAI_ERR_INVALID_ARG, "kai_stale_gang_eviction: a negative capacity, or ops_out is NULL");
    if (core->world > 1) return fail(core, KAI_ERR_UNSUPPORTED, "kai_stale_gang_eviction: a handle of a sharded group");
    if (!core->open) return fail(core, KAI_ERR_STATE, "no open session");
    if (core->shared) return fail(core, KAI_ERR_UNSUPPORTED, "kai_stale_gang_eviction: a session with shared-GPU requests (kai_op carries no GPU group)");
    if (core->st_open) return fail(core, KAI_ERR_STATE, "kai_stale_gang_eviction: a Statement is open (kai_stmt_commit or kai_stmt_discard first)");
    KaiCtx& c = core->ctx;
    if (c.now_ns <= 0) return fail(core, KAI_ERR_INVALID_ARG, "kai_stale_gang_eviction: the handle's clock is not above 0 (kai_core_set_now): 0 stands for no timestamp");
    const int J = c.J, P = c.P;
    for (int j = 0; j < J; j++) if (job_stale_since_ns[j] < 0) return fail(core, KAI_ERR_INVALID_ARG, "kai_stale_gang_eviction: a negative job_stale_since_ns entry");
    const bool dry_run = (params->flags & KAI_STALE_DRY_RUN) != 0;
    HIP_TRY(core, hipSetDevice(core->device));
    // ---- the handle's scratch and staging: grow on demand, no allocation once the handle is warm
    const int n_wgs = (int)(((int64_t)P + KAI_SG_WG - 1) / KAI_SG_WG);
    if ((size_t)J > core->sg_job_cap || (size_t)n_wgs > core->sg_wg_cap) {
        const size_t job_cap = std::max(std::max<size_t>((size_t)J + (size_t)J / 4, 1024), core->sg_job_cap), wg_cap = std::max(std::max<size_t>((size_t)n_wgs + (size_t)n_wgs / 4, 64), core->sg_wg_cap);
        const SgLayout G(job_cap, wg_cap);
        KAI_TRY(reserve(core, core->sg_dev, SIZE_MAX, G.end));
        core->sg_job_cap = job_cap; core->sg_wg_cap = wg_cap;
        HIP_TRY(core, hipMemsetAsync(core->sg_dev.p, 0, G.end, core->stream));  // the Succeeded flags: zero between calls (k_sg_jobs clears what it reads)
    }
    const SgLayout L(core->sg_job_cap, core->sg_wg_cap);
    // staging: [counts | timestamps] up; [counts | the apply's verdict | timestamps | Stale bytes | operations] down
    auto al = [](size_t x) { return (x + 15) & ~(size_t)15; };
    const size_t up_bytes = sizeof(SgHead) + (size_t)J * 8, dn_since = al(up_bytes) + sizeof(SgHead) + sizeof(OaHead), dn_stale = dn_since + (size_t)J * 8, dn_ops = al(dn_stale + (size_t)J);
    KAI_TRY(reserve(core, core->sg_pin, dn_ops, std::max<size_t>(dn_ops + dn_ops / 2, (size_t)1 << 16)));
    unsigned char* h = core->sg_pin.p; unsigned char* d = core->sg_dev.p;
    // ---- one upload: the zeroed counts and the caller's timestamps
    std::memset(h, 0, sizeof(SgHead));
    std::memcpy(h + sizeof(SgHead), job_stale_since_ns, (size_t)J * 8);
    HIP_TRY(core, hipMemcpyAsync(d + L.head, h, up_bytes, hipMemcpyHostToDevice, core->stream));
    SgArgs a{};
    a.now_ns = c.now_ns; a.grace_ns = params->grace_ns; a.n_wgs = n_wgs;
    a.head = (KAI_GP(SgHead))(d + L.head); a.since = (KAI_GP(int64_t))(d + L.since); a.expired = (KAI_GP(uint8_t))(d + L.expired);
    a.succ = (KAI_GP(int32_t))(d + L.succ); a.first = (KAI_GP(int32_t))(d + L.first); a.wg_e = (KAI_GP(int32_t))(d + L.wg_e); a.wg_f = (KAI_GP(int32_t))(d + L.wg_f);
    // ---- the decision, one small download, the apply (sg_drive)
    SgLauncher launcher(core, h + al(up_bytes));
    SgHead hd{}; OaHead hv{}; int path = KAI_APPLY_PATH_NONE;
    const int rcd = sg_drive(launcher, core->ctx, a, KAI_SG_WG, dry_run, ops_cap, hd, hv, path);
    if (rcd == KAI_ERR_CAPACITY) { *n_ops = hd.n_ops; return fail(core, KAI_ERR_CAPACITY, "kai_stale_gang_eviction: ops_cap is below the number of evictions (*n_ops holds it)"); }
    if (rcd == KAI_ERR_DEVICE_FAULT) { char buf[200]; std::snprintf(buf, sizeof buf, "kai_stale_gang_eviction: the apply refused the evictions (first bad %d, device engine fault code %d, engine source line %d)", hv.bad, hv.fault, hv.fault_line); core->err = buf; return rcd; }
    if (rcd) return rcd;
    const int n = hd.n_ops;
    if (n > 0 && !dry_run) { core->index_stale = true; c.fast_ok = 0; }  // as kai_ops_apply leaves the handle after evictions
    // ---- the timestamps, the Stale bytes and the operations down
    KAI_TRY(reserve(core, core->sg_pin, dn_ops + (size_t)n * sizeof(kai_op), dn_ops + ((size_t)n + (size_t)n / 2 + 1024) * sizeof(kai_op)));
    h = core->sg_pin.p;
    if (J) {
        HIP_TRY(core, hipMemcpyAsync(h + dn_since, d + L.since, (size_t)J * 8, hipMemcpyDeviceToHost, core->stream));
        HIP_TRY(core, hipMemcpyAsync(h + dn_stale, d + L.expired, (size_t)J, hipMemcpyDeviceToHost, core->stream));
    }
    if (n) HIP_TRY(core, hipMemcpyAsync(h + dn_ops, (const void*)a.ops, (size_t)n * sizeof(kai_op), hipMemcpyDeviceToHost, core->stream));
    HIP_TRY(core, hipStreamSynchronize(core->stream));
    std::memcpy(job_stale_since_ns, h + dn_since, (size_t)J * 8);
    if (job_stale_out) std::memcpy(job_stale_out, h + dn_stale, (size_t)J);
    {   const kai_op* src = reinterpret_cast<const kai_op*>(h + dn_ops); const int32_t* perm = core->perm.data();  // name rank -> the caller's node index
        parallel_chunks((size_t)n, [&](int, size_t i0, size_t i1) { for (size_t i = i0; i < i1; i++) { kai_op o = src[i]; o.node = perm[o.node]; ops_out[i] = o; } }); }
    *n_ops = n;
    if (result) { result->stale_jobs = hd.stale_jobs; result->expired_jobs = hd.expired_jobs; result->n_ops = n; result->path = path; result->pad = 0; }
    return KAI_OK;
}

}  // extern "C"

// A launcher that can time its launches: with `prof` every launch runs between two events and is waited for, the milliseconds per kernel summed over the call and printed.
// kai_job_order's kernels for jo_drive (kai_job_order.hpp); pin: where the head lands in the handle's staging.  KAI_JOB_ORDER_PROF: every launch between two events and waited
// for, the milliseconds per kernel summed over the call and printed (tools/job_order_timing.py reads the line).  (A member template: outside the extern "C" block.)
struct ProfLauncher {
    kai_core* core; unsigned char* pin; bool prof = false; std::vector<std::pair<const char*, float>> spent;
    static dim3 g(int n) { return dim3((unsigned)n); }
    template <class F> void run(const char* name, F&& launch) {
        if (!prof) { launch(); return; }
        (void)hipEventRecord(core->ev0, core->stream); launch(); (void)hipEventRecord(core->ev1, core->stream); (void)hipEventSynchronize(core->ev1);
        float ms = 0; if (hipEventElapsedTime(&ms, core->ev0, core->ev1) != hipSuccess) { (void)hipGetLastError(); ms = 0; }
        for (auto& e : spent) if (e.first == name) { e.second += ms; return; }
        spent.push_back({name, ms});
    }
    void report(const char* what, const char* counted, int path, long long n) const {
        if (!prof) return;
        std::fprintf(stderr, "%s: path %d %s %lld |", what, path, counted, n);
        for (const auto& e : spent) std::fprintf(stderr, " %s %.4f", e.first, e.second);
        std::fprintf(stderr, " ms\n");
    }
};
struct JoLauncher : ProfLauncher {
    JoLauncher(kai_core* core_, unsigned char* pin_, bool prof_) : ProfLauncher{core_, pin_, prof_, {}} {}
    void report(int path, int n) const { ProfLauncher::report("kai job order", "ordered", path, n); }
    void job_init(int n, int b, const KaiCtx& c) { run("k_job_init", [&] { hipLaunchKernelGGL(k_job_init, g(n), g(b), 0, core->stream, c); }); }
    void leaf_init(int n, int b, const KaiCtx& c) { run("k_leaf_init", [&] { hipLaunchKernelGGL(k_leaf_init, g(n), g(b), 0, core->stream, c); }); }
    void qualify(int n, int b, const KaiCtx& c, const JoArgs& a) { run("k_jo_qualify", [&] { hipLaunchKernelGGL(k_jo_qualify, g(n), g(b), 0, core->stream, c, a); }); }
    void static_rank(int n, int b, const KaiCtx& c) { run("k_batch_static_rank", [&] { hipLaunchKernelGGL(k_batch_static_rank, g(n), g(b), 0, core->stream, c); }); }
    void static_check(int n, int b, const KaiCtx& c) { run("k_batch_static_check", [&] { hipLaunchKernelGGL(k_batch_static_check, g(n), g(b), 0, core->stream, c); }); }
    void plan_setup(int n, int b, const KaiCtx& c, RoundParams rp) { run("k_plan_setup", [&] { hipLaunchKernelGGL(k_plan_setup, g(n), g(b), 0, core->stream, c, rp); }); }
    void leaf(int n, int b, const KaiCtx& c, const JoArgs& a) { run("k_jo_leaf", [&] { hipLaunchKernelGGL(k_jo_leaf, g(n), g(b), 0, core->stream, c, a); }); }
    void plan_rank(int n, int b, const KaiCtx& c, RoundParams rp) { run("k_plan_rank", [&] { hipLaunchKernelGGL(k_plan_rank, g(n), g(b), 0, core->stream, c, rp); }); }
    void keys(int n, int b, const KaiCtx& c, const JoArgs& a, RoundParams rp) { run("k_jo_keys", [&] { hipLaunchKernelGGL(k_jo_keys, g(n), g(b), 0, core->stream, c, a, rp); }); }
    void scan(int n, int b, const KaiCtx& c, RoundParams rp) { run("k_jo_scan", [&] { hipLaunchKernelGGL(k_jo_scan, g(n), g(b), 0, core->stream, c, rp); }); }
    void emit(int n, int b, const KaiCtx& c, const JoArgs& a) { run("k_jo_emit", [&] { hipLaunchKernelGGL(k_jo_emit, g(n), g(b), 0, core->stream, c, a); }); }
    int engine(const KaiCtx& c, const JoArgs& a) { run("k_jo_engine", [&] { hipLaunchKernelGGL(k_jo_engine, dim3(1), dim3(64), 0, core->stream, c, a); }); return KAI_OK; }
    int read_head(JoHead& hd, const JoArgs& a) {
        HIP_TRY(core, hipGetLastError());
        HIP_TRY(core, hipMemcpyAsync(pin, (const void*)a.head, sizeof(JoHead), hipMemcpyDeviceToHost, core->stream));
        HIP_TRY(core, hipStreamSynchronize(core->stream));
        std::memcpy(&hd, pin, sizeof(JoHead));
        return KAI_OK;
    }
};

extern "C" {

int kai_job_order(kai_core* core, const kai_job_order_params* params, int32_t* order_out, int32_t cap, int32_t* n_out,
                  int32_t* job_pos_out, int32_t* job_queue_pos_out, kai_job_order_result* result) {
    // every refusal before the first device call and before the first write to the caller's arrays
    if (!core) return KAI_ERR_INVALID_ARG;
    if (!params || !n_out) return fail(core, KAI_ERR_INVALID_ARG, "kai_job_order: params / n_out is NULL");
    if (params->version != KAI_JOB_ORDER_VERSION) return fail(core, KAI_ERR_INVALID_ARG, "kai_job_order: wrong params version");
    if (params->flags & ~KAI_JOB_ORDER_ENGINE_PATH) return fail(core, KAI_ERR_INVALID_ARG, "kai_job_order: unknown flag bits");
    if (params->pad != 0) return fail(core, KAI_ERR_INVALID_ARG, "kai_job_order: pad is not zero");
    if (params->depth < -1) return fail(core, KAI_ERR_INVALID_ARG, "kai_job_order: depth below -1");
    if (cap < 0 || (cap > 0 && !order_out)) return fail(core, KAI_ERR_INVALID_ARG, "kai_job_order: a negative capacity, or order_out is NULL");
    if (core->world > 1) return fail(core, KAI_ERR_UNSUPPORTED, "kai_job_order: a handle of a sharded group");
    if (!core->open) return fail(core, KAI_ERR_STATE, "no open session");
    const KaiCtx& c = core->ctx;
    const int J = c.J, Q = c.Q, n_heights = core->prep.n_heights;
    int depth = params->depth == 0 ? core->cfg.queue_depth[KAI_ACTION_ALLOCATE] : params->depth;
    if (depth < 0) depth = 0;  // (infinite)
    HIP_TRY(core, hipSetDevice(core->device));
    // ---- the handle's scratch and staging: grow on demand, no allocation once the handle is warm
    const size_t pool = jo_pool(J, Q, n_heights);
    const JoLayout L((size_t)J, (size_t)Q, (size_t)n_heights, pool);
    bool grew = false;
    KAI_TRY(reserve(core, core->jo_dev, L.end, L.end + L.end / 4, &grew));
    if (grew) HIP_TRY(core, hipMemsetAsync(core->jo_dev.p, 0, core->jo_dev.bytes, core->stream));  // (the pools' indices are checked where they are read; zeros rather than what the memory held)
    const size_t pin_need = L.down_end + sizeof(JoHead);  // [what is sent, and later what comes back][the head between the launches]
    KAI_TRY(reserve(core, core->jo_pin, pin_need, std::max<size_t>(pin_need + pin_need / 4, (size_t)1 << 16)));
    unsigned char* h = core->jo_pin.p; unsigned char* d = core->jo_dev.p;
    // ---- one upload: the zeroed head and the queue tree's tables (heights, nodes by height)
    std::memset(h, 0, L.up_end);
    std::memcpy(h + L.q_height, core->prep.q_height.data(), (size_t)(Q + 1) * 4);
    std::memcpy(h + L.h_off, core->prep.h_off.data(), (size_t)(n_heights + 1) * 4);
    std::memcpy(h + L.h_nodes, core->prep.h_nodes.data(), (size_t)(Q + 1) * 4);
    HIP_TRY(core, hipMemcpyAsync(d, h, L.up_end, hipMemcpyHostToDevice, core->stream));
    const KaiCtx cj = jo_bind_ctx(c, d, L, n_heights, pool, depth);
    const JoArgs a = jo_bind_args(c, d, L, pool);
    // ---- the init, the qualification behind one small download, the order (jo_drive)
    JoLauncher launcher{core, h + L.down_end, std::getenv("KAI_JOB_ORDER_PROF") != nullptr};
    JoHead hd{}; int path = KAI_JOB_ORDER_PATH_NONE;
    const int rcd = jo_drive(launcher, cj, a, core->shape, jo_wide_session(c, n_heights, pool), depth, params->flags, KAI_JO_WG, hd, path);
    if (rcd == KAI_ERR_DEVICE_FAULT) { char buf[160]; std::snprintf(buf, sizeof buf, "kai_job_order: device fault code %d (engine source line %d)", hd.fault, hd.fault_line); core->err = buf; return rcd; }
    if (rcd) return rcd;
    const int n = path == KAI_JOB_ORDER_PATH_NONE ? 0 : hd.n_ordered;
    launcher.report(path, n);
    if (n > cap) { *n_out = n; return fail(core, KAI_ERR_CAPACITY, "kai_job_order: cap is below the number of ordered jobs (*n_out holds it)"); }
    // ---- one download: [.. | order | positions], as far as the caller wants it
    const bool want_pos = job_pos_out || job_queue_pos_out;
    const size_t lo = L.order, hi = want_pos && J ? L.down_end : L.order + (size_t)n * 4;
    if (hi > lo) {
        HIP_TRY(core, hipMemcpyAsync(h + lo, d + lo, hi - lo, hipMemcpyDeviceToHost, core->stream));
        HIP_TRY(core, hipStreamSynchronize(core->stream));
    }
    if (n) std::memcpy(order_out, h + L.order, (size_t)n * 4);
    if (job_pos_out && J) std::memcpy(job_pos_out, h + L.pos, (size_t)J * 4);
    if (job_queue_pos_out && J) std::memcpy(job_queue_pos_out, h + L.qpos, (size_t)J * 4);
    *n_out = n;
    if (result) { result->n_ordered = n; result->path = path; result->n_leaves = n ? hd.n_leaves : 0; result->pad = 0; }
    return KAI_OK;
}

}  // extern "C"

// kai_subset_nodes' kernels for sn_count (kai_subset_nodes.hpp); pin: where the head lands in the handle's staging.  KAI_SUBSET_PROF: the per-launch times
// (tools/subset_nodes_timing.py reads the line).
struct SnLauncher : ProfLauncher {
    SnLauncher(kai_core* core_, unsigned char* pin_, bool prof_) : ProfLauncher{core_, pin_, prof_, {}} {}
    void tta(int n, int b, const KaiCtx& c, const SnArgs& a) { run("k_sn_tta", [&] { hipLaunchKernelGGL(k_sn_tta, g(n), g(b), 0, core->stream, c, a); }); }
    void prep(int n, int b, const KaiCtx& c, const SnArgs& a) { run("k_sn_prep", [&] { hipLaunchKernelGGL(k_sn_prep, g(n), g(b), 0, core->stream, c, a); }); }
    void wide(int n, int b, const KaiCtx& c, const SnArgs& a) { run("k_sn_wide", [&] { hipLaunchKernelGGL(k_sn_wide, g(n), g(b), 0, core->stream, c, a); }); }
    void offsets(int n, int b, const KaiCtx& c, const SnArgs& a) { run("k_sn_offsets", [&] { hipLaunchKernelGGL(k_sn_offsets, g(n), g(b), 0, core->stream, c, a); }); }
    void emit(int n, int b, const KaiCtx& c, const SnArgs& a) { run("k_sn_emit", [&] { hipLaunchKernelGGL(k_sn_emit, g(n), g(b), 0, core->stream, c, a); }); }
    int engine(const KaiCtx& c, const SnArgs& a) { run("k_sn_engine", [&] { hipLaunchKernelGGL(k_sn_engine, dim3(1), dim3(64), 0, core->stream, c, a); }); return KAI_OK; }
    int read_head(SnHead& hd, const SnArgs& a) {
        HIP_TRY(core, hipGetLastError());
        HIP_TRY(core, hipMemcpyAsync(pin, (const void*)a.head, sizeof(SnHead), hipMemcpyDeviceToHost, core->stream));
        HIP_TRY(core, hipStreamSynchronize(core->stream));
        std::memcpy(&hd, pin, sizeof(SnHead));
        return KAI_OK;
    }
};

// kai_subset_nodes and kai_subset_nodes_scored (scored: with the preferred-level scores into score_rows_out / deciles_out)
static int subset_nodes_call(kai_core* core, const char* who, bool scored, const kai_subset_params* params, const kai_subset_query* queries, int32_t n_queries, const uint32_t* nodeset_bitmaps,
                             int32_t n_nodesets, kai_subset_answer* answers_out, kai_node_set* sets_out, int64_t sets_cap, int64_t* n_sets_out, uint32_t* bitmaps_out,
                             kai_topo_score_row* score_rows_out, uint8_t* deciles_out, kai_subset_result* result) {
    // every refusal before the first device call and before the first write to the caller's arrays
    if (!core) return KAI_ERR_INVALID_ARG;
    auto no = [&](int code, const char* why) { core->err = std::string(who) + ": " + why; return code; };
    if (!params || !n_sets_out) return no(KAI_ERR_INVALID_ARG, "params / n_sets_out is NULL");
    if (params->version != KAI_SUBSET_VERSION) return no(KAI_ERR_INVALID_ARG, "wrong params version");
    if (params->flags & ~KAI_SUBSET_ENGINE_PATH) return no(KAI_ERR_INVALID_ARG, "unknown flag bits");
    if (n_queries < 0 || n_nodesets < 0 || sets_cap < 0) return no(KAI_ERR_INVALID_ARG, "a negative count or capacity");
    if (n_queries > 0 && (!queries || !answers_out)) return no(KAI_ERR_INVALID_ARG, "queries / answers_out is NULL");
    if (n_nodesets > 0 && !nodeset_bitmaps) return no(KAI_ERR_INVALID_ARG, "nodeset_bitmaps is NULL");
    if (sets_cap > 0 && !sets_out) return no(KAI_ERR_INVALID_ARG, "sets_out is NULL");
    if (scored && n_queries > 0 && (!score_rows_out || !deciles_out)) return no(KAI_ERR_INVALID_ARG, "score_rows_out / deciles_out is NULL");
    if (core->world > 1) return no(KAI_ERR_UNSUPPORTED, "a handle of a sharded group");
    if (!core->open) return fail(core, KAI_ERR_STATE, "no open session");
    const KaiCtx& c = core->ctx;
    const HostPrep& hp = core->prep;
    for (int i = 0; i < n_queries; i++) {
        const kai_subset_query& q = queries[i];
        if (q.job < 0 || q.job >= c.J) return no(KAI_ERR_INVALID_ARG, "job index out of range");
        if (q.group < -1 || q.podset < -1) return no(KAI_ERR_INVALID_ARG, "group / podset below -1");
        if (q.group >= 0 && q.podset >= 0) return no(KAI_ERR_INVALID_ARG, "both group and podset given");
        if ((q.group >= 0 || q.podset >= 0) && hp.groups_default) return no(KAI_ERR_INVALID_ARG, "a snapshot without groups has the root form only");
        if (q.group >= hp.G || q.podset >= c.S) return no(KAI_ERR_INVALID_ARG, "group / podset out of range");
        if (q.group >= 0 && hp.g_job[(size_t)q.group] != q.job) return no(KAI_ERR_INVALID_ARG, "the group is not the job's");
        if (q.podset >= 0 && hp.g_job[(size_t)hp.s_group[(size_t)q.podset]] != q.job) return no(KAI_ERR_INVALID_ARG, "the pod-set is not the job's");
        if (q.nodeset < -1 || q.nodeset >= n_nodesets) return no(KAI_ERR_INVALID_ARG, "nodeset outside -1 .. n_nodesets-1");
    }
    if (n_queries == 0) { *n_sets_out = 0; if (result) { result->n_sets = 0; result->path = KAI_SUBSET_PATH_NONE; result->pad = 0; } return KAI_OK; }
    const int N = c.N, M = n_queries, S = n_nodesets, W = (N + 31) / 32, DT = c.D + c.T;
    if (!core->sn_shape_ok) {  // the session's topologies: the most domains (its root included) and the most levels one of them has
        std::vector<int> cnt((size_t)std::max(c.T, 1), 1);
        for (int d = 0; d < c.D; d++) cnt[(size_t)hp.dom_topo[(size_t)d]]++;
        core->sn_stride = 1; core->sn_levels = 0;
        for (int t = 0; t < c.T; t++) { core->sn_stride = std::max(core->sn_stride, cnt[(size_t)t]); core->sn_levels = std::max(core->sn_levels, hp.topo_level_off[(size_t)t + 1] - hp.topo_level_off[(size_t)t]); }
        core->sn_shape_ok = true;
    }
    const int stride = core->sn_stride;
    if ((int64_t)M * stride > ((int64_t)1 << 30)) return no(KAI_ERR_CAPACITY, "n_queries x (domains of the largest topology + 1) above 2^30");
    HIP_TRY(core, hipSetDevice(core->device));
    const bool wide = !(params->flags & KAI_SUBSET_ENGINE_PATH) && sn_wide_session(c, core->sn_levels);
    // workgroups of k_sn_wide: as k_bn_scan's grid, and no more than 256 MiB of domain tables
    const int cus = device_cus(core);
    const size_t table_bytes = (size_t)std::max(DT, 1) * (KAI_MAX_RES * 8 + 8 + 8 + 4 + 4 + 4 + (scored ? 4 : 0));
    const int wgs = wide ? (int)std::max<size_t>(1, std::min<size_t>((size_t)std::min(M, cus * KAI_SN_WGS_PER_CU), ((size_t)256 << 20) / table_bytes)) : 0;
    const int n_children = DT > 0 ? hp.dom_child_off[(size_t)DT] : 0;
    // ---- the handle's scratch and staging: grow on demand, no allocation once the handle is warm
    const SnLayout L(N, M, S, W, stride, DT, n_children, wgs, scored, c.D);
    bool grew = false;
    KAI_TRY(reserve(core, core->sn_dev, L.end, L.end + L.end / 4, &grew));
    if (grew) core->sn_tab_ok = false;  // (the new scratch does not hold the session's tables)
    const size_t pin_need = L.up_end + sizeof(SnHead);  // [what is sent][the head between the launches]
    KAI_TRY(reserve(core, core->sn_pin, pin_need, std::max<size_t>(pin_need + pin_need / 4, (size_t)1 << 16)));
    unsigned char* h = core->sn_pin.p; unsigned char* d = core->sn_dev.p;
    // ---- one upload: [queries | rows | the zeroed head], behind the session's tables (both permutations, the children table) when the scratch does not hold them yet
    const size_t up0 = core->sn_tab_ok ? L.queries : 0;
    if (!core->sn_tab_ok) {
        int32_t* rank = reinterpret_cast<int32_t*>(h + L.rank);
        if (N > 0) std::memcpy(h + L.perm, core->perm.data(), (size_t)N * 4);
        for (int i = 0; i < N; i++) rank[core->perm[(size_t)i]] = i;
        if (n_children > 0) std::memcpy(h + L.children, hp.dom_children.data(), (size_t)n_children * 4);
    }
    std::memcpy(h + L.queries, queries, (size_t)M * sizeof(kai_subset_query));
    if (S > 0 && W > 0) std::memcpy(h + L.rows_in, nodeset_bitmaps, (size_t)S * W * 4);
    std::memset(h + L.head, 0, sizeof(SnHead));
    HIP_TRY(core, hipMemcpyAsync(d + up0, h + up0, L.up_end - up0, hipMemcpyHostToDevice, core->stream));
    core->sn_tab_ok = true;
    SnArgs a = sn_bind_args(d, L, M, S, W, stride);
    a.want_bitmaps = bitmaps_out ? 1 : 0; a.want_scores = scored ? 1 : 0;
    KaiCtx cq = c; cq.action = KAI_ACTION_ALLOCATE;  // (the chunk the allocate action hands over)
    // ---- the walks and the count, behind one small download
    SnLauncher launcher(core, h + L.up_end, std::getenv("KAI_SUBSET_PROF") != nullptr);
    SnHead hd{}; int path = KAI_SUBSET_PATH_NONE;
    const int rcd = sn_count(launcher, cq, a, wide, KAI_SN_WG, wgs, hd, path);
    if (rcd == KAI_ERR_DEVICE_FAULT) { char buf[160]; std::snprintf(buf, sizeof buf, "%s: engine fault code %d (engine source line %d)", who, hd.fault, hd.fault_line); core->err = buf; return rcd; }
    if (rcd) return rcd;
    const int64_t total = hd.total;
    if (total > sets_cap) { *n_sets_out = total; return no(KAI_ERR_CAPACITY, "sets_cap is below the number of node sets (*n_sets_out holds it)"); }
    // ---- the records and the bitmap rows into a buffer of their own, then one download: [answers][sets | bitmaps]
    const size_t set_bytes = (size_t)total * sizeof(kai_node_set), map_bytes = bitmaps_out ? (size_t)total * W * 4 : 0, ans_bytes = (size_t)M * sizeof(kai_subset_answer);
    if (total > 0) {
        KAI_TRY(reserve(core, core->sn_out, set_bytes + map_bytes, set_bytes + map_bytes + (set_bytes + map_bytes) / 4));
        a.sets = (KAI_GP(kai_node_set))core->sn_out.p; a.bitmaps = (KAI_GP(uint32_t))(core->sn_out.p + set_bytes);
        launcher.emit((int)std::min<int64_t>(total, (int64_t)cus * KAI_SN_WGS_PER_CU), KAI_SN_WG, cq, a);
        HIP_TRY(core, hipGetLastError());
    }
    const size_t score_bytes = scored ? L.end - L.score_rows : 0;  // [score_rows | deciles] as they lie in the scratch
    const size_t down = ans_bytes + set_bytes + map_bytes + score_bytes;
    KAI_TRY(reserve(core, core->sn_pin, down, std::max<size_t>(down + down / 4, (size_t)1 << 16)));  // (what the staging held has been sent)
    h = core->sn_pin.p;
    HIP_TRY(core, hipMemcpyAsync(h, d + L.answers, ans_bytes, hipMemcpyDeviceToHost, core->stream));
    if (total > 0) HIP_TRY(core, hipMemcpyAsync(h + ans_bytes, core->sn_out.p, set_bytes + map_bytes, hipMemcpyDeviceToHost, core->stream));
    if (score_bytes) HIP_TRY(core, hipMemcpyAsync(h + ans_bytes + set_bytes + map_bytes, d + L.score_rows, score_bytes, hipMemcpyDeviceToHost, core->stream));
    HIP_TRY(core, hipStreamSynchronize(core->stream));
    launcher.report("kai subset nodes", "sets", path, total);
    if (scored) {
        const unsigned char* hs = h + ans_bytes + set_bytes + map_bytes;
        std::memcpy(score_rows_out, hs, (size_t)M * sizeof(kai_topo_score_row));
        if (c.D > 0) std::memcpy(deciles_out, hs + (L.deciles - L.score_rows), (size_t)M * (size_t)c.D);
    }
    std::memcpy(answers_out, h, ans_bytes);
    if (total > 0) { std::memcpy(sets_out, h + ans_bytes, set_bytes); if (bitmaps_out) std::memcpy(bitmaps_out, h + ans_bytes + set_bytes, map_bytes); }
    *n_sets_out = total;
    if (result) { result->n_sets = total; result->path = path; result->pad = 0; }
    return KAI_OK;
}

extern "C" {

int kai_subset_nodes(kai_core* core, const kai_subset_params* params, const kai_subset_query* queries, int32_t n_queries, const uint32_t* nodeset_bitmaps, int32_t n_nodesets,
                     kai_subset_answer* answers_out, kai_node_set* sets_out, int64_t sets_cap, int64_t* n_sets_out, uint32_t* bitmaps_out, kai_subset_result* result) {
    return subset_nodes_call(core, "kai_subset_nodes", false, params, queries, n_queries, nodeset_bitmaps, n_nodesets, answers_out, sets_out, sets_cap, n_sets_out, bitmaps_out, nullptr, nullptr, result);
}

int kai_subset_nodes_scored(kai_core* core, const kai_subset_params* params, const kai_subset_query* queries, int32_t n_queries, const uint32_t* nodeset_bitmaps, int32_t n_nodesets,
                            kai_subset_answer* answers_out, kai_node_set* sets_out, int64_t sets_cap, int64_t* n_sets_out, uint32_t* bitmaps_out,
                            kai_topo_score_row* score_rows_out, uint8_t* deciles_out, kai_subset_result* result) {
    return subset_nodes_call(core, "kai_subset_nodes_scored", true, params, queries, n_queries, nodeset_bitmaps, n_nodesets, answers_out, sets_out, sets_cap, n_sets_out, bitmaps_out, score_rows_out, deciles_out, result);
}

int kai_pod_states(kai_core* core, int32_t* status_out, int32_t* node_out, int cap) {
    if (!core) return KAI_ERR_INVALID_ARG;
    if (!core->open) return fail(core, KAI_ERR_STATE, "no open session");
    const int P = core->ctx.P;
    if (cap < P) return fail(core, KAI_ERR_CAPACITY, "kai_pod_states: cap < n_pods");
    HIP_TRY(core, hipSetDevice(core->device));
    if (status_out && P) HIP_TRY(core, hipMemcpyAsync(status_out, KAI_VP(core->ctx.p_status), (size_t)P * 4, hipMemcpyDeviceToHost, core->stream));
    if (node_out && P) HIP_TRY(core, hipMemcpyAsync(node_out, KAI_VP(core->ctx.p_node), (size_t)P * 4, hipMemcpyDeviceToHost, core->stream));
    HIP_TRY(core, hipStreamSynchronize(core->stream));
    if (node_out) for (int p = 0; p < P; p++) if (node_out[p] >= 0) node_out[p] = core->perm[node_out[p]];
    return KAI_OK;
}

int kai_node_states(kai_core* core, kai_node_state* out, int cap) {
    if (!core || !out) return KAI_ERR_INVALID_ARG;
    if (!core->open) return fail(core, KAI_ERR_STATE, "no open session");
    const int N = core->ctx.N, R = core->ctx.R;
    if (cap < N) return fail(core, KAI_ERR_CAPACITY, "kai_node_states: cap < n_nodes");
    HIP_TRY(core, hipSetDevice(core->device));
    std::vector<double> idle((size_t)R * N + 1), rel((size_t)R * N + 1), used((size_t)R * N + 1);
    if (N) {
        HIP_TRY(core, hipMemcpyAsync(idle.data(), KAI_VP(core->ctx.n_idle), (size_t)R * N * 8, hipMemcpyDeviceToHost, core->stream));
        HIP_TRY(core, hipMemcpyAsync(rel.data(), KAI_VP(core->ctx.n_rel), (size_t)R * N * 8, hipMemcpyDeviceToHost, core->stream));
        HIP_TRY(core, hipMemcpyAsync(used.data(), KAI_VP(core->ctx.n_used), (size_t)R * N * 8, hipMemcpyDeviceToHost, core->stream));
    }
    HIP_TRY(core, hipStreamSynchronize(core->stream));
    for (int i = 0; i < N; i++) {
        kai_node_state& o = out[core->perm[i]];
        std::memset(&o, 0, sizeof(kai_node_state));
        for (int r = 0; r < R; r++) { o.idle[r] = idle[(size_t)r * N + i]; o.releasing[r] = rel[(size_t)r * N + i]; o.used[r] = used[(size_t)r * N + i]; }
    }
    return KAI_OK;
}

int kai_shard_attach(kai_core* core, int rank, int world, int offers_per_class, kai_allgather_fn fn, void* user) {
    if (!core || world < 1 || rank < 0 || rank >= world || (world > 1 && !fn)) return KAI_ERR_INVALID_ARG;
    if (core->open) return fail(core, KAI_ERR_STATE, "kai_shard_attach: before kai_session_open");
    core->world = world; core->rank = rank; core->shard_k = offers_per_class; core->ag_fn = fn; core->ag_user = user;
    return KAI_OK;
}

int kai_shard_attach_host(kai_core* core, kai_allgather_fn fn, void* user) {
    if (!core) return KAI_ERR_INVALID_ARG;
    core->xag_fn = fn; core->xag_user = user;
    return KAI_OK;
}

int kai_shard_rccl_id(kai_core* core, void* id_out) {
    if (!core || !id_out) return KAI_ERR_INVALID_ARG;
    RcclApi* a = rccl_api();
    if (!a) return fail(core, KAI_ERR_COMM, "kai_shard_rccl_id: librccl could not be loaded");
    RcclId id; const int rc = a->GetUniqueId(&id);
    if (rc) return rccl_fail(core, "ncclGetUniqueId", rc);
    std::memcpy(id_out, id.internal, sizeof id.internal);
    return KAI_OK;
}

int kai_shard_attach_rccl(kai_core* core, int rank, int world, int offers_per_class, const void* id) {
    if (!core || !id || world < 1 || rank < 0 || rank >= world) return KAI_ERR_INVALID_ARG;
    if (core->open) return fail(core, KAI_ERR_STATE, "kai_shard_attach_rccl: before kai_session_open");
    RcclApi* a = rccl_api();
    if (!a) return fail(core, KAI_ERR_COMM, "kai_shard_attach_rccl: librccl could not be loaded");
    HIP_TRY(core, hipSetDevice(core->device));
    if (core->rccl_comm) { (void)a->CommDestroy(core->rccl_comm); core->rccl_comm = nullptr; }
    RcclId uid; std::memcpy(uid.internal, id, sizeof uid.internal);
    void* comm = nullptr; const int rc = a->CommInitRank(&comm, world, uid, rank);
    if (rc) return rccl_fail(core, "ncclCommInitRank", rc);
    core->rccl_comm = comm; core->world = world; core->rank = rank; core->shard_k = offers_per_class; core->ag_fn = nullptr; core->ag_user = nullptr;
    return KAI_OK;
}

int kai_shard_allgather_probe(kai_core* core, const void* send, void* recv, int64_t bytes_per_rank) {
    if (!core || !send || !recv || bytes_per_rank <= 0) return KAI_ERR_INVALID_ARG;
    HIP_TRY(core, hipSetDevice(core->device));
    DevLauncher dl{core};
    if (int rc = dl.allgather(send, recv, bytes_per_rank)) return rc;
    HIP_TRY(core, hipStreamSynchronize(core->stream));
    return KAI_OK;
}

int kai_pod_gpu_groups(kai_core* core, int32_t* out, int cap) {
    if (!core || !out) return KAI_ERR_INVALID_ARG;
    if (!core->open) return fail(core, KAI_ERR_STATE, "no open session");
    const int P = core->ctx.P;
    if (cap < P) return fail(core, KAI_ERR_CAPACITY, "kai_pod_gpu_groups: cap < n_pods");
    HIP_TRY(core, hipSetDevice(core->device));
    std::vector<int32_t> st((size_t)std::max(P, 1)); std::vector<uint8_t> por((size_t)std::max(P, 1));
    if (P) { HIP_TRY(core, hipMemcpyAsync(out, KAI_VP(core->ctx.p_group), (size_t)P * 4, hipMemcpyDeviceToHost, core->stream));
             HIP_TRY(core, hipMemcpyAsync(st.data(), KAI_VP(core->ctx.p_status), (size_t)P * 4, hipMemcpyDeviceToHost, core->stream));
             HIP_TRY(core, hipMemcpyAsync(por.data(), KAI_VP(core->ctx.p_shared), (size_t)P, hipMemcpyDeviceToHost, core->stream)); }
    HIP_TRY(core, hipStreamSynchronize(core->stream));
    for (int p = 0; p < P; p++) if (!(core->shared && por[p] && (st[p] & KAI_POD_ACTIVE))) out[p] = -1;
    return KAI_OK;
}

int kai_action_stats_get(kai_core* core, kai_action_stats* out) {
    if (!core || !out) return KAI_ERR_INVALID_ARG;
    *out = core->stats;
    return KAI_OK;
}

}  // extern "C"
