// ops_apply_sim.cpp — TEST INFRASTRUCTURE: kai_ops_apply's kernel bodies and control flow (kai-scheduler_amd/csrc/kai_ops_apply.hpp) compiled with plain g++ and run with
// the emulated lanes of kai_simt.hpp on a session of the host simulation (sim_session.hpp: struct SimSession, opened and driven as kai_hostsim_run drives one).
// tests/test_ops_apply.py replays the oracle's operations into such a session and compares states, shares and the operations of the actions run afterwards with the oracle.
// NOT a CPU fallback: libkai_core never contains it; the parity claim is tests/test_gpu_ops_apply.py on the MI355X.
//
// The harness: open the session; run the actions `pre`; apply the batch on its context — check kernel, chip-wide apply, engine walk, through the same oa_drive the library
// uses, and what kai_core.hip does on the host afterwards (sim_session.hpp sim_ops_apply); copy the state right behind the apply; run the actions `post`; read back.
//
// -DKAI_OASIM_MAIN adds a main() with one fixed case (the stand-alone program the sanitizers are run on).
#include "sim_session.hpp"

extern "C" {

// Runs the actions `pre`, applies `batch` (nodes: caller's indices) with `flags` and workgroups of `lanes` lanes, runs the actions `post`.  The batch goes in as n_calls
// calls, one after the other: call k = operations [call_off[k], call_off[k + 1]) (call_off NULL: one call); paths_out[k] = the path that took call k; a refused call ends it
// (its status and result are what the caller sees).
//   apply_status / result: what kai_ops_apply would return for the batch;
//   mid_*: pod states, node states and shares right behind the apply; hidden / hidden_cap / n_hidden: the state no read-back shows at that point (sim_session.hpp StateCopy);
//   ops_out ...: the operations of ALL actions (pre and post) and the final state, as kai_hostsim_run returns them (no post action: the state behind the apply).
int kai_oasim_run(const kai_config* cfg, const kai_snapshot_soa* s, const int* pre, int n_pre, const kai_op* batch, int64_t n_batch, uint32_t flags, int lanes,
                  const int64_t* call_off, int n_calls, int32_t* paths_out, const int* post, int n_post, int* apply_status, kai_apply_result* result,
                  int32_t* mid_status, int32_t* mid_node, kai_queue_share* mid_shares, kai_node_state* mid_nodes, int32_t* hidden, int64_t hidden_cap, int64_t* n_hidden,
                  kai_op* ops_out, int64_t ops_cap, int64_t* n_ops, int32_t* pod_status_out, int32_t* pod_node_out, kai_queue_share* shares_final, kai_node_state* nodes_out) {
    if (!cfg || !s || n_pre < 0 || n_post < 0 || n_batch < 0 || lanes < 1 || lanes > 4096 || s->n_jobs < 1 || n_calls < 1) return KAI_ERR_INVALID_ARG;
    for (int64_t i = 0; i < n_batch; i++) if (batch[i].node < 0 || batch[i].node >= s->n_nodes || batch[i].pod < 0 || batch[i].pod >= s->n_pods || batch[i].kind < 0 || batch[i].kind > 2) return KAI_ERR_INVALID_ARG;
    SimSession ss;
    if (int rc = ss.open(cfg, s, n_pre + n_post, n_post > 0)) return rc;  // (as it always was: without a post action, `pre` runs on the sequential engine — the two paths of allocate leave different p_accepted / j_tta_valid words in `hidden`)
    for (int i = 0; i < n_pre; i++) if (int rc = ss.action(pre[i])) return rc;
    static ApplyScratch scratch; int status = KAI_OK; kai_apply_result res{};
    for (int k = 0; k < (call_off ? n_calls : 1); k++) {
        const int64_t lo = call_off ? call_off[k] : 0, hi = call_off ? call_off[k + 1] : n_batch;
        status = sim_ops_apply(ss, scratch, batch + lo, (int)(hi - lo), flags, lanes, res);
        if (paths_out) paths_out[k] = res.path;
        if (status != KAI_OK) break;
    }
    const StateCopy mid = ss.snapshot_state();
    for (int i = 0; i < n_post; i++) if (int rc = ss.action(post[i])) return rc;
    if (int rc = ss.finish()) return rc;
    if (apply_status) *apply_status = status;
    if (result) *result = res;
    if (int rc = ss.write(mid, mid_status, mid_node, mid_shares, mid_nodes, hidden, hidden_cap, n_hidden)) return rc;
    if (int rc = ss.ops(ops_out, ops_cap, n_ops)) return rc;
    ss.pod_state(pod_status_out, pod_node_out); ss.shares(shares_final); ss.nodes(nodes_out);
    return KAI_OK;
}

}  // extern "C"

#ifdef KAI_OASIM_MAIN
// One fixed case: 6 nodes of 8 GPUs whose name ranks are the reverse of their indices, 3 queues, 12 jobs of 3 one-GPU pods — six of them running, six pending.  Three batches:
// allocations only; evictions, a pipeline and allocations in several Statements, every pod once (the chip-wide path takes both); a pod evicted and pipelined again (the engine
// walk).  Each with 256, 100 and 1 lanes and on both paths: the same state everywhere, a few amounts checked against plain arithmetic; a batch with a bad operation writes nothing.
int main() {
    const int N = 6, Q = 3, J = 12, PJ = 3, P = J * PJ, R = 4;
    std::vector<double> alloc((size_t)R * N), req((size_t)R * P);
    std::vector<uint32_t> nflags(N, 0u), nrank(N), pflags(P, 0u), puid(P), juid(J), quid(Q), psrank(J, 0u);
    std::vector<int32_t> ngc(N, -1), ncls(N, 0), pjob(P), pps(P), pst(P), pnode(P), pprio(P, 0), pcls(P, 0), pnom(P, -1), psjob(J), psmin(J, 1), jq(J), jprio(J, 50), jpre(J), jfp(J), jnp(J, PJ), jfps(J), jnps(J, 1), qpar = {-1, 0, 0}, qprio(Q, 0);
    std::vector<int64_t> pcreated(P), jcreated(J), qcreated(Q);
    for (int n = 0; n < N; n++) { nrank[n] = (uint32_t)(N - 1 - n); alloc[0 * N + n] = 64000; alloc[1 * N + n] = 256000; alloc[2 * N + n] = 8; alloc[3 * N + n] = 110; }
    for (int j = 0; j < J; j++) { psjob[j] = j; jq[j] = 1 + j % 2; jpre[j] = j % 3 != 0; jfp[j] = j * PJ; jfps[j] = j; juid[j] = (uint32_t)j; jcreated[j] = 1000 + j; }
    for (int p = 0; p < P; p++) {
        const int j = p / PJ; pjob[p] = j; pps[p] = j; puid[p] = (uint32_t)p; pcreated[p] = 2000 + p;
        pst[p] = j < 6 ? KAI_POD_RUNNING : KAI_POD_PENDING; pnode[p] = j < 6 ? p % N : -1;
        req[0 * P + p] = 1000; req[1 * P + p] = 4000; req[2 * P + p] = 1; req[3 * P + p] = 1;
    }
    for (int q = 0; q < Q; q++) { quid[q] = (uint32_t)q; qcreated[q] = 10 + q; }
    std::vector<double> qdes = {384000, 192000, 192000, 1536000, 768000, 768000, 48, 24, 24}, qlim(9, -1.0), qoqw(9, 1.0);
    const uint8_t fit = 1;
    kai_snapshot_soa s; std::memset(&s, 0, sizeof s);
    s.abi_version = KAI_ABI_VERSION; s.n_res = R;
    s.n_nodes = N; s.node_allocatable = alloc.data(); s.node_flags = nflags.data(); s.node_gpu_count = ngc.data(); s.node_name_rank = nrank.data(); s.node_class = ncls.data();
    s.n_pods = P; s.pod_req = req.data(); s.pod_job = pjob.data(); s.pod_podset = pps.data(); s.pod_status = pst.data(); s.pod_node = pnode.data(); s.pod_flags = pflags.data();
    s.pod_task_priority = pprio.data(); s.pod_created_ns = pcreated.data(); s.pod_uid_rank = puid.data(); s.pod_class = pcls.data(); s.pod_nominated_node = pnom.data();
    s.n_podsets = J; s.podset_job = psjob.data(); s.podset_min_available = psmin.data(); s.podset_name_rank = psrank.data();
    s.n_jobs = J; s.job_queue = jq.data(); s.job_priority = jprio.data(); s.job_preemptible = jpre.data(); s.job_created_ns = jcreated.data(); s.job_uid_rank = juid.data();
    s.job_first_pod = jfp.data(); s.job_n_pods = jnp.data(); s.job_first_podset = jfps.data(); s.job_n_podsets = jnps.data();
    s.n_queues = Q; s.queue_parent = qpar.data(); s.queue_priority = qprio.data(); s.queue_created_ns = qcreated.data(); s.queue_uid_rank = quid.data();
    s.queue_deserved = qdes.data(); s.queue_limit = qlim.data(); s.queue_oqw = qoqw.data();
    s.n_pod_classes = 1; s.n_node_classes = 1; s.class_fit = &fit;
    kai_config cfg; std::memset(&cfg, 0, sizeof cfg);
    cfg.abi_version = KAI_ABI_VERSION; cfg.k_value = 1.0; cfg.reclaimer_saturation_multiplier = 1.0; cfg.plugins = KAI_PLUGIN_ALL; cfg.max_consolidation_preemptees = 16;
    cfg.allow_consolidating_reclaim = 1; cfg.full_hierarchy_fairness = 1; cfg.min_node_gpu_memory = 100; for (int i = 0; i < 4; i++) cfg.queue_depth[i] = -1;

    auto op = [](int kind, int pod, int node, int stmt) { kai_op o; std::memset(&o, 0, sizeof o); o.kind = kind; o.pod = pod; o.node = node; o.stmt = stmt; o.job = -1; return o; };
    std::vector<std::vector<kai_op>> batches(3);
    for (int p = 18; p < 27; p++) batches[0].push_back(op(KAI_OP_ALLOCATE, p, p % N, (p - 18) / 3));
    batches[1] = {op(KAI_OP_EVICT, 0, 0, 0), op(KAI_OP_EVICT, 7, 1, 0), op(KAI_OP_PIPELINE, 30, 0, 0), op(KAI_OP_ALLOCATE, 18, 5, 1), op(KAI_OP_ALLOCATE, 19, 5, 1), op(KAI_OP_EVICT, 3, 3, 4), op(KAI_OP_ALLOCATE, 33, 2, 4)};
    batches[2] = {op(KAI_OP_EVICT, 4, 4, 0), op(KAI_OP_PIPELINE, 4, 2, 0), op(KAI_OP_ALLOCATE, 20, 1, 1), op(KAI_OP_EVICT, 20, 1, 2), op(KAI_OP_PIPELINE, 20, 1, 2), op(KAI_OP_EVICT, 5, 5, 3), op(KAI_OP_EVICT, 5, 5, 3)};
    struct Out { int status = 99; kai_apply_result res{}; std::vector<int32_t> st, nd, hidden; std::vector<kai_queue_share> sh; std::vector<kai_node_state> ns; };
    auto run = [&](const std::vector<kai_op>& b, uint32_t flags, int lanes, Out& o) {
        o.st.assign(P, 0); o.nd.assign(P, 0); o.hidden.assign((size_t)4 * P + 4 * J + 8 * J + 8, 0); o.sh.resize(Q); o.ns.resize(N); int64_t nh = 0, nops = 0;
        std::vector<kai_op> ops((size_t)8 * P + 64);
        const int rc = kai_oasim_run(&cfg, &s, nullptr, 0, b.data(), (int64_t)b.size(), flags, lanes, nullptr, 1, nullptr, nullptr, 0, &o.status, &o.res, o.st.data(), o.nd.data(), o.sh.data(), o.ns.data(),
                                     o.hidden.data(), (int64_t)o.hidden.size(), &nh, ops.data(), (int64_t)ops.size(), &nops, nullptr, nullptr, nullptr, nullptr);
        o.hidden.resize((size_t)nh);
        return rc;
    };
    auto same = [&](const Out& a, const Out& b) {
        return a.status == b.status && a.st == b.st && a.nd == b.nd && a.hidden == b.hidden && std::memcmp(a.sh.data(), b.sh.data(), sizeof(kai_queue_share) * Q) == 0 &&
               std::memcmp(a.ns.data(), b.ns.data(), sizeof(kai_node_state) * N) == 0;
    };
    int bad = 0, checks = 0;
    auto expect = [&](bool ok, const char* what) { checks++; if (!ok) { bad++; std::printf("FAILED: %s\n", what); } };
    Out open; expect(run({}, 0, 256, open) == 0 && open.status == 0, "the untouched session");
    for (int bi = 0; bi < 3; bi++) {
        Out first; bool have = false;
        for (uint32_t flags : {0u, (uint32_t)KAI_APPLY_ENGINE_PATH}) for (int lanes : {256, 100, 1}) {
            Out o; expect(run(batches[bi], flags, lanes, o) == 0 && o.status == KAI_OK && o.res.first_bad == -1, "a valid batch is taken");
            expect(o.res.path == ((flags || bi == 2) ? KAI_APPLY_PATH_ENGINE : KAI_APPLY_PATH_WIDE), "the path");
            if (!have) { first = o; have = true; } else expect(same(o, first), "both paths and every workgroup size leave the same state");
        }
        if (bi == 0) { expect(first.res.statements == 3 && first.st[18] == KAI_POD_BINDING && first.nd[18] == 0 && first.ns[0].idle[2] == open.ns[0].idle[2] - 2 && first.ns[0].used[2] == open.ns[0].used[2] + 2, "allocations: Binding, two GPUs of node 0 taken");
                       expect(first.sh[1].allocated[2] + first.sh[2].allocated[2] == open.sh[1].allocated[2] + open.sh[2].allocated[2] + 9 && first.sh[0].allocated[2] == open.sh[0].allocated[2] + 9, "allocations: nine GPUs more in the queues"); }
        if (bi == 1) expect(first.res.statements == 3 && first.st[0] == KAI_POD_RELEASING && first.nd[0] == 0 && first.st[30] == KAI_POD_PIPELINED && first.ns[0].releasing[2] == 0 && first.ns[0].idle[2] == open.ns[0].idle[2] &&
                            first.ns[0].used[2] == open.ns[0].used[2] + 1 && first.ns[1].releasing[2] == 1, "evict + pipeline on node 0: its Releasing GPU pays for the pipelined pod");
        if (bi == 2) expect(first.st[4] == KAI_POD_PIPELINED && first.nd[4] == 2 && first.ns[4].releasing[2] == 1 && first.ns[2].releasing[2] == -1 && first.st[20] == KAI_POD_PIPELINED && first.st[5] == KAI_POD_RELEASING && first.ns[5].releasing[2] == 1,
                            "a pod evicted and pipelined again lives on two nodes");
        Out chk; expect(run(batches[bi], KAI_APPLY_CHECK_ONLY, 256, chk) == 0 && chk.status == KAI_OK && chk.st == open.st && chk.hidden == open.hidden && std::memcmp(chk.ns.data(), open.ns.data(), sizeof(kai_node_state) * N) == 0, "check only writes nothing");
    }
    {   std::vector<kai_op> b = batches[1]; b.insert(b.begin() + 3, op(KAI_OP_EVICT, 31, 0, 0));  // a pending pod has no node
        for (uint32_t flags : {0u, (uint32_t)KAI_APPLY_ENGINE_PATH}) { Out o; expect(run(b, flags, 100, o) == 0 && o.status == KAI_ERR_STATE && o.res.first_bad == 3 && o.st == open.st && o.hidden == open.hidden && std::memcmp(o.ns.data(), open.ns.data(), sizeof(kai_node_state) * N) == 0, "a refused batch writes nothing"); }
        b = batches[2]; b.push_back(op(KAI_OP_ALLOCATE, 4, 0, 9));  // pipelined by then
        Out o; expect(run(b, 0, 256, o) == 0 && o.status == KAI_ERR_STATE && o.res.first_bad == (int64_t)b.size() - 1 && o.st == open.st && o.hidden == open.hidden, "... also when only the walk over the shadow can tell"); }
    for (char* st : kw::emu().stacks) std::free(st);  // the emulator keeps its fibers' stacks for the life of the process: handed back so that a leak check ends clean
    kw::emu().stacks.clear();
    std::printf(bad ? "ops_apply_sim: %d of %d checks FAILED\n" : "ops_apply_sim: ok (%d checks)\n", bad ? bad : checks, checks);
    return bad ? 1 : 0;
}
#endif
