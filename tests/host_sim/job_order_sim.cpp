// job_order_sim.cpp — TEST INFRASTRUCTURE: kai_job_order's kernel bodies and control flow (kai-scheduler_amd/csrc/kai_job_order.hpp: jo_drive, with the plan's own kb_static_rank /
// kb_static_check / kb_plan_setup / kb_plan_rank and the open's job_init_body / leaf_init_body) compiled with plain g++ and run with the emulated lanes of kai_simt.hpp on a session
// of the host simulation (sim_session.hpp: struct SimSession, opened and driven as kai_hostsim_run drives one).  tests/test_job_order.py compares the order with the oracle's
// JobsOrderByQueues (kai_oracle_jobs_order) and the session with a TWIN that never made the call.  NOT a CPU fallback: libkai_core never contains it; the parity claim is
// tests/test_gpu_job_order.py on the MI355X.
//
// The harness: open the session; run the actions `pre`; copy the state; make the call on its context; compare the state with the copy; run the actions `post`; read back.
//
// -DKAI_JOSIM_MAIN adds a main() with one fixed case (the stand-alone program the sanitizers are run on).
#include "sim_session.hpp"
#include "../../kai-scheduler_amd/csrc/kai_job_order.hpp"

namespace {

// the handle's scratch: grows, zero-filled where it grew, keeps what the last call left
struct JoScratch { std::vector<unsigned char> dev; };

struct JoSimLauncher {
    int launches = 0, reads = 0;
    void job_init(int g, int b, const KaiCtx& c) { launches++; kw::launch(g, b, 0, [&] { job_init_body(c); }); }
    void leaf_init(int g, int b, const KaiCtx& c) { launches++; kw::launch(g, b, 0, [&] { leaf_init_body(c); }); }
    void qualify(int g, int b, const KaiCtx& c, const JoArgs& a) { launches++; kw::launch(g, b, 0, [&] { jo_qualify_body(c, a); }); }
    void static_rank(int g, int b, const KaiCtx& c) { launches++; kw::launch(g, b, 0, [&] { kb_static_rank(c); }); }
    void static_check(int g, int b, const KaiCtx& c) { launches++; kw::launch(g, b, 0, [&] { kb_static_check(c); }); }
    void plan_setup(int g, int b, const KaiCtx& c, RoundParams rp) { launches++; kw::launch(g, b, 0, [&] { kb_plan_setup(c, rp); }); }
    void leaf(int g, int b, const KaiCtx& c, const JoArgs& a) { launches++; kw::launch(g, b, 0, [&] { jo_leaf_body(c, a); }); }
    void plan_rank(int g, int b, const KaiCtx& c, RoundParams rp) { launches++; kw::launch(g, b, 0, [&] { kb_plan_rank(c, rp); }); }
    void keys(int g, int b, const KaiCtx& c, const JoArgs& a, RoundParams rp) { launches++; kw::launch(g, b, 0, [&] { jo_keys_body(c, a, rp); }); }
    int64_t longest_tiles = 0;  // the most tiles a workgroup of the scan walked
    void scan(int g, int b, const KaiCtx& c, RoundParams rp) {
        launches++; kw::launch(g, b, 0, [&] { jo_scan_body(c, rp); });
        for (int i = c.bt.h_off[rp.height]; i < c.bt.h_off[rp.height + 1]; i++) { const int x = c.bt.h_nodes[i]; if (x != c.Q) longest_tiles = std::max<int64_t>(longest_tiles, (c.bt.q_cnt[x] + (int64_t)b * KB_PLAN_SCAN_ELEMS - 1) / ((int64_t)b * KB_PLAN_SCAN_ELEMS)); }
    }
    void emit(int g, int b, const KaiCtx& c, const JoArgs& a) { launches++; kw::launch(g, b, 0, [&] { jo_emit_body(c, a); }); }
    int engine(const KaiCtx& c, const JoArgs& a) { launches++; KaiCtx cv = c; cv.use_index = 0; HostBackend be; jo_engine_walk(cv, be, a); return 0; }  // as k_jo_engine: one lane, no class index
    int read_head(JoHead& hd, const JoArgs& a) { reads++; hd = *a.head; return 0; }
};

// kai_job_order from its first device call on (the refusals in front of it are host code of kai_core.hip, tested under tests/host_sim/fake_hip.cpp): order_out [cap],
// pos_out / qpos_out [J] or NULL; -> what the entry point would return.  tiles (may be NULL): the most tiles one workgroup of the scan walked.
int sim_job_order(SimSession& ss, JoScratch& sc, int depth_param, uint32_t flags, int lanes, int cap, int32_t* order_out, int32_t* n_out, int32_t* pos_out, int32_t* qpos_out,
                  kai_job_order_result& res, int64_t* tiles = nullptr) {
    const KaiCtx& c = ss.ctx();
    const int J = c.J, Q = c.Q, n_heights = ss.prep.n_heights;
    int depth = depth_param == 0 ? ss.cfg->queue_depth[KAI_ACTION_ALLOCATE] : depth_param;
    if (depth < 0) depth = 0;
    const size_t pool = jo_pool(J, Q, n_heights);
    const JoLayout L((size_t)J, (size_t)Q, (size_t)n_heights, pool);
    if (sc.dev.size() < L.end) sc.dev.assign(L.end + L.end / 4, 0);
    unsigned char* d = sc.dev.data();
    std::memset(d, 0, L.up_end);
    std::memcpy(d + L.q_height, ss.prep.q_height.data(), (size_t)(Q + 1) * 4);
    std::memcpy(d + L.h_off, ss.prep.h_off.data(), (size_t)(n_heights + 1) * 4);
    std::memcpy(d + L.h_nodes, ss.prep.h_nodes.data(), (size_t)(Q + 1) * 4);
    const KaiCtx cj = jo_bind_ctx(c, d, L, n_heights, pool, depth);
    const JoArgs a = jo_bind_args(c, d, L, pool);
    JoSimLauncher l; JoHead hd{}; int path = KAI_JOB_ORDER_PATH_NONE;
    const int status = jo_drive(l, cj, a, ss.prep.shape, jo_wide_session(c, n_heights, pool), depth, flags, lanes, hd, path);
    if (tiles) *tiles = l.longest_tiles;
    if (status != KAI_OK) return status;
    const int n = path == KAI_JOB_ORDER_PATH_NONE ? 0 : hd.n_ordered;
    if (n > cap) { *n_out = n; return KAI_ERR_CAPACITY; }
    if (n) std::memcpy(order_out, d + L.order, (size_t)n * 4);
    if (pos_out && J) std::memcpy(pos_out, d + L.pos, (size_t)J * 4);
    if (qpos_out && J) std::memcpy(qpos_out, d + L.qpos, (size_t)J * 4);
    *n_out = n;
    res.n_ordered = n; res.path = path; res.n_leaves = n ? hd.n_leaves : 0; res.pad = 0;
    return KAI_OK;
}

// what the call may re-derive (include/kai_core.h): the tasks-to-allocate caches' validity is the one word of StateCopy::hidden it may change
void mask_rederived(const KaiCtx& c, StateCopy& g) { for (int j = 0; j < c.J; j++) g.hidden[(size_t)4 * c.P + (size_t)4 * c.S + (size_t)8 * j + 1] = 0; }
bool same_state(const StateCopy& a, const StateCopy& b) {
    return a.p_status == b.p_status && a.p_node == b.p_node && a.hidden == b.hidden && a.n_idle.size() == b.n_idle.size() && a.shares.size() == b.shares.size() &&
           std::memcmp(a.n_idle.data(), b.n_idle.data(), a.n_idle.size() * 8) == 0 && std::memcmp(a.n_rel.data(), b.n_rel.data(), a.n_rel.size() * 8) == 0 &&
           std::memcmp(a.n_used.data(), b.n_used.data(), a.n_used.size() * 8) == 0 && std::memcmp(a.shares.data(), b.shares.data(), a.shares.size() * sizeof(QShare)) == 0;
}

}  // namespace

extern "C" {

// Runs the actions `pre` (batch: allocate actions may take the batch path), then — mode 0 — kai_job_order with `depth`, `flags` and a capacity of `cap` jobs in workgroups of
// `lanes` lanes (mode 1: no call, the twin), then the actions `post`.  call_status: what the entry point would return.  *unchanged: the state right behind the call (read-backs,
// the state no read-back shows, the action statistics, fast_ok, the class index's staleness) is the state right in front of it.  *tiles: the most tiles one workgroup of the
// scan walked.  ops_out ...: the operations of ALL actions and the final state, as kai_hostsim_run returns them.
int kai_josim_run(const kai_config* cfg, const kai_snapshot_soa* s, const int* pre, int n_pre, int batch, int mode, int depth, uint32_t flags, int lanes, int cap,
                  int32_t* order_out, int32_t* n_out, int32_t* pos_out, int32_t* qpos_out, kai_job_order_result* result, int* call_status, int* unchanged, int64_t* tiles,
                  const int* post, int n_post, kai_op* ops_out, int64_t ops_cap, int64_t* n_ops, int32_t* pod_status_out, int32_t* pod_node_out, kai_queue_share* shares_final,
                  kai_node_state* nodes_out) {
    if (!cfg || !s || n_pre < 0 || n_post < 0 || lanes < 1 || lanes > 4096 || (mode != 0 && mode != 1) || (mode == 0 && (!n_out || cap < 0 || (cap > 0 && !order_out)))) return KAI_ERR_INVALID_ARG;
    SimSession ss;
    if (int rc = ss.open(cfg, s, n_pre + n_post, batch != 0)) return rc;
    for (int i = 0; i < n_pre; i++) if (int rc = ss.action(pre[i])) return rc;
    static JoScratch scratch; int status = KAI_OK; kai_job_order_result res{}; int same = 1; int64_t nt = 0;
    if (mode == 0) {
        StateCopy before = ss.snapshot_state(); kai_action_stats st0{}, st1{}; ss.stats(&st0);
        const int fast0 = ss.ctx().fast_ok, act0 = ss.ctx().action, depth0 = ss.ctx().queue_depth; const bool stale0 = ss.index_stale; const EngineState es0 = *ss.ctx().st;
        status = sim_job_order(ss, scratch, depth, flags, lanes, cap, order_out, n_out, pos_out, qpos_out, res, &nt);
        StateCopy after = ss.snapshot_state(); ss.stats(&st1);
        mask_rederived(ss.ctx(), before); mask_rederived(ss.ctx(), after);
        same = same_state(before, after) && std::memcmp(&st0, &st1, sizeof st0) == 0 && fast0 == ss.ctx().fast_ok && act0 == ss.ctx().action && depth0 == ss.ctx().queue_depth &&
               stale0 == ss.index_stale && std::memcmp(&es0, ss.ctx().st, sizeof es0) == 0;
    }
    for (int i = 0; i < n_post; i++) if (int rc = ss.action(post[i])) return rc;
    if (int rc = ss.finish()) return rc;
    if (call_status) *call_status = status;
    if (result) *result = res;
    if (unchanged) *unchanged = same;
    if (tiles) *tiles = nt;
    if (int rc = ss.ops(ops_out, ops_cap, n_ops)) return rc;
    ss.pod_state(pod_status_out, pod_node_out); ss.shares(shares_final); ss.nodes(nodes_out);
    return KAI_OK;
}

}  // extern "C"

#ifdef KAI_JOSIM_MAIN
// One fixed case: 4 nodes of 8 GPUs; queues: two departments (0, 1) with two teams each (2, 3 under 0; 4, 5 under 1) and a top-level leaf (6); NJ pending gangs of one to three
// one-GPU pods spread over the five leaves with priorities and creation times that interleave, and a few running jobs that give the queues different shares.  The call with
// 256, 100 and 1 lanes, both paths, fresh and behind an allocate, at depth -1, 2 and 1: the two paths agree, the positions are the inverse of the order, the per-queue positions
// count up inside every leaf, the depth caps every leaf, the session is as it was, a capacity below the count reports the count and writes nothing.
int main() {
    const int N = 4, Q = 7, NJ = 150, RUN = 6, J = NJ + RUN, R = 4;
    std::vector<int32_t> jnp(J), jfp(J), jq(J), jprio(J), jpre(J, 1), jfps(J), jnps(J, 1); std::vector<int64_t> jcreated(J); std::vector<uint32_t> juid(J);
    const int leaves[5] = {2, 3, 4, 5, 6};
    int P = 0;
    for (int j = 0; j < J; j++) { jnp[j] = 1 + j % 3; jfp[j] = P; P += jnp[j]; jq[j] = leaves[(j * 7 + j / 5) % 5]; jprio[j] = 50 + (j * 13) % 3; jfps[j] = j; juid[j] = (uint32_t)(J - 1 - j); jcreated[j] = 1000 + (j * 37) % 101; }
    const int S = J;
    std::vector<double> alloc((size_t)R * N), req((size_t)R * P);
    std::vector<uint32_t> nflags(N, 0u), nrank(N), pflags(P, 0u), puid(P), quid(Q), psrank(S, 0u);
    std::vector<int32_t> ngc(N, -1), ncls(N, 0), pjob(P), pps(P), pst(P), pnode(P), pprio(P, 0), pcls(P, 0), pnom(P, -1), psjob(S), psmin(S), qpar = {-1, -1, 0, 0, 1, 1, -1}, qprio = {0, 0, 0, 1, 0, 0, 0};
    std::vector<int64_t> pcreated(P), qcreated(Q);
    for (int n = 0; n < N; n++) { nrank[n] = (uint32_t)(N - 1 - n); alloc[0 * N + n] = 64000; alloc[1 * N + n] = 256000; alloc[2 * N + n] = 8; alloc[3 * N + n] = 110; }
    for (int j = 0; j < J; j++) { psjob[j] = j; psmin[j] = jnp[j]; }
    for (int p = 0, j = 0; p < P; p++) {
        while (p >= jfp[j] + jnp[j]) j++;
        pjob[p] = j; pps[p] = j; puid[p] = (uint32_t)p; pcreated[p] = 2000 + p;
        const bool running = j >= NJ;
        pst[p] = running ? KAI_POD_RUNNING : KAI_POD_PENDING; pnode[p] = running ? p % N : -1;
        req[0 * P + p] = 1000; req[1 * P + p] = 4000; req[2 * P + p] = 1; req[3 * P + p] = 1;
    }
    for (int q = 0; q < Q; q++) { quid[q] = (uint32_t)q; qcreated[q] = 10 + (q * 3) % 7; }
    std::vector<double> qdes((size_t)3 * Q), qlim((size_t)3 * Q, -1.0), qoqw((size_t)3 * Q, 1.0);
    const double dg[Q] = {12, 12, 6, 6, 8, 4, 8};
    for (int q = 0; q < Q; q++) { qdes[0 * Q + q] = dg[q] * 8000; qdes[1 * Q + q] = dg[q] * 32000; qdes[2 * Q + q] = dg[q]; }
    const uint8_t fit = 1;
    kai_snapshot_soa s; std::memset(&s, 0, sizeof s);
    s.abi_version = KAI_ABI_VERSION; s.n_res = R;
    s.n_nodes = N; s.node_allocatable = alloc.data(); s.node_flags = nflags.data(); s.node_gpu_count = ngc.data(); s.node_name_rank = nrank.data(); s.node_class = ncls.data();
    s.n_pods = P; s.pod_req = req.data(); s.pod_job = pjob.data(); s.pod_podset = pps.data(); s.pod_status = pst.data(); s.pod_node = pnode.data(); s.pod_flags = pflags.data();
    s.pod_task_priority = pprio.data(); s.pod_created_ns = pcreated.data(); s.pod_uid_rank = puid.data(); s.pod_class = pcls.data(); s.pod_nominated_node = pnom.data();
    s.n_podsets = S; s.podset_job = psjob.data(); s.podset_min_available = psmin.data(); s.podset_name_rank = psrank.data();
    s.n_jobs = J; s.job_queue = jq.data(); s.job_priority = jprio.data(); s.job_preemptible = jpre.data(); s.job_created_ns = jcreated.data(); s.job_uid_rank = juid.data();
    s.job_first_pod = jfp.data(); s.job_n_pods = jnp.data(); s.job_first_podset = jfps.data(); s.job_n_podsets = jnps.data();
    s.n_queues = Q; s.queue_parent = qpar.data(); s.queue_priority = qprio.data(); s.queue_created_ns = qcreated.data(); s.queue_uid_rank = quid.data();
    s.queue_deserved = qdes.data(); s.queue_limit = qlim.data(); s.queue_oqw = qoqw.data();
    s.n_pod_classes = 1; s.n_node_classes = 1; s.class_fit = &fit;
    kai_config cfg; std::memset(&cfg, 0, sizeof cfg);
    cfg.abi_version = KAI_ABI_VERSION; cfg.k_value = 1.0; cfg.reclaimer_saturation_multiplier = 1.0; cfg.plugins = KAI_PLUGIN_ALL; cfg.max_consolidation_preemptees = 16;
    cfg.allow_consolidating_reclaim = 1; cfg.full_hierarchy_fairness = 1; cfg.min_node_gpu_memory = 100; for (int i = 0; i < 4; i++) cfg.queue_depth[i] = -1;
    cfg.now_ns = 1;

    struct Out { int rc = 99, status = 99, same = 0; kai_job_order_result res{}; std::vector<int32_t> order, pos, qpos, st, nd; int32_t n = -3; std::vector<kai_op> ops; };
    const int ALLOC[1] = {KAI_ACTION_ALLOCATE};
    auto run = [&](bool pre, int mode, int depth, uint32_t flags, int lanes, int cap, bool post, Out& o) {
        o.order.assign((size_t)J, -9); o.pos.assign((size_t)J, -9); o.qpos.assign((size_t)J, -9); o.st.assign(P, 0); o.nd.assign(P, 0); o.ops.assign((size_t)8 * P + 64, kai_op{}); int64_t nops = 0;
        o.rc = kai_josim_run(&cfg, &s, pre ? ALLOC : nullptr, pre ? 1 : 0, 0, mode, depth, flags, lanes, cap, o.order.data(), &o.n, o.pos.data(), o.qpos.data(), &o.res, &o.status, &o.same, nullptr,
                             post ? ALLOC : nullptr, post ? 1 : 0, o.ops.data(), (int64_t)o.ops.size(), &nops, o.st.data(), o.nd.data(), nullptr, nullptr);
        o.ops.resize((size_t)nops);
        return o.rc;
    };
    int bad = 0, checks = 0;
    auto expect = [&](bool ok, const char* what) { checks++; if (!ok) { bad++; std::printf("FAILED: %s\n", what); } };
    auto consistent = [&](const Out& o, int depth) {
        if (o.n < 0 || o.n > J) return false;
        std::vector<int> seen((size_t)J, 0), per_leaf((size_t)Q, 0);
        for (int t = 0; t < o.n; t++) {
            const int j = o.order[(size_t)t]; if (j < 0 || j >= NJ || seen[(size_t)j]++) return false;
            if (o.pos[(size_t)j] != t || o.qpos[(size_t)j] != per_leaf[(size_t)jq[j]]++) return false;
        }
        for (int j = 0; j < J; j++) if (!seen[(size_t)j] && (o.pos[(size_t)j] != -1 || o.qpos[(size_t)j] != -1)) return false;
        if (depth > 0) for (int q = 0; q < Q; q++) if (per_leaf[(size_t)q] > depth) return false;
        int leaves_in = 0; for (int q = 0; q < Q; q++) if (per_leaf[(size_t)q]) leaves_in++;
        return o.res.n_ordered == o.n && o.res.n_leaves == leaves_in;
    };
    for (bool pre : {false, true}) for (int depth : {-1, 2, 1}) {
        Out first; bool have = false;
        for (int lanes : {256, 100, 1}) {
            Out w, e;
            expect(run(pre, 0, depth, 0, lanes, J, false, w) == 0 && w.status == KAI_OK && w.res.path == KAI_JOB_ORDER_PATH_WIDE, "the call on the chip-wide path");
            expect(run(pre, 0, depth, KAI_JOB_ORDER_ENGINE_PATH, lanes, J, false, e) == 0 && e.status == KAI_OK && e.res.path == KAI_JOB_ORDER_PATH_ENGINE, "the call on the engine path");
            expect(consistent(w, depth) && consistent(e, depth), "order, positions and per-queue positions belong together");
            expect(w.n == e.n && w.order == e.order && w.pos == e.pos && w.qpos == e.qpos && w.res.n_leaves == e.res.n_leaves, "the two paths agree");
            expect(w.same && e.same, "the call changes nothing");
            if (!pre && depth == -1) expect(w.n == NJ, "every pending job is in the order");
            if (depth == 1) expect(w.n == 5, "depth 1: one job per leaf");
            if (!have) { first = w; have = true; } else expect(w.order == first.order && w.n == first.n, "every workgroup size: the same order");
        }
        Out small; expect(run(pre, 0, depth, 0, 256, first.n - 1, false, small) == 0 && small.status == KAI_ERR_CAPACITY && small.n == first.n && small.order[0] == -9 && small.pos[0] == -9 && small.same, "a capacity below the count: the count needed, nothing written");
    }
    {   Out a, b; expect(run(false, 0, -1, 0, 256, J, true, a) == 0 && a.status == KAI_OK, "allocate behind the call");
        expect(run(false, 1, -1, 0, 256, J, true, b) == 0, "allocate on the twin");
        expect(a.ops.size() == b.ops.size() && !a.ops.empty() && std::memcmp(a.ops.data(), b.ops.data(), a.ops.size() * sizeof(kai_op)) == 0 && a.st == b.st && a.nd == b.nd, "the next allocate commits the same operations");
        Out c0, c1; expect(run(true, 0, -1, 0, 256, J, false, c0) == 0 && run(false, 0, -1, 0, 256, J, false, c1) == 0 && c0.n < c1.n && c0.n > 0, "behind an allocate fewer jobs are queued"); }
    for (char* st : kw::emu().stacks) std::free(st);  // the emulator keeps its fibers' stacks for the life of the process: handed back so that a leak check ends clean
    kw::emu().stacks.clear();
    std::printf(bad ? "job_order_sim: %d of %d checks FAILED\n" : "job_order_sim: ok (%d checks)\n", bad ? bad : checks, checks);
    return bad ? 1 : 0;
}
#endif
