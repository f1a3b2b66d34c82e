// ops_apply_sim.cpp — TEST INFRASTRUCTURE: kai_ops_apply's kernel bodies and control flow (kai-scheduler_amd/csrc/kai_ops_apply.hpp) compiled with plain g++ and run with
// the emulated lanes of kai_simt.hpp on a session set up exactly as the host simulation sets one up: this file INCLUDES host_sim.cpp.  tests/test_ops_apply.py replays the
// oracle's operations into such a session and compares states, shares and the operations of the actions run afterwards with the oracle.  NOT a CPU fallback: libkai_core
// never contains it; the parity claim is tests/test_gpu_ops_apply.py on the MI355X.
//
// How the batch gets INTO kai_hostsim_run's cycle: that function calls job_init_state(c, 0) first thing in every action (its twin of k_job_init).  The headers are included
// here first, then the name is routed through oasim_job_init_state for the text of host_sim.cpp only; in front of action number `at` the hook applies the batch — check
// kernel, chip-wide apply, engine walk, through the same oa_drive the library uses — does what kai_core.hip does on the host afterwards (class index, fast_ok) and keeps
// a copy of the state right behind the apply.  (The one macro host_sim.cpp defines in front of those headers, KAI_DOM_LANES_MIN, is defined the same way here.)
//
// -DKAI_OASIM_MAIN adds a main() with one fixed case (the stand-alone program the sanitizers are run on).
#define KAI_SHARED_GPUS 1
#include <cstdlib>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>
namespace kai { extern int oasim_dom_lanes_min; }
#define KAI_DOM_LANES_MIN ::kai::oasim_dom_lanes_min
#include "../../kai-scheduler_amd/csrc/kai_host_prep.hpp"
#include "../../kai-scheduler_amd/csrc/kai_batch_kernels.hpp"
#include "../../kai-scheduler_amd/csrc/kai_batch_driver.hpp"
#include "../../kai-scheduler_amd/csrc/kai_victim_shard.hpp"
#include "../../kai-scheduler_amd/csrc/kai_ops_apply.hpp"
#undef KAI_DOM_LANES_MIN
namespace kai { int oasim_dom_lanes_min = 16; }

static uint8_t oasim_job_init_state(const kai::KaiCtx& c, int j);
#define job_init_state(c, j) oasim_job_init_state(c, j)
#include "host_sim.cpp"
#undef job_init_state

namespace {

struct OaSim {
    bool on = false; int at = 0, seen = 0, lanes = 256;
    const kai_op* ops = nullptr; int64_t n = 0; uint32_t flags = 0; const uint32_t* rank = nullptr;  // the batch (caller's node indices), node index -> name rank
    const int64_t* call_off = nullptr; int n_calls = 1; std::vector<int32_t> paths;                   // the batch goes in as n_calls calls: call k = operations [call_off[k], call_off[k + 1])
    int status = 0; kai_apply_result res{}; int64_t n_ops_before = 0;  // operations the cycle had committed when the batch was applied
    std::vector<int32_t> p_status, p_node, hidden; std::vector<double> n_idle, n_rel, n_used; std::vector<QShare> shares;  // the state right behind the apply
} g_oa;

struct SimLauncher {
    void check(int g, int b, const KaiCtx& c, const OaArgs& a) { kw::launch(g, b, 0, [&] { oa_check_body(c, a); }); }
    void wide(int g, int b, const KaiCtx& c, const OaArgs& a) { kw::launch(g, b, 0, [&] { oa_wide_body(c, a); }); }
    int engine(const KaiCtx& c, const OaArgs& a) { KaiCtx cv = c; cv.use_index = 0; HostBackend be; oa_engine_walk(cv, be, a); return 0; }  // as k_oa_engine: one lane, no class index
    int read_head(OaHead& hv, const OaArgs& a) { hv = *a.head; return 0; }
};

// kai_ops_apply from its first device call on (the refusals in front of it are host code of kai_core.hip, tested under tests/host_sim/fake_hip.cpp)
void oasim_call(KaiCtx& c, const kai_op* src, int n) {
    OaSim& g = g_oa;
    g.res.first_bad = -1; g.res.path = KAI_APPLY_PATH_NONE; g.res.statements = 0; g.status = KAI_OK;
    if (!n) return;
    static std::vector<int32_t> stamp, sh_status, sh_node;  // the handle's scratch: zero between calls
    if ((int)stamp.size() < c.P) { stamp.assign((size_t)c.P, 0); sh_status.assign((size_t)c.P, 0); sh_node.assign((size_t)c.P, 0); }
    std::vector<kai_op> ops(src, src + n); bool non_alloc = false; int statements = 1;
    for (int i = 0; i < n; i++) { ops[i].node = (int32_t)g.rank[ops[i].node]; if (ops[i].kind != KAI_OP_ALLOCATE) non_alloc = true; if (i && ops[i].stmt != ops[i - 1].stmt) statements++; }
    OaHead head{}; head.bad = KAI_OA_NONE;
    OaArgs a{}; a.n = n; a.flags = g.flags | (oa_wide_session(c) ? 0u : KAI_OA_NOT_WIDE); a.use_islot = oa_use_islot(c);
    a.ops = ops.data(); a.head = &head; a.stamp = stamp.data(); a.sh_status = sh_status.data(); a.sh_node = sh_node.data();
    SimLauncher l; OaHead hv{}; int path = 0;
    g.status = oa_drive(l, c, a, g.lanes, hv, path);
    if (g.status == KAI_ERR_STATE) g.res.first_bad = hv.bad;
    if (g.status == KAI_OK) { g.res.path = path; g.res.statements = statements; }
    for (int p = 0; p < c.P; p++) if (stamp[p] || sh_status[p]) g.status = KAI_ERR_DEVICE_FAULT;  // the scratch must be clean again
    if (g.status == KAI_OK && !(g.flags & KAI_APPLY_CHECK_ONLY)) {  // the host side behind the kernels (kai_core.hip)
        if (c.use_index) for (int b = 0; b < c.NB; b++) for (int k = 0; k < c.C; k++) HostBackend::build_block(c, k, b);  // index_stale
        if (non_alloc) c.fast_ok = 0;
    }
}
void oasim_apply(KaiCtx& c) {
    OaSim& g = g_oa;
    g.n_ops_before = c.st->out_len; g.paths.clear();
    if (g.at == 0) for (int q = 0; q < c.Q; q++) qnode_init(c, q, 0);  // k_qnode_static of the open (kai_session_open.hpp launch_open_kernels): the host simulation fills the tree in its first action only, and the event handlers walk its parents
    for (int k = 0; k < g.n_calls; k++) {  // (a refused call ends the sequence: its status and result are what the caller sees)
        const int64_t lo = g.call_off ? g.call_off[k] : 0, hi = g.call_off ? g.call_off[k + 1] : g.n;
        oasim_call(c, g.ops + lo, (int)(hi - lo));
        g.paths.push_back(g.res.path);
        if (g.status != KAI_OK) break;
    }
    g.p_status.assign(c.p_status, c.p_status + c.P); g.p_node.assign(c.p_node, c.p_node + c.P);
    g.n_idle.assign(c.n_idle, c.n_idle + (size_t)c.R * c.N); g.n_rel.assign(c.n_rel, c.n_rel + (size_t)c.R * c.N); g.n_used.assign(c.n_used, c.n_used + (size_t)c.R * c.N);
    g.shares.assign(c.q_share, c.q_share + (size_t)c.Q * 3);
    // what no read-back shows, as one comparable record per pod / pod-set / job
    g.hidden.clear();
    for (int p = 0; p < c.P; p++) { g.hidden.push_back(c.p_on_node[p]); g.hidden.push_back(c.p_on_node[p] >= 0 ? c.p_on_node_status[p] : 0); g.hidden.push_back(c.p_accepted[p]); g.hidden.push_back(c.p_virtual[p]); }
    for (int s = 0; s < c.S; s++) { g.hidden.push_back(c.s_active_alloc[s]); g.hidden.push_back(c.s_active_used[s]); g.hidden.push_back(c.s_alive[s]); g.hidden.push_back(c.s_pipelined[s]); }
    for (int j = 0; j < c.J; j++) { g.hidden.push_back(c.j_n_pending[j]); g.hidden.push_back(c.j_tta_valid[j]); for (int k = 0; k < 3; k++) { int64_t b; std::memcpy(&b, &c.j_allocated[(size_t)j * 4 + k], 8); g.hidden.push_back((int32_t)b); g.hidden.push_back((int32_t)(b >> 32)); } }
}

}  // namespace

static uint8_t oasim_job_init_state(const kai::KaiCtx& c, int j) {
    if (j == 0 && g_oa.on && g_oa.seen++ == g_oa.at) oasim_apply(const_cast<kai::KaiCtx&>(c));  // (the context is kai_hostsim_run's own, non-const object)
    return job_init_state(c, j);
}

extern "C" {

// Runs the actions `pre`, applies `batch` (nodes: caller's indices) with `flags` and workgroups of `lanes` lanes, runs the actions `post`.  The batch goes in as n_calls
// calls, one after the other: call k = operations [call_off[k], call_off[k + 1]) (call_off NULL: one call); paths_out[k] = the path that took call k; a refused call ends it.
//   apply_status / result: what kai_ops_apply would return for the batch;
//   mid_*: pod states, node states and shares right behind the apply; hidden / hidden_cap / n_hidden: the state no read-back shows at that point, as int32 words
//   (per pod: p_on_node, its status, p_accepted, p_virtual; per pod-set: active_alloc, active_used, alive, pipelined; per job: n_pending, j_tta_valid, j_allocated's bits);
//   ops_out ...: the operations of ALL actions (pre and post) and the final state, as kai_hostsim_run returns them.
// With no post action the cycle is given one allocate to carry the hook; its results are dropped (the final state then is the state behind the apply).
int kai_oasim_run(const kai_config* cfg, const kai_snapshot_soa* s, const int* pre, int n_pre, const kai_op* batch, int64_t n_batch, uint32_t flags, int lanes,
                  const int64_t* call_off, int n_calls, int32_t* paths_out, const int* post, int n_post, int* apply_status, kai_apply_result* result,
                  int32_t* mid_status, int32_t* mid_node, kai_queue_share* mid_shares, kai_node_state* mid_nodes, int32_t* hidden, int64_t hidden_cap, int64_t* n_hidden,
                  kai_op* ops_out, int64_t ops_cap, int64_t* n_ops, int32_t* pod_status_out, int32_t* pod_node_out, kai_queue_share* shares_final, kai_node_state* nodes_out) {
    if (!cfg || !s || n_pre < 0 || n_post < 0 || n_batch < 0 || lanes < 1 || lanes > 4096 || s->n_jobs < 1 || n_calls < 1) return KAI_ERR_INVALID_ARG;
    // caller's node index -> engine node: the name rank itself.  HostPrep::build refuses a snapshot whose node_name_rank is not a permutation of 0 .. N-1 and sets
    // perm[rank] = index, which is what the library inverts (kai_core.hip oa_rank); checked here so that the two cannot part unnoticed
    { std::vector<char> seen_rank((size_t)std::max(s->n_nodes, 1), 0); for (int n = 0; n < s->n_nodes; n++) { const uint32_t rk = s->node_name_rank[n]; if (rk >= (uint32_t)s->n_nodes || seen_rank[rk]) return KAI_ERR_INVALID_ARG; seen_rank[rk] = 1; } }
    for (int64_t i = 0; i < n_batch; i++) if (batch[i].node < 0 || batch[i].node >= s->n_nodes || batch[i].pod < 0 || batch[i].pod >= s->n_pods || batch[i].kind < 0 || batch[i].kind > 2) return KAI_ERR_INVALID_ARG;
    std::vector<int> acts(pre, pre + n_pre); acts.insert(acts.end(), post, post + n_post);
    const bool carrier = n_post == 0;
    if (carrier) acts.push_back(KAI_ACTION_ALLOCATE);
    g_oa = OaSim{}; g_oa.on = true; g_oa.at = n_pre; g_oa.lanes = lanes; g_oa.ops = batch; g_oa.n = n_batch; g_oa.flags = flags; g_oa.rank = s->node_name_rank; g_oa.call_off = call_off; g_oa.n_calls = call_off ? n_calls : 1;
    std::vector<kai_op> all((size_t)ops_cap + 1); int64_t n_all = 0;
    const bool had_nb = std::getenv("KAI_HOSTSIM_NO_BATCH") != nullptr;
    if (carrier && !had_nb) setenv("KAI_HOSTSIM_NO_BATCH", "1", 1);  // the carrier's results are dropped: the sequential engine gets through it far sooner than the emulated batch path
    const int rc = kai_hostsim_run(cfg, s, acts.data(), (int)acts.size(), all.data(), ops_cap, &n_all, pod_status_out, pod_node_out, nullptr, shares_final, nodes_out, nullptr, nullptr);
    if (carrier && !had_nb) unsetenv("KAI_HOSTSIM_NO_BATCH");
    const OaSim g = g_oa; g_oa = OaSim{};
    if (rc) return rc;
    if (g.seen <= g.at) { std::fprintf(stderr, "ops_apply_sim: kai_hostsim_run did not pass job_init_state(c, 0) in front of action %d: the batch was never applied (host_sim.cpp changed?)\n", g.at); return KAI_ERR_STATE; }
    const int N = s->n_nodes, P = s->n_pods, Q = s->n_queues, R = s->n_res;
    if (apply_status) *apply_status = g.status;
    if (result) *result = g.res;
    if (paths_out) for (size_t k = 0; k < g.paths.size(); k++) paths_out[k] = g.paths[k];
    auto put_shares = [&](kai_queue_share* out) { for (int q = 0; q < Q; q++) for (int k = 0; k < 3; k++) { const QShare& x = g.shares[(size_t)q * 3 + k];
        out[q].fair_share[k] = x.fair; out[q].allocated[k] = x.allocated; out[q].allocated_non_preemptible[k] = x.allocated_np; out[q].request[k] = x.request; out[q].deserved[k] = x.deserved; out[q].max_allowed[k] = x.max_allowed; } };
    auto put_nodes = [&](kai_node_state* out) { for (int n = 0; n < N; n++) { kai_node_state o; std::memset(&o, 0, sizeof o); const int e = (int)s->node_name_rank[n];
        for (int r = 0; r < R; r++) { o.idle[r] = g.n_idle[(size_t)r * N + e]; o.releasing[r] = g.n_rel[(size_t)r * N + e]; o.used[r] = g.n_used[(size_t)r * N + e]; } out[n] = o; } };
    std::vector<int32_t> caller_of((size_t)std::max(N, 1)); for (int n = 0; n < N; n++) caller_of[s->node_name_rank[n]] = n;
    if (mid_status) std::memcpy(mid_status, g.p_status.data(), (size_t)P * 4);
    if (mid_node) for (int p = 0; p < P; p++) mid_node[p] = g.p_node[p] >= 0 ? caller_of[g.p_node[p]] : -1;
    if (mid_shares) put_shares(mid_shares);
    if (mid_nodes) put_nodes(mid_nodes);
    if (n_hidden) *n_hidden = (int64_t)g.hidden.size();
    if (hidden) { if ((int64_t)g.hidden.size() > hidden_cap) return KAI_ERR_CAPACITY; std::memcpy(hidden, g.hidden.data(), g.hidden.size() * 4); }
    if (carrier) {  // drop the carrier action: the final state is the one behind the apply, its operations are not the caller's
        if (pod_status_out) std::memcpy(pod_status_out, g.p_status.data(), (size_t)P * 4);
        if (pod_node_out) for (int p = 0; p < P; p++) pod_node_out[p] = g.p_node[p] >= 0 ? caller_of[g.p_node[p]] : -1;
        if (shares_final) put_shares(shares_final);
        if (nodes_out) put_nodes(nodes_out);
    }
    if (carrier) n_all = g.n_ops_before;  // (the carrier's operations are the tail behind the pre-actions')
    if (n_ops) *n_ops = n_all;
    if (ops_out) std::memcpy(ops_out, all.data(), (size_t)n_all * sizeof(kai_op));
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
