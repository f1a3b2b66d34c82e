// stale_gangs_sim.cpp — TEST INFRASTRUCTURE: kai_stale_gang_eviction's kernel bodies and control flow (kai-scheduler_amd/csrc/kai_stale_gangs.hpp: sg_drive, and through it the
// library's own oa_drive) compiled with plain g++ and run with the emulated lanes of kai_simt.hpp on a session set up exactly as the host simulation sets one up: this file
// INCLUDES host_sim.cpp, as ops_apply_sim.cpp does.  tests/test_stale_gangs.py compares the decision with a numpy restatement of the reference's rules and the state with a TWIN
// session that takes the same operations through kai_ops_apply's emulated apply (mode 1 below).  NOT a CPU fallback: libkai_core never contains it; the parity claim is
// tests/test_gpu_stale_gangs.py on the MI355X.
//
// The call gets into kai_hostsim_run's cycle the way ops_apply_sim.cpp's batch does: job_init_state(c, 0) is the first thing every action calls; the name is routed through
// sgsim_job_init_state for the text of host_sim.cpp only, and in front of action number `at` the hook runs the call.
//
// -DKAI_SGSIM_MAIN adds a main() with one fixed case (the stand-alone program the sanitizers are run on).
#define KAI_SHARED_GPUS 1
#include <cstdlib>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>
namespace kai { extern int sgsim_dom_lanes_min; }
#define KAI_DOM_LANES_MIN ::kai::sgsim_dom_lanes_min
#include "../../kai-scheduler_amd/csrc/kai_host_prep.hpp"
#include "../../kai-scheduler_amd/csrc/kai_batch_kernels.hpp"
#include "../../kai-scheduler_amd/csrc/kai_batch_driver.hpp"
#include "../../kai-scheduler_amd/csrc/kai_victim_shard.hpp"
#include "../../kai-scheduler_amd/csrc/kai_stale_gangs.hpp"
#undef KAI_DOM_LANES_MIN
namespace kai { int sgsim_dom_lanes_min = 16; }

static uint8_t sgsim_job_init_state(const kai::KaiCtx& c, int j);
#define job_init_state(c, j) sgsim_job_init_state(c, j)
#include "host_sim.cpp"
#undef job_init_state

namespace {

struct SgSim {
    bool on = false; int at = 0, seen = 0, lanes = 256, mode = 0;
    int64_t* since = nullptr; uint8_t* stale = nullptr; int64_t grace_ns = 0; uint32_t flags = 0; int64_t call_cap = 0;  // mode 0: the call's arguments
    kai_op* ops = nullptr; int64_t n = 0; const uint32_t* rank = nullptr;  // mode 0: the evictions out (caller's node indices); mode 1: the batch in.  node index -> name rank
    int status = 0; kai_stale_result res{}; int64_t n_ops_before = 0;
    std::vector<int32_t> p_status, p_node, hidden; std::vector<double> n_idle, n_rel, n_used; std::vector<QShare> shares;  // the state right behind the call
} g_sg;

// the handle's scratch of both entry points: zero between calls
struct Scratch { std::vector<int32_t> stamp, sh_status, sh_node, succ, first, wg_e, wg_f; std::vector<int64_t> since; std::vector<uint8_t> expired; std::vector<kai_op> ops; OaHead oa_head{}; SgHead head{}; };
Scratch& scratch(const KaiCtx& c) {
    static Scratch s;
    if ((int)s.stamp.size() < c.P) { s.stamp.assign((size_t)c.P, 0); s.sh_status.assign((size_t)c.P, 0); s.sh_node.assign((size_t)c.P, 0); }
    if ((int)s.succ.size() < c.J) s.succ.assign((size_t)c.J, 0);
    return s;
}

struct SimLauncher {
    Scratch& s;
    void check(int g, int b, const KaiCtx& c, const OaArgs& a) { kw::launch(g, b, 0, [&] { oa_check_body(c, a); }); }
    void wide(int g, int b, const KaiCtx& c, const OaArgs& a) { kw::launch(g, b, 0, [&] { oa_wide_body(c, a); }); }
    int engine(const KaiCtx& c, const OaArgs& a) { KaiCtx cv = c; cv.use_index = 0; HostBackend be; oa_engine_walk(cv, be, a); return 0; }  // as k_oa_engine: one lane, no class index
    int read_head(OaHead& hv, const OaArgs& a) { hv = *a.head; return 0; }
    void succeeded(int g, int b, const KaiCtx& c, const SgArgs& a) { kw::launch(g, b, 0, [&] { sg_succeeded_body(c, a); }); }
    void jobs(int g, int b, const KaiCtx& c, const SgArgs& a) { kw::launch(g, b, 0, [&] { sg_jobs_body(c, a); }); }
    void first(int g, int b, const KaiCtx& c, const SgArgs& a) { kw::launch(g, b, 0, [&] { sg_first_body(c, a); }); }
    void totals(int g, int b, const KaiCtx& c, const SgArgs& a) { kw::launch(g, b, 0, [&] { sg_totals_body(c, a); }); }
    void scan(int b, const SgArgs& a) { kw::launch(1, b, 0, [&] { sg_scan_body(a); }); }
    void emit(int g, int b, const KaiCtx& c, const SgArgs& a) { kw::launch(g, b, 0, [&] { sg_emit_body(c, a); }); }
    int read_counts(SgHead& hd, const SgArgs& a) { hd = *a.head; return 0; }
    int reserve_ops(int n, SgArgs& a, OaArgs& oa) {
        s.ops.assign((size_t)n, kai_op{}); std::memset(&s.oa_head, 0xff, sizeof s.oa_head);  // (k_sg_emit writes the verdict's start values itself)
        a.oa_head = &s.oa_head; a.ops = s.ops.data();
        oa.ops = s.ops.data(); oa.head = &s.oa_head; oa.stamp = s.stamp.data(); oa.sh_status = s.sh_status.data(); oa.sh_node = s.sh_node.data();
        return 0;
    }
};

bool scratch_clean(const KaiCtx& c, const Scratch& s) {
    for (int p = 0; p < c.P; p++) if (s.stamp[p] || s.sh_status[p]) return false;
    for (int j = 0; j < c.J; j++) if (s.succ[j]) return false;
    return true;
}
void after_apply(KaiCtx& c) {  // the host side behind the kernels (kai_core.hip): index_stale, fast_ok
    if (c.use_index) for (int b = 0; b < c.NB; b++) for (int k = 0; k < c.C; k++) HostBackend::build_block(c, k, b);
    c.fast_ok = 0;
}

// kai_stale_gang_eviction from its first device call on (the refusals in front of it are host code of kai_core.hip, tested under tests/host_sim/fake_hip.cpp)
void sgsim_call(KaiCtx& c) {
    SgSim& g = g_sg; Scratch& s = scratch(c);
    const int lanes = g.lanes, n_wgs = (int)(((int64_t)c.P + lanes - 1) / lanes);
    s.since.assign(g.since, g.since + c.J); s.expired.assign((size_t)c.J, 0xee); s.first.assign((size_t)c.J, -7); s.wg_e.assign((size_t)n_wgs + 1, -7); s.wg_f.assign((size_t)n_wgs + 1, -7);
    s.head = SgHead{};
    SgArgs a{}; a.now_ns = c.now_ns; a.grace_ns = g.grace_ns; a.n_wgs = n_wgs;
    a.head = &s.head; a.since = s.since.data(); a.expired = s.expired.data(); a.succ = s.succ.data(); a.first = s.first.data(); a.wg_e = s.wg_e.data(); a.wg_f = s.wg_f.data();
    SimLauncher l{s}; SgHead hd{}; OaHead hv{}; int path = 0;
    const bool dry = (g.flags & KAI_STALE_DRY_RUN) != 0;
    g.status = sg_drive(l, c, a, lanes, dry, g.call_cap, hd, hv, path);
    if (!scratch_clean(c, s)) g.status = KAI_ERR_DEVICE_FAULT;
    if (g.status == KAI_ERR_CAPACITY) { g.n = hd.n_ops; return; }
    if (g.status != KAI_OK) return;
    if (hd.n_ops > 0 && !dry) after_apply(c);
    std::vector<int32_t> caller_of((size_t)std::max(c.N, 1)); for (int n = 0; n < c.N; n++) caller_of[g.rank[n]] = n;
    std::memcpy(g.since, s.since.data(), (size_t)c.J * 8);
    if (g.stale) std::memcpy(g.stale, s.expired.data(), (size_t)c.J);
    for (int i = 0; i < hd.n_ops; i++) { kai_op o = s.ops[(size_t)i]; o.node = caller_of[o.node]; g.ops[i] = o; }
    g.n = hd.n_ops;
    g.res.stale_jobs = hd.stale_jobs; g.res.expired_jobs = hd.expired_jobs; g.res.n_ops = hd.n_ops; g.res.path = path; g.res.pad = 0;
}

// mode 1, the twin: kai_ops_apply from its first device call on, as ops_apply_sim.cpp's oasim_call
void oasim_call(KaiCtx& c) {
    SgSim& g = g_sg; Scratch& s = scratch(c);
    const int n = (int)g.n;
    if (!n) return;
    std::vector<kai_op> ops(g.ops, g.ops + n);
    for (int i = 0; i < n; i++) ops[i].node = (int32_t)g.rank[ops[i].node];
    OaHead head{}; head.bad = KAI_OA_NONE;
    OaArgs a{}; a.n = n; a.flags = oa_wide_session(c) ? 0u : KAI_OA_NOT_WIDE; a.use_islot = oa_use_islot(c);
    a.ops = ops.data(); a.head = &head; a.stamp = s.stamp.data(); a.sh_status = s.sh_status.data(); a.sh_node = s.sh_node.data();
    SimLauncher l{s}; OaHead hv{}; int path = 0;
    g.status = oa_drive(l, c, a, g.lanes, hv, path);
    if (!scratch_clean(c, s)) g.status = KAI_ERR_DEVICE_FAULT;
    if (g.status == KAI_OK) { g.res.path = path; g.res.n_ops = n; after_apply(c); }
}

void sgsim_apply(KaiCtx& c) {
    SgSim& g = g_sg;
    g.n_ops_before = c.st->out_len;
    if (g.at == 0) for (int q = 0; q < c.Q; q++) qnode_init(c, q, 0);  // k_qnode_static of the open: the host simulation fills the tree in its first action only, and the event handlers walk its parents
    if (g.mode == 0) sgsim_call(c); else oasim_call(c);
    g.p_status.assign(c.p_status, c.p_status + c.P); g.p_node.assign(c.p_node, c.p_node + c.P);
    g.n_idle.assign(c.n_idle, c.n_idle + (size_t)c.R * c.N); g.n_rel.assign(c.n_rel, c.n_rel + (size_t)c.R * c.N); g.n_used.assign(c.n_used, c.n_used + (size_t)c.R * c.N);
    g.shares.assign(c.q_share, c.q_share + (size_t)c.Q * 3);
    // what no read-back shows, as one comparable record per pod / pod-set / job
    g.hidden.clear();
    for (int p = 0; p < c.P; p++) { g.hidden.push_back(c.p_on_node[p]); g.hidden.push_back(c.p_on_node[p] >= 0 ? c.p_on_node_status[p] : 0); g.hidden.push_back(c.p_accepted[p]); g.hidden.push_back(c.p_virtual[p]); }
    for (int s = 0; s < c.S; s++) { g.hidden.push_back(c.s_active_alloc[s]); g.hidden.push_back(c.s_active_used[s]); g.hidden.push_back(c.s_alive[s]); g.hidden.push_back(c.s_pipelined[s]); }
    for (int j = 0; j < c.J; j++) { g.hidden.push_back(c.j_n_pending[j]); g.hidden.push_back(c.j_tta_valid[j]); for (int k = 0; k < 3; k++) { int64_t b; std::memcpy(&b, &c.j_allocated[(size_t)j * 4 + k], 8); g.hidden.push_back((int32_t)b); g.hidden.push_back((int32_t)(b >> 32)); } }
    g.hidden.push_back(c.fast_ok);
}

}  // namespace

static uint8_t sgsim_job_init_state(const kai::KaiCtx& c, int j) {
    if (j == 0 && g_sg.on && g_sg.seen++ == g_sg.at) sgsim_apply(const_cast<kai::KaiCtx&>(c));  // (the context is kai_hostsim_run's own, non-const object)
    return job_init_state(c, j);
}

extern "C" {

// Runs the actions `pre`, then
//   mode 0: kai_stale_gang_eviction at the clock cfg->now_ns with `grace_ns`, `flags` (KAI_STALE_DRY_RUN) and a capacity of `call_cap` operations, in workgroups of `lanes` lanes:
//           since [J] in/out, stale_out [J] or NULL, sg_ops [call_cap] out, *n_sg_ops out, result out;
//   mode 1: kai_ops_apply's emulated apply of sg_ops[0 .. *n_sg_ops) (the twin);
// then the actions `post`.  call_status: what the entry point would return.  mid_* / hidden: the state right behind the call (hidden: what no read-back shows, as int32 words:
// per pod p_on_node, its status, p_accepted, p_virtual; per pod-set active_alloc, active_used, alive, pipelined; per job n_pending, j_tta_valid, j_allocated's bits; fast_ok).
// ops_out ...: the operations of ALL actions and the final state, as kai_hostsim_run returns them.  With no post action the cycle is given one allocate to carry the hook; its
// results are dropped (the final state then is the state behind the call).
int kai_sgsim_run(const kai_config* cfg, const kai_snapshot_soa* s, const int* pre, int n_pre, int mode, int64_t* since, uint8_t* stale_out, int64_t grace_ns, uint32_t flags, int lanes,
                  int64_t call_cap, kai_op* sg_ops, int64_t* n_sg_ops, kai_stale_result* result, int* call_status, const int* post, int n_post,
                  int32_t* mid_status, int32_t* mid_node, kai_queue_share* mid_shares, kai_node_state* mid_nodes, int32_t* hidden, int64_t hidden_cap, int64_t* n_hidden,
                  kai_op* ops_out, int64_t ops_cap, int64_t* n_ops, int32_t* pod_status_out, int32_t* pod_node_out, kai_queue_share* shares_final, kai_node_state* nodes_out) {
    if (!cfg || !s || n_pre < 0 || n_post < 0 || lanes < 1 || lanes > 4096 || s->n_jobs < 1 || !n_sg_ops || (mode != 0 && mode != 1) || (mode == 0 && (!since || call_cap < 0))) return KAI_ERR_INVALID_ARG;
    { std::vector<char> seen_rank((size_t)std::max(s->n_nodes, 1), 0); for (int n = 0; n < s->n_nodes; n++) { const uint32_t rk = s->node_name_rank[n]; if (rk >= (uint32_t)s->n_nodes || seen_rank[rk]) return KAI_ERR_INVALID_ARG; seen_rank[rk] = 1; } }
    if (mode == 1) for (int64_t i = 0; i < *n_sg_ops; i++) if (sg_ops[i].node < 0 || sg_ops[i].node >= s->n_nodes || sg_ops[i].pod < 0 || sg_ops[i].pod >= s->n_pods || sg_ops[i].kind < 0 || sg_ops[i].kind > 2) return KAI_ERR_INVALID_ARG;
    std::vector<int> acts(pre, pre + n_pre); acts.insert(acts.end(), post, post + n_post);
    const bool carrier = n_post == 0;
    if (carrier) acts.push_back(KAI_ACTION_ALLOCATE);
    g_sg = SgSim{}; g_sg.on = true; g_sg.at = n_pre; g_sg.lanes = lanes; g_sg.mode = mode; g_sg.since = since; g_sg.stale = stale_out; g_sg.grace_ns = grace_ns; g_sg.flags = flags; g_sg.call_cap = call_cap;
    g_sg.ops = sg_ops; g_sg.n = mode == 1 ? *n_sg_ops : 0; g_sg.rank = s->node_name_rank;
    std::vector<kai_op> all((size_t)ops_cap + 1); int64_t n_all = 0;
    const bool had_nb = std::getenv("KAI_HOSTSIM_NO_BATCH") != nullptr;
    if (carrier && !had_nb) setenv("KAI_HOSTSIM_NO_BATCH", "1", 1);  // the carrier's results are dropped: the sequential engine gets through it far sooner than the emulated batch path
    const int rc = kai_hostsim_run(cfg, s, acts.data(), (int)acts.size(), all.data(), ops_cap, &n_all, pod_status_out, pod_node_out, nullptr, shares_final, nodes_out, nullptr, nullptr);
    if (carrier && !had_nb) unsetenv("KAI_HOSTSIM_NO_BATCH");
    const SgSim g = g_sg; g_sg = SgSim{};
    if (rc) return rc;
    if (g.seen <= g.at) { std::fprintf(stderr, "stale_gangs_sim: kai_hostsim_run did not pass job_init_state(c, 0) in front of action %d: the call was never made (host_sim.cpp changed?)\n", g.at); return KAI_ERR_STATE; }
    const int N = s->n_nodes, P = s->n_pods, Q = s->n_queues, R = s->n_res;
    if (call_status) *call_status = g.status;
    if (result) *result = g.res;
    if (mode == 0) *n_sg_ops = g.n;
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
    if (carrier) {  // drop the carrier action: the final state is the one behind the call, its operations are not the caller's
        if (pod_status_out) std::memcpy(pod_status_out, g.p_status.data(), (size_t)P * 4);
        if (pod_node_out) for (int p = 0; p < P; p++) pod_node_out[p] = g.p_node[p] >= 0 ? caller_of[g.p_node[p]] : -1;
        if (shares_final) put_shares(shares_final);
        if (nodes_out) put_nodes(nodes_out);
        n_all = g.n_ops_before;
    }
    if (n_ops) *n_ops = n_all;
    if (ops_out) std::memcpy(ops_out, all.data(), (size_t)n_all * sizeof(kai_op));
    return KAI_OK;
}

}  // extern "C"

#ifdef KAI_SGSIM_MAIN
// One fixed case: 6 nodes of 8 GPUs whose name ranks are the reverse of their indices, 3 queues, 14 jobs of 3 one-GPU pods with minAvailable 3 (job 13: two pod-sets, 2 + 1):
//   jobs 0-5 running; job 1 lost a pod to Failed (stamped long ago: evicted, two evictions); job 2 lost one (stamped just now: inside its grace); job 3 lost one (never
//   stamped: newly stale); job 4 lost one but has a Succeeded pod (not stale, its old stamp is cleared); job 5: one pod Failed, two Releasing (expired, nothing to evict);
//   jobs 6-11 pending; job 12: a Pipelined and a Running pod, one Failed (expired: the engine walk); job 13: stale through its second pod-set only.
// The call with 256, 100 and 1 lanes: the decision checked against the list above, the state against the twin that takes the same operations through the emulated kai_ops_apply,
// also through the allocate action run behind either; a dry run and a call without capacity write nothing.
int main() {
    const int N = 6, Q = 3, J = 14, PJ = 3, P = J * PJ, R = 4, S = J + 1;
    const int64_t SEC = 1000000000ll, NOW = 1000 * SEC, GRACE = 60 * SEC;
    std::vector<double> alloc((size_t)R * N), req((size_t)R * P);
    std::vector<uint32_t> nflags(N, 0u), nrank(N), pflags(P, 0u), puid(P), juid(J), quid(Q), psrank(S, 0u);
    std::vector<int32_t> ngc(N, -1), ncls(N, 0), pjob(P), pps(P), pst(P), pnode(P), pprio(P, 0), pcls(P, 0), pnom(P, -1), psjob(S), psmin(S, 3), jq(J), jprio(J, 50), jpre(J), jfp(J), jnp(J, PJ), jfps(J), jnps(J, 1), qpar = {-1, 0, 0}, qprio(Q, 0);
    std::vector<int64_t> pcreated(P), jcreated(J), qcreated(Q);
    for (int n = 0; n < N; n++) { nrank[n] = (uint32_t)(N - 1 - n); alloc[0 * N + n] = 64000; alloc[1 * N + n] = 256000; alloc[2 * N + n] = 8; alloc[3 * N + n] = 110; }
    for (int j = 0; j < J; j++) { psjob[j] = j; jq[j] = 1 + j % 2; jpre[j] = j % 3 != 0; jfp[j] = j * PJ; jfps[j] = j; juid[j] = (uint32_t)j; jcreated[j] = 1000 + j; }
    psjob[J] = 13; jnps[13] = 2; psmin[13] = 2; psmin[14] = 1; psrank[14] = 1;
    for (int p = 0; p < P; p++) {
        const int j = p / PJ; pjob[p] = j; pps[p] = j; puid[p] = (uint32_t)p; pcreated[p] = 2000 + p;
        const bool placed = j < 6 || j >= 12;
        pst[p] = placed ? KAI_POD_RUNNING : KAI_POD_PENDING; pnode[p] = placed ? p % N : -1;
        req[0 * P + p] = 1000; req[1 * P + p] = 4000; req[2 * P + p] = 1; req[3 * P + p] = 1;
    }
    auto lose = [&](int p, int st) { pst[p] = st; };
    lose(1 * PJ + 1, KAI_POD_FAILED); lose(2 * PJ + 0, KAI_POD_FAILED); lose(3 * PJ + 2, KAI_POD_FAILED); lose(4 * PJ + 0, KAI_POD_FAILED); lose(4 * PJ + 1, KAI_POD_SUCCEEDED);
    lose(5 * PJ + 0, KAI_POD_FAILED); lose(5 * PJ + 1, KAI_POD_RELEASING); lose(5 * PJ + 2, KAI_POD_RELEASING);
    lose(12 * PJ + 0, KAI_POD_PIPELINED); lose(12 * PJ + 2, KAI_POD_FAILED);
    pps[13 * PJ + 2] = 14; lose(13 * PJ + 2, KAI_POD_FAILED);
    for (int q = 0; q < Q; q++) { quid[q] = (uint32_t)q; qcreated[q] = 10 + q; }
    std::vector<double> qdes = {384000, 192000, 192000, 1536000, 768000, 768000, 48, 24, 24}, qlim(9, -1.0), qoqw(9, 1.0);
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
    cfg.now_ns = NOW;

    std::vector<int64_t> since0(J, 0);
    since0[1] = NOW - GRACE; since0[2] = NOW - GRACE + 1; since0[4] = NOW - 5 * GRACE; since0[5] = NOW - GRACE - 1; since0[12] = 1; since0[13] = NOW - GRACE;
    since0[6] = 77;  // a pending job that carries a stamp: cleared
    struct Out { int rc = 99, status = 99; kai_stale_result res{}; std::vector<int64_t> since; std::vector<uint8_t> stale; std::vector<kai_op> sg, ops; std::vector<int32_t> st, nd, hidden; std::vector<kai_queue_share> sh; std::vector<kai_node_state> ns; };
    const int ALLOC[1] = {KAI_ACTION_ALLOCATE};
    auto run = [&](int mode, const std::vector<kai_op>* batch, uint32_t flags, int lanes, int64_t cap, bool post, Out& o) {
        o.since = since0; o.stale.assign(J, 9); o.sg.assign((size_t)P, kai_op{}); int64_t n_sg = 0;
        if (batch) { o.sg = *batch; n_sg = (int64_t)batch->size(); o.sg.resize((size_t)P); }
        o.st.assign(P, 0); o.nd.assign(P, 0); o.hidden.assign((size_t)4 * P + 4 * S + 8 * J + 8, 0); o.sh.resize(Q); o.ns.resize(N); int64_t nh = 0, nops = 0;
        o.ops.assign((size_t)8 * P + 64, kai_op{});
        o.rc = kai_sgsim_run(&cfg, &s, nullptr, 0, mode, o.since.data(), o.stale.data(), GRACE, flags, lanes, cap, o.sg.data(), &n_sg, &o.res, &o.status, post ? ALLOC : nullptr, post ? 1 : 0,
                             o.st.data(), o.nd.data(), o.sh.data(), o.ns.data(), o.hidden.data(), (int64_t)o.hidden.size(), &nh, o.ops.data(), (int64_t)o.ops.size(), &nops, nullptr, nullptr, nullptr, nullptr);
        o.hidden.resize((size_t)nh); o.ops.resize((size_t)nops); o.sg.resize((size_t)n_sg);
        return o.rc;
    };
    auto same_state = [&](const Out& a, const Out& b) {
        return a.st == b.st && a.nd == b.nd && a.hidden == b.hidden && std::memcmp(a.sh.data(), b.sh.data(), sizeof(kai_queue_share) * Q) == 0 && std::memcmp(a.ns.data(), b.ns.data(), sizeof(kai_node_state) * N) == 0;
    };
    auto same_ops = [](const std::vector<kai_op>& a, const std::vector<kai_op>& b) { return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(kai_op)) == 0); };
    int bad = 0, checks = 0;
    auto expect = [&](bool ok, const char* what) { checks++; if (!ok) { bad++; std::printf("FAILED: %s\n", what); } };
    const std::vector<kai_op> none;
    Out open; expect(run(1, &none, 0, 256, 0, false, open) == 0 && open.status == 0, "the untouched session");
    std::vector<int64_t> want_since(J, 0); want_since[1] = since0[1]; want_since[2] = since0[2]; want_since[3] = NOW; want_since[5] = since0[5]; want_since[12] = 1; want_since[13] = since0[13];
    std::vector<uint8_t> want_stale(J, 0); want_stale[1] = want_stale[5] = want_stale[12] = want_stale[13] = 1;
    const int want_pod[6] = {3, 5, 36, 37, 39, 40}, want_stmt[6] = {0, 0, 1, 1, 2, 2};
    Out first; bool have = false;
    for (int lanes : {256, 100, 1}) {
        Out o; expect(run(0, nullptr, 0, lanes, P, false, o) == 0 && o.status == KAI_OK, "the call");
        expect(o.since == want_since && o.stale == want_stale, "timestamps and Stale");
        expect(o.res.stale_jobs == 6 && o.res.expired_jobs == 4 && o.res.n_ops == 6 && o.res.path == KAI_APPLY_PATH_ENGINE && o.sg.size() == 6, "the counts, and the engine walk for a Pipelined pod");
        for (size_t i = 0; i < o.sg.size() && i < 6; i++) { const kai_op& e = o.sg[i];
            expect(e.seq == (int64_t)i && e.kind == KAI_OP_EVICT && e.pod == want_pod[i] && e.node == want_pod[i] % N && e.job == want_pod[i] / PJ && e.stmt == want_stmt[i] && e.pad == 0, "an eviction"); }
        expect(o.st[3] == KAI_POD_RELEASING && o.st[4] == KAI_POD_FAILED && o.st[36] == KAI_POD_RELEASING && o.st[6] == KAI_POD_FAILED && o.st[7] == KAI_POD_RUNNING && o.ns[3].releasing[2] == open.ns[3].releasing[2] + 2, "evicted pods are Releasing on their nodes");
        Out twin; expect(run(1, &o.sg, 0, lanes, 0, false, twin) == 0 && twin.status == KAI_OK && twin.res.path == o.res.path, "the twin takes the operations");
        expect(same_state(o, twin), "the call leaves what kai_ops_apply of its operations leaves");
        if (!have) { first = o; have = true; } else expect(same_state(o, first) && same_ops(o.sg, first.sg), "every workgroup size: the same operations and state");
        Out dry; expect(run(0, nullptr, KAI_STALE_DRY_RUN, lanes, P, false, dry) == 0 && dry.status == KAI_OK && same_state(dry, open), "a dry run writes nothing");
        expect(dry.since == want_since && dry.stale == want_stale && same_ops(dry.sg, o.sg) && dry.res.path == o.res.path && dry.res.n_ops == 6, "... and reports the same");
        Out small; expect(run(0, nullptr, 0, lanes, 5, false, small) == 0 && small.status == KAI_ERR_CAPACITY && small.sg.size() == 6 && same_state(small, open) && small.since == since0, "a capacity below the evictions: the count needed, nothing written");
    }
    {   Out a, b; expect(run(0, nullptr, 0, 256, P, true, a) == 0 && a.status == KAI_OK, "allocate behind the call");
        expect(run(1, &first.sg, 0, 256, 0, true, b) == 0 && b.status == KAI_OK, "allocate behind the twin's apply");
        expect(same_ops(a.ops, b.ops) && !a.ops.empty(), "the next allocate commits the same operations"); }
    {   const int64_t keep = since0[12]; since0[12] = NOW - GRACE + 5; since0[13] = 0;  // without the Pipelined pod's job and the two-pod-set job: placed pods only
        Out o; expect(run(0, nullptr, 0, 256, P, false, o) == 0 && o.status == KAI_OK && o.res.n_ops == 2 && o.res.expired_jobs == 2 && o.res.path == KAI_APPLY_PATH_WIDE && o.since[13] == NOW && o.stale[13] == 0, "placed pods only: the chip-wide path");
        Out twin; expect(run(1, &o.sg, 0, 256, 0, false, twin) == 0 && same_state(o, twin), "... and the twin");
        since0[12] = keep; }
    for (char* st : kw::emu().stacks) std::free(st);  // the emulator keeps its fibers' stacks for the life of the process: handed back so that a leak check ends clean
    kw::emu().stacks.clear();
    std::printf(bad ? "stale_gangs_sim: %d of %d checks FAILED\n" : "stale_gangs_sim: ok (%d checks)\n", bad ? bad : checks, checks);
    return bad ? 1 : 0;
}
#endif
