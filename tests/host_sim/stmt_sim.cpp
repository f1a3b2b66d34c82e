// stmt_sim.cpp — TEST INFRASTRUCTURE: the kai_stmt_* kernel bodies and control flow (kai-scheduler_amd/csrc/kai_stmt.hpp) compiled with plain g++ and run with the emulated
// lanes of kai_simt.hpp on a session of the host simulation (sim_session.hpp).  tests/test_stmt.py runs scripts of calls — begin, apply, rollback, discard, commit, actions,
// kai_ops_apply for the twins, kai_job_order and kai_subset_nodes while the Statement is open — and compares the state behind every call with the oracle's Statement and with
// twins, and the composed walk (kai_subset_nodes, kai_ordered_nodes, apply, rollback, commit).  NOT a CPU fallback: libkai_core never contains it; the parity claim is tests/test_gpu_stmt.py on the MI355X.
//
// What kai_core.hip does on the host around the kernels (the log's length, one byte per record, which path a range takes, index_stale / fast_ok) is mirrored by SimStmt below;
// the refusals in front of the first device call are host code of kai_core.hip, tested under tests/host_sim/fake_hip.cpp.
#include "sim_session.hpp"
#include "../../kai-scheduler_amd/csrc/kai_stmt.hpp"
#include "../../kai-scheduler_amd/csrc/kai_best_nodes.hpp"
#include "../../kai-scheduler_amd/csrc/kai_ordered_nodes.hpp"
// the query calls' harnesses, for their sim_job_order / sim_subset_nodes (their helpers of equal names kept apart)
#define mask_rederived jo_mask_rederived
#define same_state jo_same_state
#include "job_order_sim.cpp"
#undef mask_rederived
#undef same_state
#define mask_rederived sn_mask_rederived
#define same_state sn_same_state
#include "subset_nodes_sim.cpp"
#undef mask_rederived
#undef same_state

namespace {

struct StSimLauncher : ApplyLauncher {
    void apply(int g, int b, const KaiCtx& c, const StArgs& s) { kw::launch(g, b, 0, [&] { st_apply_body(c, s); }); }
    void undo(int g, int b, const KaiCtx& c, const StArgs& s) { kw::launch(g, b, 0, [&] { st_undo_body(c, s); }); }
    void commit(int g, int b, const KaiCtx& c, const StArgs& s) { kw::launch(g, b, 0, [&] { st_commit_body(c, s); }); }
    int engine(const KaiCtx& c, const StArgs& s) {  // as k_st_engine: one lane, no class index, the commit's operations into the call's own array
        KaiCtx cv = c; cv.use_index = 0;
        if (s.mode == KAI_ST_COMMIT) { cv.out_ops = s.out; cv.out_cap = s.out_cap; }
        HostBackend be; st_engine_walk(cv, be, s); return 0;
    }
};

// the handle's side of the Statement, as kai_core.hip keeps it
struct SimStmt {
    bool open = false; std::vector<uint8_t> rec; std::vector<int32_t> stamp; std::vector<kai_op> out; OaHead head{};
    StArgs args(SimSession& ss, int mode) {
        const KaiCtx& c = ss.ctx();
        StArgs s{}; s.a.flags = oa_wide_session(c) ? 0u : KAI_OA_NOT_WIDE; s.a.use_islot = oa_use_islot(c);
        head = OaHead{}; head.bad = KAI_OA_NONE;
        s.a.head = &head; s.a.stamp = stamp.data(); s.len = (int32_t)rec.size(); s.mode = mode; s.out = out.data(); s.out_cap = (int64_t)out.size();
        return s;
    }
    // every stamp is the number of surviving records that name the pod: what the kernels and the walk must keep
    bool stamps_right(const KaiCtx& c) const {
        std::vector<int32_t> want((size_t)c.P, 0);
        for (size_t i = 0; i < rec.size(); i++) { const int p = c.ops[i].pod; if (p < 0 || p >= c.P) return false; want[(size_t)p]++; }
        for (int p = 0; p < c.P; p++) if (stamp[(size_t)p] != want[(size_t)p]) return false;
        return true;
    }
};

int sim_stmt_begin(SimSession& ss, SimStmt& st) {
    if (st.open) return KAI_ERR_STATE;
    const KaiCtx& c = ss.ctx();
    st.stamp.assign((size_t)std::max(c.P, 1), 0); st.out.assign((size_t)st_log_room(c), kai_op{}); st.rec.clear();
    c.st->ops_len = 0; c.st->n_undo = 0;
    st.open = true;
    return KAI_OK;
}
int sim_stmt_apply(SimSession& ss, SimStmt& st, ApplyScratch& sc, const kai_op* src, int n, uint32_t flags, int lanes, kai_stmt_result& res) {
    KaiCtx& c = ss.ctx();
    res.first_bad = -1; res.path = KAI_APPLY_PATH_NONE; res.log_len = (int64_t)st.rec.size(); res.pad = 0;
    if (!st.open) return KAI_ERR_STATE;
    if (!n) return KAI_OK;
    if ((int64_t)st.rec.size() + n > st_log_room(c)) return KAI_ERR_CAPACITY;
    sc.fit(c.P);
    std::vector<kai_op> ops(src, src + n);
    for (int i = 0; i < n; i++) ops[i].node = ss.engine_node(ops[i].node);
    StArgs s = st.args(ss, KAI_ST_APPLY);
    s.a.n = n; s.a.flags |= flags; s.a.ops = ops.data(); s.a.sh_status = sc.sh_status.data(); s.a.sh_node = sc.sh_node.data();
    StSimLauncher l; OaHead hv{}; int path = 0;
    int status = st_apply_drive(l, c, s, lanes, hv, path);
    if (status == KAI_ERR_STATE) res.first_bad = hv.bad;
    if (status == KAI_OK && !(flags & KAI_APPLY_CHECK_ONLY)) {
        for (int i = 0; i < n; i++) st.rec.push_back((uint8_t)(ops[i].kind | (path == KAI_APPLY_PATH_WIDE ? 4 : 0)));
        ss.index_stale = true;
    }
    if (status == KAI_OK) { res.path = path; res.log_len = (int64_t)st.rec.size(); }
    for (int p = 0; p < c.P; p++) if (sc.sh_status[(size_t)p]) status = KAI_ERR_DEVICE_FAULT;  // the shadow must be clean again
    if (!st.stamps_right(c) || c.st->ops_len != (int)st.rec.size() || c.st->n_undo != 0) status = KAI_ERR_DEVICE_FAULT;
    return status;
}
int sim_stmt_rollback(SimSession& ss, SimStmt& st, int64_t cp, uint32_t flags, bool close, int lanes, kai_stmt_result& res) {
    KaiCtx& c = ss.ctx();
    res.first_bad = -1; res.path = KAI_APPLY_PATH_NONE; res.log_len = (int64_t)st.rec.size(); res.pad = 0;
    if (!st.open) return KAI_ERR_STATE;
    const int64_t len = (int64_t)st.rec.size();
    if (cp < 0 || cp > len) return KAI_ERR_INVALID_ARG;
    if (cp == len) { if (close) st.open = false; return KAI_OK; }
    bool wide = !(flags & KAI_APPLY_ENGINE_PATH) && oa_wide_session(c);
    for (int64_t i = cp; i < len && wide; i++) wide = (st.rec[(size_t)i] & 4) != 0;
    StArgs s = st.args(ss, close ? KAI_ST_DISCARD : KAI_ST_ROLLBACK); s.cp = (int32_t)cp;
    StSimLauncher l; OaHead hv{}; int path = 0;
    int status = st_range_drive(l, c, s, lanes, wide, hv, path);
    if (status) { st.open = false; return status; }
    st.rec.resize((size_t)cp); ss.index_stale = true;
    if (close) st.open = false;
    res.path = path; res.log_len = cp;
    if (!st.stamps_right(c) || c.st->ops_len != (int)cp || c.st->n_undo != 0) status = KAI_ERR_DEVICE_FAULT;
    return status;
}
int sim_stmt_commit(SimSession& ss, SimStmt& st, int lanes, kai_op* ops_out, int64_t cap, int64_t* n_out, kai_stmt_result& res) {
    KaiCtx& c = ss.ctx();
    res.first_bad = -1; res.path = KAI_APPLY_PATH_NONE; res.log_len = (int64_t)st.rec.size(); res.pad = 0;
    if (!st.open) return KAI_ERR_STATE;
    const int64_t len = (int64_t)st.rec.size();
    if (n_out) *n_out = len;
    if (ops_out && cap < len) return KAI_ERR_CAPACITY;
    if (!len) { st.open = false; return KAI_OK; }
    bool wide = oa_wide_session(c), non_alloc = false;
    for (uint8_t r : st.rec) { if (!(r & 4)) wide = false; if ((r & 3) != KAI_OP_ALLOCATE) non_alloc = true; }
    StArgs s = st.args(ss, KAI_ST_COMMIT);
    StSimLauncher l; OaHead hv{}; int path = 0;
    int status = st_range_drive(l, c, s, lanes, wide, hv, path);
    st.open = false;
    if (status) return status;
    if (ops_out) for (int64_t i = 0; i < len; i++) { ops_out[i] = st.out[(size_t)i]; ops_out[i].node = ss.caller_node(ops_out[i].node); }
    st.rec.clear(); ss.state_written(non_alloc);
    res.path = path; res.log_len = 0;
    if (!st.stamps_right(c) || c.st->ops_len != 0 || c.st->n_undo != 0) status = KAI_ERR_DEVICE_FAULT;
    return status;
}

// kai_best_nodes (k = 0) / kai_ordered_nodes (k >= 1) on the session's context from the first launch on, as kai_core.hip launches them: k_bn_prep, k_bn_range where a
// bin-pack strategy needs the range, k_bn_scan / k_on_scan.  rows_in: S node sets in the caller's node indices.  out: [M] or [M][k], n_out: [M] (k = 0: untouched).
// k_on_scan's workgroup is whole wavefronts (at most 256 lanes): a `lanes` that is not takes 256 there.
void sim_node_queries(SimSession& ss, const std::vector<kai_node_query>& qs, const uint32_t* rows_in, int S, int k, int lanes, std::vector<kai_node_answer>& out, std::vector<int32_t>& n_out) {
    const KaiCtx& c = ss.ctx();
    const int M = (int)qs.size(), W = (c.N + 31) / 32;
    out.assign((size_t)M * std::max(k, 1) + 1, kai_node_answer{-7, -7}); n_out.assign((size_t)M + 1, -7);
    if (!M) return;
    std::vector<uint32_t> rows((size_t)S * W + 1, 0u); std::vector<int32_t> need((size_t)2 * (S + 1), 0); std::vector<double> range((size_t)4 * (S + 1), 0.0);
    std::vector<BnQuery> prep((size_t)M + 1); std::vector<kai_node_answer> one((size_t)M + 1);
    BnArgs a; std::memset((void*)&a, 0, sizeof a);
    a.M = M; a.S = S; a.W = W; a.queries = qs.data(); a.rows_in = rows_in; a.perm = ss.prep.perm.data();
    a.rows = rows.data(); a.need = need.data(); a.range = range.data(); a.prep = prep.data(); a.out = k ? one.data() : out.data();
    const size_t items = std::max<size_t>((size_t)M, (size_t)S * W);
    kw::launch((int)((items + lanes - 1) / lanes), lanes, 0, [&] { bn_prep_body(c, a); });
    if ((c.plugins & KAI_PLUGIN_NODEPLACEMENT) && (c.gpu_strategy == KAI_BINPACK || c.cpu_strategy == KAI_BINPACK)) kw::launch(2 * (S + 1), lanes, 0, [&] { bn_range_body(c, a); });
    if (!k) { kw::launch(std::min(M, 64), lanes, 0, [&] { bn_scan_body(c, a); }); return; }
    OnArgs o; std::memset((void*)&o, 0, sizeof o); o.k = k; o.out = out.data(); o.n_out = n_out.data();
    const int on_lanes = (lanes % 64 == 0 && lanes <= 64 * KAI_ON_MAX_WAVES) ? lanes : 64 * KAI_ON_MAX_WAVES;
    kw::launch(std::min(M, 64), on_lanes, 0, [&] { on_scan_body(c, a, o); });
}

// The composed walk for one job, as a caller of the C ABI makes it: begin; kai_subset_nodes for the job's root group with the sets' bitmaps; per set a
// checkpoint, per Pending task of the job (pod order) kai_ordered_nodes(k = 1) inside the set and kai_stmt_apply of the answer; a task without a node rolls the set back to
// its checkpoint and the next set is tried; commit when a set took the gang, discard when none did.  flags: KAI_APPLY_ENGINE_PATH for apply / rollback / discard.
// q: [placed, sets tried, per tried set the operations it had applied when it ended], then the committed operations (kind, pod, node, job, stmt, seq).
int sim_walk(SimSession& ss, SimStmt& st, ApplyScratch& sc, SnScratch& sn, int job, uint32_t flags, int lanes, std::vector<int32_t>& q, kai_stmt_result& res) {
    const KaiCtx& c = ss.ctx();
    const int W = (c.N + 31) / 32;
    if (int rc = sim_stmt_begin(ss, st)) return rc;
    kai_subset_query sq; sq.job = job; sq.group = -1; sq.podset = -1; sq.nodeset = -1;
    kai_subset_answer ans{}; kai_subset_result sr{}; int64_t total = 0, cap = 64;
    std::vector<kai_node_set> sets; std::vector<uint32_t> maps; int status = KAI_OK;
    for (int t = 0; t < 2; t++) {
        sets.assign((size_t)cap, kai_node_set{}); maps.assign((size_t)cap * W + 1, 0u);
        status = sim_subset_nodes(ss, sn, 0, lanes, 64, &sq, 1, nullptr, 0, &ans, sets.data(), cap, &total, maps.data(), sr);
        if (status != KAI_ERR_CAPACITY) break;
        cap = total;
    }
    if (status) return status;
    std::vector<int> tasks;
    for (int i = 0; i < c.j_n_pods[job]; i++) { const int p = c.j_first_pod[job] + i; if (c.p_status[p] == KAI_POD_PENDING) tasks.push_back(p); }
    bool placed = false; std::vector<int32_t> tried;
    for (int s = ans.first; s < ans.first + ans.n_sets && !placed; s++) {
        const int64_t cp = (int64_t)st.rec.size();  // kai_stmt_checkpoint
        placed = !tasks.empty();
        for (int p : tasks) {
            std::vector<kai_node_query> nq(1); nq[0].pod = p; nq[0].nodeset = 0; nq[0].flags = 0; nq[0].pad = 0;
            std::vector<kai_node_answer> out; std::vector<int32_t> n_out;
            sim_node_queries(ss, nq, maps.data() + (size_t)s * W, 1, 1, lanes, out, n_out);
            if (n_out[0] < 1) { placed = false; break; }
            kai_op o; std::memset(&o, 0, sizeof o); o.kind = out[0].is_pipeline ? KAI_OP_PIPELINE : KAI_OP_ALLOCATE; o.pod = p; o.node = out[0].node; o.job = -1;
            if (int rc = sim_stmt_apply(ss, st, sc, &o, 1, flags & KAI_APPLY_ENGINE_PATH, lanes, res)) return rc;
        }
        tried.push_back((int32_t)((int64_t)st.rec.size() - cp));
        if (!placed) if (int rc = sim_stmt_rollback(ss, st, cp, flags & KAI_APPLY_ENGINE_PATH, false, lanes, res)) return rc;
    }
    q.push_back(placed ? 1 : 0); q.push_back((int32_t)tried.size()); q.insert(q.end(), tried.begin(), tried.end());
    if (!placed) return sim_stmt_rollback(ss, st, 0, flags & KAI_APPLY_ENGINE_PATH, true, lanes, res);
    std::vector<kai_op> out((size_t)st.rec.size() + 1); int64_t n = 0;
    status = sim_stmt_commit(ss, st, lanes, out.data(), (int64_t)out.size(), &n, res);
    if (status == KAI_OK) for (int64_t i = 0; i < n; i++) { const kai_op& o = out[(size_t)i]; q.insert(q.end(), {o.kind, o.pod, o.node, o.job, o.stmt, (int32_t)o.seq}); }
    return status;
}

}  // namespace

extern "C" {

// one call of a script.  kind: 0 begin; 1 apply batch[lo, hi) with `flags`; 2 rollback to cp = lo with `flags`; 3 discard with `flags`; 4 commit; 5 the action lo;
// 6 kai_ops_apply of batch[lo, hi) with `flags` (the twins); 7 kai_job_order with `flags` (depth -1); 8 kai_subset_nodes with `flags` for the root groups of jobs[lo, hi);
// 9 kai_best_nodes and 10 kai_ordered_nodes (k = lo) over ALL Pending pods, all nodes; 11 the composed walk (sim_walk) for the job lo with `flags`
struct kai_stsim_call { int32_t kind; uint32_t flags; int64_t lo, hi; };
// what a call returned: status / first_bad / path / log_len as the entry point would; n_hidden, n_q: words of this call's rows of `hidden` and `q_out`
struct kai_stsim_ret { int32_t status, path; int64_t first_bad, log_len, n_hidden, n_q; };

// Opens the session (batch: allocate actions may take the batch path) and makes the calls one after the other, in workgroups of `lanes` lanes.  Behind EVERY call, row k of:
//   pod_status / pod_node [n_calls][P], shares [n_calls][Q], nodes [n_calls][N]: the three read-backs;
//   hidden [n_calls][hidden_stride]: the state no read-back shows (sim_session.hpp StateCopy), then fast_ok, index_stale, whether a Statement is open, EngineState's ops_len
//     and n_undo, non_allocate_commits, and the log's records (10 words each);
//   q_out [n_calls][q_stride]: kind 4: the committed operations (kind, pod, node, job, stmt, seq per operation); kind 7: the order; kind 8: per query status, n_sets, tasks,
//     common_domain, then per set domain, level, allocatable_pods, n_nodes; kind 9: per Pending pod the pod, node, is_pipeline; kind 10: per Pending pod the pod, the
//     list's length, then k x (node, is_pipeline); kind 11: sim_walk's.
// A call the handle refuses (an action while a Statement is open ...) is reported in its row and the script goes on.  ops_out ...: the operations of all actions, the action
// statistics at the end.
int kai_stsim_run(const kai_config* cfg, const kai_snapshot_soa* s, int batch, const kai_op* ops, int64_t n_ops, const int32_t* jobs, int64_t n_jobs, const kai_stsim_call* calls, int n_calls,
                  int lanes, kai_stsim_ret* ret, int32_t* pod_status, int32_t* pod_node, kai_queue_share* shares, kai_node_state* nodes, int32_t* hidden, int64_t hidden_stride,
                  int32_t* q_out, int64_t q_stride, kai_op* ops_out, int64_t ops_cap, int64_t* n_ops_out, kai_action_stats* stats) {
    if (!cfg || !s || !calls || n_calls < 1 || lanes < 1 || lanes > 4096 || n_ops < 0 || n_jobs < 0 || !ret) return KAI_ERR_INVALID_ARG;
    for (int64_t i = 0; i < n_ops; i++) if (ops[i].node < 0 || ops[i].node >= s->n_nodes || ops[i].pod < 0 || ops[i].pod >= s->n_pods || ops[i].kind < 0 || ops[i].kind > 2) return KAI_ERR_INVALID_ARG;
    int n_actions = 0;
    for (int k = 0; k < n_calls; k++) {
        const kai_stsim_call& cl = calls[k];
        if (cl.kind < 0 || cl.kind > 11) return KAI_ERR_INVALID_ARG;
        if (cl.kind == 10 && (cl.lo < 1 || cl.lo > KAI_ORDERED_MAX_K)) return KAI_ERR_INVALID_ARG;
        if (cl.kind == 11 && (cl.lo < 0 || cl.lo >= s->n_jobs)) return KAI_ERR_INVALID_ARG;
        if ((cl.kind == 1 || cl.kind == 6) && (cl.lo < 0 || cl.hi < cl.lo || cl.hi > n_ops)) return KAI_ERR_INVALID_ARG;
        if (cl.kind == 8 && (cl.lo < 0 || cl.hi < cl.lo || cl.hi > n_jobs)) return KAI_ERR_INVALID_ARG;
        if (cl.kind == 5) n_actions++;
    }
    SimSession ss;
    if (int rc = ss.open(cfg, s, n_actions, batch != 0)) return rc;
    const KaiCtx& c = ss.ctx();
    const int P = c.P, Q = c.Q, N = c.N;
    SimStmt st; static ApplyScratch scratch; static JoScratch jo_scratch; SnScratch sn_scratch;
    for (int k = 0; k < n_calls; k++) {
        const kai_stsim_call& cl = calls[k];
        kai_stmt_result res{}; res.first_bad = -1; res.log_len = st.open ? (int64_t)st.rec.size() : 0;
        int status = KAI_OK; std::vector<int32_t> q;
        if (cl.kind == 0) status = sim_stmt_begin(ss, st);
        else if (cl.kind == 1) status = sim_stmt_apply(ss, st, scratch, ops + cl.lo, (int)(cl.hi - cl.lo), cl.flags, lanes, res);
        else if (cl.kind == 2) status = sim_stmt_rollback(ss, st, cl.lo, cl.flags, false, lanes, res);
        else if (cl.kind == 3) status = sim_stmt_rollback(ss, st, 0, cl.flags, true, lanes, res);
        else if (cl.kind == 4) {
            std::vector<kai_op> out((size_t)st.rec.size() + 1); int64_t n = 0;
            status = sim_stmt_commit(ss, st, lanes, out.data(), (int64_t)out.size(), &n, res);
            if (status == KAI_OK) for (int64_t i = 0; i < n; i++) { const kai_op& o = out[(size_t)i]; q.insert(q.end(), {o.kind, o.pod, o.node, o.job, o.stmt, (int32_t)o.seq}); }
        } else if (cl.kind == 5) { if (st.open) status = KAI_ERR_STATE; else if (int rc = ss.action((int)cl.lo)) return rc; }
        else if (cl.kind == 6) {
            kai_apply_result ar{};
            if (st.open) status = KAI_ERR_STATE; else status = sim_ops_apply(ss, scratch, ops + cl.lo, (int)(cl.hi - cl.lo), cl.flags, lanes, ar);
            res.first_bad = ar.first_bad; res.path = ar.path;
        } else if (cl.kind == 7) {
            std::vector<int32_t> order((size_t)std::max(c.J, 1)); int32_t n = 0; kai_job_order_result jr{};
            status = sim_job_order(ss, jo_scratch, -1, cl.flags, lanes, c.J, order.data(), &n, nullptr, nullptr, jr);
            if (status == KAI_OK) { q.assign(order.begin(), order.begin() + n); res.path = jr.path; }
        } else if (cl.kind == 9 || cl.kind == 10) {
            const int k = cl.kind == 10 ? (int)cl.lo : 0;
            std::vector<kai_node_query> nq;
            for (int p = 0; p < P; p++) if (c.p_status[p] == KAI_POD_PENDING) { kai_node_query x; x.pod = p; x.nodeset = -1; x.flags = 0; x.pad = 0; nq.push_back(x); }
            std::vector<kai_node_answer> out; std::vector<int32_t> n_out;
            sim_node_queries(ss, nq, nullptr, 0, k, lanes, out, n_out);
            for (size_t i = 0; i < nq.size(); i++) {
                q.push_back(nq[i].pod);
                if (!k) { q.push_back(out[i].node); q.push_back(out[i].is_pipeline); continue; }
                q.push_back(n_out[i]);
                for (int e = 0; e < k; e++) { q.push_back(out[i * k + e].node); q.push_back(out[i * k + e].is_pipeline); }
            }
        } else if (cl.kind == 11) {
            if (st.open) status = KAI_ERR_STATE; else status = sim_walk(ss, st, scratch, sn_scratch, (int)cl.lo, cl.flags, lanes, q, res);
        } else {
            const int M = (int)(cl.hi - cl.lo);
            std::vector<kai_subset_query> qs((size_t)std::max(M, 1)); std::vector<kai_subset_answer> ans((size_t)std::max(M, 1));
            for (int i = 0; i < M; i++) { qs[(size_t)i].job = jobs[cl.lo + i]; qs[(size_t)i].group = -1; qs[(size_t)i].podset = -1; qs[(size_t)i].nodeset = -1; }
            int64_t cap = 64 + 8 * (int64_t)M, total = 0; kai_subset_result sr{}; std::vector<kai_node_set> sets;
            for (int t = 0; t < 2; t++) {
                sets.assign((size_t)cap, kai_node_set{});
                status = sim_subset_nodes(ss, sn_scratch, cl.flags, lanes, 64, qs.data(), M, nullptr, 0, ans.data(), sets.data(), cap, &total, nullptr, sr);
                if (status != KAI_ERR_CAPACITY) break;
                cap = total;
            }
            if (status == KAI_OK) {
                for (int i = 0; i < M; i++) q.insert(q.end(), {ans[(size_t)i].status, ans[(size_t)i].n_sets, ans[(size_t)i].tasks, ans[(size_t)i].common_domain});
                for (int64_t i = 0; i < total; i++) q.insert(q.end(), {sets[(size_t)i].domain, sets[(size_t)i].level, sets[(size_t)i].allocatable_pods, sets[(size_t)i].n_nodes});
                res.path = sr.path;
            }
        }
        if (c.st->fault) return KAI_ERR_DEVICE_FAULT;
        // ---- the state behind the call
        StateCopy g = ss.snapshot_state();
        g.hidden.push_back(c.fast_ok); g.hidden.push_back(ss.index_stale ? 1 : 0); g.hidden.push_back(st.open ? 1 : 0);
        g.hidden.push_back(st.open ? c.st->ops_len : 0); g.hidden.push_back(st.open ? c.st->n_undo : 0); g.hidden.push_back((int32_t)c.st->non_allocate_commits);
        if (st.open) for (int i = 0; i < c.st->ops_len; i++) { int32_t w[10]; std::memcpy(w, &c.ops[i], sizeof w); g.hidden.insert(g.hidden.end(), w, w + 10); }
        static_assert(sizeof(StmtOp) == 40, "a log record is ten words");
        if ((int64_t)g.hidden.size() > hidden_stride || (int64_t)q.size() > q_stride) return KAI_ERR_CAPACITY;
        kai_stsim_ret& r = ret[k];
        r.status = status; r.path = res.path; r.first_bad = res.first_bad; r.log_len = st.open ? (int64_t)st.rec.size() : 0; r.n_hidden = (int64_t)g.hidden.size(); r.n_q = (int64_t)q.size();
        if (int rc = ss.write(g, pod_status + (size_t)k * P, pod_node + (size_t)k * P, shares + (size_t)k * Q, nodes + (size_t)k * N, hidden + (size_t)k * hidden_stride, hidden_stride, nullptr)) return rc;
        if (!q.empty()) std::memcpy(q_out + (size_t)k * q_stride, q.data(), q.size() * 4);
    }
    if (int rc = ss.finish()) return rc;
    if (int rc = ss.ops(ops_out, ops_cap, n_ops_out)) return rc;
    ss.stats(stats);
    return KAI_OK;
}

}  // extern "C"
