// stmt_place_sim.cpp — TEST INFRASTRUCTURE: kai_stmt_place's kernel bodies (kai-scheduler_amd/csrc/kai_stmt_place.hpp) compiled with plain g++ and run with the emulated lanes
// of kai_simt.hpp on a session of the host simulation, beside the kai_stmt_* calls of stmt_sim.cpp (included as it is: its harness functions are this file's too).
// tests/test_stmt_place.py runs scripts of calls and compares kai_stmt_place with THE LOOP OVER THE EXISTING CALLS its contract names (sim_place_loop below: checkpoint,
// kai_ordered_nodes_scored with k = 1, kai_stmt_apply of one operation, kai_stmt_rollback), with the oracle and with the allocate action.  NOT a CPU fallback: libkai_core
// never contains it; the parity claim is tests/test_gpu_stmt_place.py on the MI355X.
//
// What kai_core.hip does on the host around the two kernels (the rows the sets name and their sizes, the mode, one byte per surviving record, index_stale) is mirrored by
// sim_stmt_place; the refusals in front of the first device call are host code of kai_core.hip, tested under tests/host_sim/fake_hip.cpp.
#include "stmt_sim.cpp"
#include "../../kai-scheduler_amd/csrc/kai_stmt_place.hpp"

namespace {

// the place data of a script (kai_spsim_set): every place / loop call of the script takes a range of these gangs
struct PlaceData {
    std::vector<kai_place_gang> gangs; std::vector<int32_t> tasks, sets; std::vector<uint32_t> rows; int R = 0;
    std::vector<kai_topo_score_row> score_rows; std::vector<uint8_t> deciles;
};
PlaceData g_place;

// what both a place call and the loop report: per gang status, set, sets_tried, first_op, n_ops; fail_at [S]; per surviving operation kind, pod, node, job, stmt, seq
void report(std::vector<int32_t>& q, const std::vector<kai_place_answer>& ans, const std::vector<int32_t>& fail_at, const std::vector<kai_op>& ops) {
    for (const kai_place_answer& x : ans) q.insert(q.end(), {x.status, x.set, x.sets_tried, (int32_t)x.first_op, (int32_t)x.n_ops});
    q.insert(q.end(), fail_at.begin(), fail_at.end());
    for (const kai_op& o : ops) q.insert(q.end(), {o.kind, o.pod, o.node, o.job, o.stmt, (int32_t)o.seq});
}

// kai_stmt_place from its first device call on, for the gangs [g0, g1) of the script's place data.  flags: KAI_APPLY_ENGINE_PATH | KAI_PLACE_PIPELINE_ONLY
int sim_stmt_place(SimSession& ss, SimStmt& st, const PlaceData& d, int g0, int g1, uint32_t flags, int lanes, std::vector<int32_t>& q, kai_stmt_result& res) {
    KaiCtx& c = ss.ctx();
    res.first_bad = -1; res.path = KAI_APPLY_PATH_NONE; res.log_len = (int64_t)st.rec.size(); res.pad = 0;
    if (!st.open) return KAI_ERR_STATE;
    const int G = g1 - g0, T = (int)d.tasks.size(), S = (int)d.sets.size(), R = d.R, N = c.N, W = (N + 31) / 32;
    if (G == 0) return KAI_OK;
    const int len0 = (int)st.rec.size();
    if ((int64_t)len0 + T > st_log_room(c)) return KAI_ERR_CAPACITY;
    if (lanes % 64) return KAI_ERR_INVALID_ARG;  // whole wavefronts
    // ---- the rows the sets name and their sizes
    std::vector<int32_t> row_off((size_t)R + 1, 0), size((size_t)R, 0), used; std::vector<uint8_t> seen((size_t)R, 0);
    for (int i = 0; i < S; i++) if (d.sets[i] >= 0 && !seen[(size_t)d.sets[i]]) { seen[(size_t)d.sets[i]] = 1; used.push_back(d.sets[i]); }
    const uint32_t last = (N & 31) ? ((1u << (N & 31)) - 1u) : 0xffffffffu;
    for (int r : used) for (int w = 0; w < W; w++) size[(size_t)r] += __builtin_popcount(w == W - 1 ? d.rows[(size_t)r * W + w] & last : d.rows[(size_t)r * W + w]);
    int64_t list_len = 0;
    for (int r = 0; r < R; r++) { row_off[(size_t)r] = (int32_t)list_len; list_len += size[(size_t)r]; }
    row_off[(size_t)R] = (int32_t)list_len;
    std::vector<uint32_t> packed(used.size() * (size_t)W + 1, 0u);  // only the rows the sets name, in the order of `used` (as kai_core.hip sends them)
    for (size_t i = 0; i < used.size(); i++) std::memcpy(packed.data() + i * W, d.rows.data() + (size_t)used[i] * W, (size_t)W * 4);
    std::vector<int32_t> list((size_t)list_len + 1, -1), fail_at((size_t)S + 1, -7);
    std::vector<kai_place_answer> ans((size_t)G); std::vector<kai_op> ops((size_t)T + 1);
    SpHead head{}; head.bad = KAI_OA_NONE; head.len = len0;
    SpArgs a; std::memset((void*)&a, 0, sizeof a);
    a.G = G; a.T = T; a.S = S; a.R = R; a.W = W; a.n_used = (int)used.size(); a.len0 = len0; a.flags = flags & KAI_PLACE_PIPELINE_ONLY;
    a.gangs = d.gangs.data() + g0; a.tasks = d.tasks.data(); a.sets = d.sets.data(); a.rows_in = packed.data(); a.perm = ss.prep.perm.data();
    a.used_rows = used.data(); a.row_off = row_off.data(); a.list = list.data(); a.score_rows = d.score_rows.data(); a.deciles = d.deciles.data();
    a.head = &head; a.stamp = st.stamp.data(); a.answers = ans.data(); a.fail_at = fail_at.data(); a.ops = ops.data();
    const size_t items = std::max<size_t>(std::max<size_t>((size_t)T, (size_t)S), used.size() * 64);
    kw::launch((int)((items + lanes - 1) / lanes), lanes, 0, [&] { sp_prep_body(c, a); });
    for (int r : used) for (int i = row_off[(size_t)r]; i < row_off[(size_t)r + 1]; i++) if (list[(size_t)i] < 0 || list[(size_t)i] >= N || (i > row_off[(size_t)r] && list[(size_t)i] <= list[(size_t)i - 1])) return KAI_ERR_DEVICE_FAULT;  // every list filled, ascending
    const bool wide = !(flags & KAI_APPLY_ENGINE_PATH) && oa_wide_session(c);
    auto place = [&](bool w) {
        if (w) { SpWide ap; kw::launch(1, lanes, 0, [&] { sp_place_body(c, a, ap); }); }
        else {  // as k_sp_place_engine: one wavefront, no class index
            KaiCtx cv = c; cv.use_index = 0; HostBackend be; Engine<HostBackend> eng(cv, be); SpEngine<HostBackend> ap{eng};
            kw::launch(1, 64, 0, [&] { sp_place_body(cv, a, ap); });
        }
    };
    place(wide);
    if (head.bad != KAI_OA_NONE) { res.first_bad = head.bad; return KAI_ERR_STATE; }
    if (head.fault || head.applied != (wide ? KAI_APPLY_PATH_WIDE : KAI_APPLY_PATH_ENGINE) || head.len < len0 || head.len > len0 + T) { st.open = false; return KAI_ERR_DEVICE_FAULT; }
    const int n = head.len - len0;
    ops.resize((size_t)n);
    for (kai_op& o : ops) { o.node = ss.caller_node(o.node); st.rec.push_back((uint8_t)(o.kind | (wide ? 4 : 0))); }
    if (head.wrote) ss.index_stale = true;
    fail_at.resize((size_t)S);
    // fail_at of the sets of other gangs than [g0, g1) stay -1: reported as they are
    report(q, ans, fail_at, ops);
    res.path = wide ? KAI_APPLY_PATH_WIDE : KAI_APPLY_PATH_ENGINE; res.log_len = (int64_t)st.rec.size();
    int status = KAI_OK;
    if (!st.stamps_right(c) || c.st->ops_len != (int)st.rec.size() || c.st->n_undo != 0) status = KAI_ERR_DEVICE_FAULT;
    return status;
}

// kai_ordered_nodes_scored with k = 1 for one task, as kai_core.hip launches it: k_bn_prep, k_bn_range under bin-pack, k_on_scan_scored.  row: the caller's node set or NULL
kai_node_answer sim_scored_query1(SimSession& ss, const PlaceData& d, int pod, const uint32_t* row, uint32_t qflags, int scores, int lanes, int& n_found) {
    const KaiCtx& c = ss.ctx();
    const int W = (c.N + 31) / 32, S = row ? 1 : 0;
    kai_node_query nq; nq.pod = pod; nq.nodeset = row ? 0 : -1; nq.flags = qflags; nq.pad = scores;  // (kai_scored_query: the same layout)
    std::vector<uint32_t> rows((size_t)S * W + 1, 0u); std::vector<int32_t> need((size_t)2 * (S + 1), 0); std::vector<double> range((size_t)4 * (S + 1), 0.0);
    BnQuery prep{}; kai_node_answer one{-7, -7}, out{-7, -7}; int32_t n_out = -7;
    BnArgs a; std::memset((void*)&a, 0, sizeof a);
    a.M = 1; a.S = S; a.W = W; a.queries = &nq; a.rows_in = row; a.perm = ss.prep.perm.data();
    a.rows = rows.data(); a.need = need.data(); a.range = range.data(); a.prep = &prep; a.out = &one;
    const size_t items = std::max<size_t>(1, (size_t)S * W);
    kw::launch((int)((items + lanes - 1) / lanes), lanes, 0, [&] { bn_prep_body(c, a); });
    if ((c.plugins & KAI_PLUGIN_NODEPLACEMENT) && (c.gpu_strategy == KAI_BINPACK || c.cpu_strategy == KAI_BINPACK)) kw::launch(2 * (S + 1), lanes, 0, [&] { bn_range_body(c, a); });
    OnArgs o; std::memset((void*)&o, 0, sizeof o); o.k = 1; o.out = &out; o.n_out = &n_out;
    OnScoreArgs sa; std::memset((void*)&sa, 0, sizeof sa); sa.D = c.D; sa.rows = d.score_rows.data(); sa.deciles = d.deciles.data();
    kw::launch(1, lanes, 0, [&] { on_scan_scored_body(c, a, o, sa); });
    n_found = n_out;
    return out;
}

// the loop of kai_stmt_place's contract over the existing calls (include/kai_core.h), for the gangs [g0, g1)
int sim_place_loop(SimSession& ss, SimStmt& st, ApplyScratch& sc, const PlaceData& d, int g0, int g1, uint32_t flags, int lanes, std::vector<int32_t>& q, kai_stmt_result& res) {
    const KaiCtx& c = ss.ctx();
    res.first_bad = -1; res.path = KAI_APPLY_PATH_NONE; res.log_len = (int64_t)st.rec.size(); res.pad = 0;
    if (!st.open) return KAI_ERR_STATE;
    const int W = (c.N + 31) / 32;
    const int64_t len0 = (int64_t)st.rec.size();
    const uint32_t ep = flags & KAI_APPLY_ENGINE_PATH, qflags = (flags & KAI_PLACE_PIPELINE_ONLY) ? KAI_QUERY_PIPELINE_ONLY : 0u;
    std::vector<kai_place_answer> ans; std::vector<int32_t> fail_at(d.sets.size(), -1); std::vector<kai_op> ops;
    for (int g = g0; g < g1; g++) {
        const kai_place_gang& gg = d.gangs[(size_t)g];
        const int64_t cp = (int64_t)st.rec.size();  // kai_stmt_checkpoint
        kai_place_answer x{}; x.status = KAI_PLACE_NO_FIT; x.set = -1; x.first_op = cp - len0;
        for (int si = 0; si < gg.n_sets && x.set < 0; si++) {
            const int row = d.sets[(size_t)gg.first_set + si];
            x.sets_tried++;
            int fail = gg.n_tasks;
            for (int ti = 0; ti < gg.n_tasks; ti++) {
                const int p = d.tasks[(size_t)gg.first_task + ti];
                int found = 0;
                const kai_node_answer na = sim_scored_query1(ss, d, p, row < 0 ? nullptr : d.rows.data() + (size_t)row * W, qflags, gg.scores, lanes, found);
                if (found < 1) { fail = ti; break; }
                kai_op o; std::memset(&o, 0, sizeof o); o.kind = na.is_pipeline ? KAI_OP_PIPELINE : KAI_OP_ALLOCATE; o.pod = p; o.node = na.node; o.job = -1;
                if (int rc = sim_stmt_apply(ss, st, sc, &o, 1, ep, lanes, res)) return rc;
                o.job = c.p_job[p]; o.seq = (int64_t)st.rec.size() - 1;
                ops.push_back(o);
            }
            fail_at[(size_t)gg.first_set + si] = fail;
            if (fail == gg.n_tasks) { x.set = si; x.status = KAI_PLACE_PLACED; break; }
            if (int rc = sim_stmt_rollback(ss, st, cp, ep, false, lanes, res)) return rc;
            ops.resize((size_t)(cp - len0));
        }
        x.n_ops = (int64_t)st.rec.size() - cp;
        ans.push_back(x);
    }
    report(q, ans, fail_at, ops);
    res.log_len = (int64_t)st.rec.size();
    bool wide = !ep && oa_wide_session(c);
    for (int64_t i = len0; i < (int64_t)st.rec.size(); i++) if (!(st.rec[(size_t)i] & 4)) wide = false;
    res.path = wide ? KAI_APPLY_PATH_WIDE : KAI_APPLY_PATH_ENGINE;
    return KAI_OK;
}

}  // namespace

extern "C" {

// the place data of the scripts that follow (copied)
int kai_spsim_set(const kai_place_gang* gangs, int32_t n_gangs, const int32_t* tasks, int32_t n_tasks, const int32_t* sets, int32_t n_sets, const uint32_t* rows, int32_t n_rows, int32_t words,
                  const kai_topo_score_row* score_rows, const uint8_t* deciles, int32_t n_score_rows, int32_t n_domains) {
    if (n_gangs < 0 || n_tasks < 0 || n_sets < 0 || n_rows < 0 || n_score_rows < 0 || words < 0 || n_domains < 0) return KAI_ERR_INVALID_ARG;
    PlaceData& d = g_place;
    d.gangs.assign(gangs, gangs + n_gangs); d.tasks.assign(tasks, tasks + n_tasks); d.sets.assign(sets, sets + n_sets);
    d.rows.assign(rows, rows + (size_t)n_rows * words); d.rows.push_back(0u); d.R = n_rows;
    d.score_rows.assign(score_rows, score_rows + n_score_rows); d.score_rows.push_back(kai_topo_score_row{KAI_TOPO_SCORES_NONE, 0});
    d.deciles.assign(deciles, deciles + (size_t)n_score_rows * n_domains); d.deciles.push_back(0);
    return KAI_OK;
}

// kai_stsim_run's script runner (stmt_sim.cpp: the same arguments, rows and kinds 0 .. 6, 9, 10) with two more kinds over the gangs [lo, hi) of kai_spsim_set's data:
// 12 kai_stmt_place with `flags`; 13 the loop over the existing calls with `flags`.  Both report the same words (report() above).
int kai_spsim_run(const kai_config* cfg, const kai_snapshot_soa* s, int batch, const kai_op* ops, int64_t n_ops, const kai_stsim_call* calls, int n_calls,
                  int lanes, kai_stsim_ret* ret, int32_t* pod_status, int32_t* pod_node, kai_queue_share* shares, kai_node_state* nodes, int32_t* hidden, int64_t hidden_stride,
                  int32_t* q_out, int64_t q_stride, kai_op* ops_out, int64_t ops_cap, int64_t* n_ops_out, kai_action_stats* stats) {
    if (!cfg || !s || !calls || n_calls < 1 || lanes < 1 || lanes > 4096 || n_ops < 0 || !ret) return KAI_ERR_INVALID_ARG;
    const PlaceData& d = g_place;
    for (int64_t i = 0; i < n_ops; i++) if (ops[i].node < 0 || ops[i].node >= s->n_nodes || ops[i].pod < 0 || ops[i].pod >= s->n_pods || ops[i].kind < 0 || ops[i].kind > 2) return KAI_ERR_INVALID_ARG;
    for (int32_t p : d.tasks) if (p < 0 || p >= s->n_pods) return KAI_ERR_INVALID_ARG;
    for (int32_t r : d.sets) if (r < -1 || r >= d.R) return KAI_ERR_INVALID_ARG;
    for (const kai_place_gang& g : d.gangs) if (g.n_tasks < 1 || g.n_sets < 1 || g.first_task < 0 || g.first_task + g.n_tasks > (int)d.tasks.size() || g.first_set < 0 || g.first_set + g.n_sets > (int)d.sets.size() || g.scores < -1 || g.scores >= (int)d.score_rows.size() - 1) return KAI_ERR_INVALID_ARG;
    if (d.R && d.rows.size() != (size_t)d.R * ((s->n_nodes + 31) / 32) + 1) return KAI_ERR_INVALID_ARG;
    int n_actions = 0;
    for (int k = 0; k < n_calls; k++) {
        const kai_stsim_call& cl = calls[k];
        const bool known = (cl.kind >= 0 && cl.kind <= 6) || cl.kind == 9 || cl.kind == 10 || cl.kind == 12 || cl.kind == 13;
        if (!known) return KAI_ERR_INVALID_ARG;
        if (cl.kind == 10 && (cl.lo < 1 || cl.lo > KAI_ORDERED_MAX_K)) return KAI_ERR_INVALID_ARG;
        if ((cl.kind == 1 || cl.kind == 6) && (cl.lo < 0 || cl.hi < cl.lo || cl.hi > n_ops)) return KAI_ERR_INVALID_ARG;
        if ((cl.kind == 12 || cl.kind == 13) && (cl.lo < 0 || cl.hi < cl.lo || cl.hi > (int64_t)d.gangs.size())) return KAI_ERR_INVALID_ARG;
        if (cl.kind == 5) n_actions++;
    }
    SimSession ss;
    if (int rc = ss.open(cfg, s, n_actions, batch != 0)) return rc;
    const KaiCtx& c = ss.ctx();
    if (d.score_rows.size() > 1 && d.deciles.size() != (d.score_rows.size() - 1) * (size_t)c.D + 1) return KAI_ERR_INVALID_ARG;
    const int P = c.P, Q = c.Q, N = c.N;
    SimStmt st; static ApplyScratch scratch;
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
        } else if (cl.kind == 9 || cl.kind == 10) {
            const int kk = cl.kind == 10 ? (int)cl.lo : 0;
            std::vector<kai_node_query> nq;
            for (int p = 0; p < P; p++) if (c.p_status[p] == KAI_POD_PENDING) { kai_node_query x; x.pod = p; x.nodeset = -1; x.flags = 0; x.pad = 0; nq.push_back(x); }
            std::vector<kai_node_answer> out; std::vector<int32_t> n_out;
            sim_node_queries(ss, nq, nullptr, 0, kk, lanes, out, n_out);
            for (size_t i = 0; i < nq.size(); i++) {
                q.push_back(nq[i].pod);
                if (!kk) { q.push_back(out[i].node); q.push_back(out[i].is_pipeline); continue; }
                q.push_back(n_out[i]);
                for (int e = 0; e < kk; e++) { q.push_back(out[i * kk + e].node); q.push_back(out[i * kk + e].is_pipeline); }
            }
        } else if (cl.kind == 12) status = sim_stmt_place(ss, st, d, (int)cl.lo, (int)cl.hi, cl.flags, lanes, q, res);
        else status = sim_place_loop(ss, st, scratch, d, (int)cl.lo, (int)cl.hi, cl.flags, lanes, q, res);
        if (c.st->fault) return KAI_ERR_DEVICE_FAULT;
        // ---- the state behind the call (stmt_sim.cpp's rows)
        StateCopy g = ss.snapshot_state();
        g.hidden.push_back(c.fast_ok); g.hidden.push_back(ss.index_stale ? 1 : 0); g.hidden.push_back(st.open ? 1 : 0);
        g.hidden.push_back(st.open ? c.st->ops_len : 0); g.hidden.push_back(st.open ? c.st->n_undo : 0); g.hidden.push_back((int32_t)c.st->non_allocate_commits);
        if (st.open) for (int i = 0; i < c.st->ops_len; i++) { int32_t w[10]; std::memcpy(w, &c.ops[i], sizeof w); g.hidden.insert(g.hidden.end(), w, w + 10); }
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
