// kai_stmt_place.hpp — kai_stmt_place: allocatePodSet's loop over node sets with allocateTasksOnNodeSet inside (actions/common/allocate.go:83-107) for MANY gangs, inside the
// open Statement and over its own log, in two launches.  A task's answer depends on the state its predecessor left — the node it took, its queue's allocated amounts, the
// bin-pack pre-order range — so the chain runs on the device, where a step costs a scan of the node set and a barrier instead of two host round trips.
//
//   k_sp_prep    chip-wide.  A thread per task: Pending at entry, else the lowest offending index by atomic minimum into the head (nothing is written then); whether the
//                pod lies on no node and in no record (an invariant: a fault otherwise).  A thread per entry of `sets`: fail_at = -1.  A WAVEFRONT per set row the call names: the row's words
//                re-indexed to name-rank order (bn_reindex_word), their popcounts prefix-summed over the wavefront, the nodes written as an ascending name-rank list at the
//                row's offset (the host counted the rows' sizes: a popcount of the caller's words).  Ascending is what the tie-break needs; with the list a task's scan costs
//                |set| and not N.  Row -1 is the identity and has no list.
//   k_sp_place   ONE workgroup walks gangs, sets and tasks.  Per task: lane 0 forms the ScanReq (Engine::fill_req) and task_over_capacity at the CURRENT state and hands
//                them round through LDS; under bin-pack the pre-order range is reduced again over the WHOLE set (bn_range_body's arithmetic: earlier placements move
//                it); the lanes stride over the set's list with scan_node_score and the decile rule of on_scan_body_t<true> and fold "greater key, or equal key and lower
//                name rank" as bn_scan_body does; lane 0 takes the winner's is_pipeline from fits(..., false), applies the operation, writes its kai_op.  A set that has no
//                node for a task is undone back to the gang's checkpoint and the next set is tried.
//
// Two apply modes, one search.  SpWide (the session qualifies for the chip-wide kernels, oa_wide_session): the record and the state are written as st_apply_body writes
// them, a failed set is undone by the lanes, a record each (st_undo_record): the host marks the records `wide`.  SpEngine: the placing lane goes through the engine's own
// stmt_allocate / stmt_pipeline(…, true) and Engine::rollback(cp), as k_st_engine does; on the device that kernel is ONE wavefront (the engine's functions want its register
// budget) on the action kernel's LDS objects.
//
// No kernel waits on another workgroup.  Every cross-lane call is reached by whole wavefronts: the loops over gangs, sets and tasks, their exits and the strides' trip counts
// are the same in every lane (what decides them is read from LDS behind a barrier).  Every loop is bounded by the call's counts (the host admits sum n_tasks x n_sets <= 2^20)
// or by the size of a set.  A kw::sync() stands between every state write and the next scan that reads it; the node, queue and pod arrays are read through the ordinary
// vector path (no const __restrict__ on them: the scalar cache would serve stale lines).
//
// Written against kai_simt.hpp, so that tests/host_sim/stmt_place_sim.cpp runs the bodies with emulated lanes on a machine without a GPU.
#pragma once
#include "kai_ordered_nodes.hpp"
#include "kai_stmt.hpp"

namespace kai {

constexpr int64_t KAI_SP_MAX_WORK = (int64_t)1 << 20;  // sum of n_tasks x n_sets over the gangs of one call

// the call's verdict: sent with the call (bad = KAI_OA_NONE, len = the log's length before the call, the rest 0), read back with the answers
struct SpHead {
    int32_t bad;        // lowest index in `tasks` of a pod that is not Pending at entry
    int32_t pad0;
    int32_t applied;    // KAI_APPLY_PATH_WIDE / KAI_APPLY_PATH_ENGINE: that mode walked the gangs
    int32_t fault, fault_line;
    int32_t len;        // the log's length after the call
    int32_t wrote;      // an operation was applied (it may have been rolled back since): the class index is stale, as after kai_stmt_apply
    int32_t pad[9];
};
static_assert(sizeof(SpHead) == 64, "SpHead is one 64-byte record between what is sent and what comes back");

struct SpArgs {
    int32_t G, T, S, R;          // gangs, entries of tasks, entries of sets, node-set rows
    int32_t W, n_used, len0;     // words per row; rows the call names; the log's length before the call
    uint32_t flags;              // KAI_PLACE_PIPELINE_ONLY
    KAI_GP(const kai_place_gang) gangs; KAI_GP(const int32_t) tasks; KAI_GP(const int32_t) sets;
    KAI_GP(const uint32_t) rows_in;      // [n_used][W] the caller's rows that the sets name, in the order of used_rows, caller's node indices
    KAI_GP(const int32_t) perm;          // [N] name rank -> caller's node index
    KAI_GP(const int32_t) used_rows;     // [n_used] the rows that get a list
    KAI_GP(const int32_t) row_off;       // [R + 1] where a row's list starts in `list`; a row no set names has an empty one
    KAI_GP(int32_t) list;                // the lists: name ranks, ascending
    KAI_GP(const kai_topo_score_row) score_rows; KAI_GP(const uint8_t) deciles;
    KAI_GP(SpHead) head; KAI_GP(int32_t) stamp;  // the Statement's own stamps
    KAI_GP(kai_place_answer) answers;    // [G]
    KAI_GP(int32_t) fail_at;             // [S]
    KAI_GP(kai_op) ops;                  // [T] the surviving operations, ops[log position - len0], node = name rank
};

KW_BODY void sp_prep_body(const KaiCtx& c, const SpArgs& a) {
    const int64_t t = (int64_t)kw::bid() * kw::bdim() + kw::tid();
    if (t < a.T) {
        const int p = a.tasks[t];
        if (c.p_status[p] != KAI_POD_PENDING) kw::atomic_min((int32_t*)&a.head->bad, (int)t);
        // A Pending pod lies on no node and no surviving record names it: the open leaves p_on_node = -1 for every pod that is not active-used, every operation of the log
        // takes its pod out of Pending, and both undo paths clear p_on_node when they bring it back.  So every task starts from the state the chip-wide apply takes
        // (k_oa_check's `wide`); a session that breaks this is reported as a fault and nothing is written.
        else if (c.p_on_node[p] >= 0 || a.stamp[p] != 0) { a.head->fault = FAULT_INTERNAL; a.head->fault_line = __LINE__; }
    }
    if (t < a.S) a.fail_at[t] = -1;
    const int64_t wv = t >> 6;  // the same in every lane of a wavefront (the block size is a multiple of 64)
    if (wv < a.n_used) {
        const int lane = kw::lane(), row = a.used_rows[wv];
        KAI_GP(const uint32_t) in = a.rows_in + (size_t)wv * a.W;
        int base = a.row_off[row];
        const int end = a.row_off[row + 1];
        for (int w0 = 0; w0 < a.W; w0 += 64) {  // the trip count is the wavefront's
            const int w = w0 + lane;
            uint32_t word = w < a.W ? bn_reindex_word(c.N, in, a.perm, w) : 0u;
            const int cnt = __builtin_popcount(word);
            const int incl = kw::wave_scan_add(cnt);
            int o = base + incl - cnt;
            while (word) {
                const int b = __builtin_ctz(word); word &= word - 1;
                if (o < end) a.list[o] = w * 32 + b;  // (the host's count is the row's popcount over the N nodes: the bound never cuts)
                o++;
            }
            base += kw::shfl(incl, 63);
        }
    }
}

// the chip-wide mode's apply and undo: what st_apply_body and st_undo_body do per record, by the placing lane and by a lane per record
struct SpWide {
    static constexpr bool kWide = true;
    KW_BODY bool begin(const KaiCtx&, const SpArgs&) { return true; }
    KW_BODY bool apply(const KaiCtx& c, const SpArgs& a, int kind, int p, int n, int len) {
        const int j = c.p_job[p];
        StmtOp r{}; r.pod = p; r.op_index = -1; r.prev_virtual = c.p_virtual[p];  // as push_op gets it from stmt_allocate / stmt_pipeline
        kw::atomic_add((int32_t*)&a.stamp[p], 1);
        c.p_accepted[p] = 1; c.j_tta_valid[j] = 0; c.p_virtual[p] = 1;
        if (kind == KAI_OP_ALLOCATE) {
            r.name = OP_ALLOCATE; r.next_node = n;
            c.p_status[p] = KAI_POD_ALLOCATED; c.p_node[p] = n; c.p_on_node[p] = n; c.p_on_node_status[p] = KAI_POD_ALLOCATED;
        } else {
            r.name = OP_PIPELINE; r.prev_status = c.p_status[p]; r.prev_node = c.p_node[p]; r.next_node = n;
#ifdef KAI_SHARED_GPUS
            r.pad = -1;  // (no shared-GPU group: the Statement takes no such session)
#endif
            c.p_status[p] = KAI_POD_PIPELINED; c.p_node[p] = n; c.p_on_node[p] = n; c.p_on_node_status[p] = KAI_POD_PIPELINED;
        }
        c.ops[len] = r;
        st_amounts(c, nullptr, 0, kind, p, n, 1.0);
        return true;
    }
    KW_BODY void end(const KaiCtx& c, const SpArgs& a, int len) { c.st->ops_len = len; a.head->len = len; a.head->applied = KAI_APPLY_PATH_WIDE; }
};

// the engine mode: the placing lane through the engine's own Statement functions, as st_engine_walk.  The log must be the Statement's, without an OP_UNDO on it.
template <class Backend>
struct SpEngine {
    static constexpr bool kWide = false;
    Engine<Backend>& eng;
    KAI_HD void say_fault(const KaiCtx& c, const SpArgs& a) { a.head->fault = c.st->fault ? c.st->fault : FAULT_INTERNAL; a.head->fault_line = c.st->fault ? c.st->fault_line : __LINE__; }
    KAI_HD bool begin(const KaiCtx& c, const SpArgs& a) {
        EngineState& st = *c.st;
        if (st.ops_len != a.len0 || st.n_undo != 0) { st.fault = 0; say_fault(c, a); return false; }
        st.fault = 0; st.fault_line = 0;
        eng.el().h.out_len = 0; eng.el().h.stmts = 0;
        return true;
    }
    KAI_HD bool apply(const KaiCtx& c, const SpArgs& a, int kind, int p, int n, int) {
        a.stamp[p]++;
        const bool ok = kind == KAI_OP_ALLOCATE ? eng.stmt_allocate(p, n) : eng.stmt_pipeline(p, n, true);
        if (!ok) eng.fault(FAULT_INTERNAL);
        if (c.st->fault) { say_fault(c, a); return false; }
        return true;
    }
    KAI_HD bool rollback(const KaiCtx& c, const SpArgs& a, int cp, int len) {
        for (int i = cp; i < len; i++) a.stamp[c.ops[i].pod]--;
        eng.rollback(cp);
        if (c.st->fault || c.st->ops_len != cp || c.st->n_undo != 0) { say_fault(c, a); return false; }
        return true;
    }
    KAI_HD void end(const KaiCtx& c, const SpArgs& a, int len) {
        if (c.st->ops_len != len) { say_fault(c, a); return; }
        a.head->len = len; a.head->applied = KAI_APPLY_PATH_ENGINE;
    }
};

template <class Ap>
KW_BODY void sp_place_body(const KaiCtx& c, const SpArgs& a, Ap& ap) {
    KW_SHARED ScanReq s_q;
    KW_SHARED int32_t s_dead, s_node, s_stop;
    KW_SHARED uint64_t part_key[KAI_BN_MAX_WAVES]; KW_SHARED int32_t part_node[KAI_BN_MAX_WAVES];
    KW_SHARED double part_lo[KAI_BN_MAX_WAVES], part_hi[KAI_BN_MAX_WAVES];
    const int tid = kw::tid(), lanes = kw::bdim(), lane = kw::lane(), wave = tid >> 6, nw = (lanes + 63) / 64;
    const int wl = lanes - wave * 64 < 64 ? lanes - wave * 64 : 64;  // lanes of this wave
    // the same for every lane: the prep kernel finished before this one started
    if (a.head->bad != KAI_OA_NONE) return;          // a task is not Pending: refused, nothing is written
    if (a.head->fault) return;                       // (k_sp_prep: a Pending pod on a node or in the log)
    if (tid == 0) s_stop = ap.begin(c, a) ? 0 : 1;
    kw::sync();
    if (s_stop) return;
    BnBackend nb; Engine<BnBackend> eng(c, nb);      // the engine's pure helpers over this context (fill_req, task_over_capacity)
    const bool pipeline_only = (a.flags & KAI_PLACE_PIPELINE_ONLY) != 0;
    int len = a.len0;                                // the log's length: every lane counts it the same way
    for (int g = 0; g < a.G; g++) {
        const kai_place_gang gg = a.gangs[g];
        int trow = -1; KAI_GP(const uint8_t) dec = nullptr; bool no_scores = false;  // the level row the nodes' domains are read from and the gang's deciles; -1: no topology term
        if ((c.plugins & KAI_PLUGIN_TOPOLOGY) && gg.scores >= 0) {
            const int lr = a.score_rows[gg.scores].level_row;
            if (lr == KAI_TOPO_SCORES_EMPTY) no_scores = true;  // scores were recorded and no node has one: every node is dropped
            else if (lr >= 0) { trow = lr; dec = a.deciles + (size_t)gg.scores * (size_t)c.D; }
        }
        const int cp = len;                          // kai_stmt_checkpoint
        int took = -1, tried = 0;
        for (int si = 0; si < gg.n_sets && took < 0; si++) {
            const int row = a.sets[gg.first_set + si];
            const int cnt = row < 0 ? c.N : a.row_off[row + 1] - a.row_off[row];
            KAI_GP(const int32_t) list = a.list + (row < 0 ? 0 : a.row_off[row]);
            tried++;
            int fail = gg.n_tasks;
            for (int ti = 0; ti < gg.n_tasks; ti++) {
                const int p = a.tasks[gg.first_task + ti];
                if (tid == 0) {
                    eng.fill_req(s_q, p);
                    s_dead = (no_scores || ((c.plugins & KAI_PLUGIN_PREDICATES) && eng.task_over_capacity(p))) ? 1 : 0;
                }
                kw::sync();
                ScanReq q = s_q;
                if (s_dead) { fail = ti; break; }    // over its queue's capacity: an empty answer without a scan
                if ((c.plugins & KAI_PLUGIN_NODEPLACEMENT) && q.strategy == KAI_BINPACK) {  // NodePreOrderFn: getMinMaxPerNode over the whole set, at the state reached
                    const int r = q.r_place == KAI_RES_GPU ? KAI_RES_GPU : KAI_RES_CPU;
                    double lo = 1.7976931348623157e308, hi = 0;  // math.MaxFloat64, 0 (pack.go:66-68)
                    for (int i = tid; i < cnt; i += lanes) {
                        const int n = row < 0 ? i : list[i];
                        if (c.n_alloc[(size_t)r * c.N + n] == 0) continue;
                        const double cur = c.n_idle[(size_t)r * c.N + n] + c.n_rel[(size_t)r * c.N + n];
                        if (cur < lo) lo = cur;
                        if (cur > hi) hi = cur;
                    }
                    for (int o = 32; o > 0; o >>= 1) {
                        const int src = (lane ^ o) < wl ? (lane ^ o) : lane;
                        const double x = kw::shfl(lo, src), y = kw::shfl(hi, src);
                        if (x < lo) lo = x;
                        if (y > hi) hi = y;
                    }
                    if (lane == 0) { part_lo[wave] = lo; part_hi[wave] = hi; }
                    kw::sync();
                    lo = part_lo[0]; hi = part_hi[0];
                    for (int w = 1; w < nw; w++) { if (part_lo[w] < lo) lo = part_lo[w]; if (part_hi[w] > hi) hi = part_hi[w]; }
                    q.min_a = lo; q.max_a = hi;
                }
                int best = -1; uint64_t bk = 0;
                for (int i = tid; i < cnt; i += lanes) {  // ascending: a later node takes over only with a greater key
                    const int n = row < 0 ? i : list[i];
                    double sc = 0;
                    if (!scan_node_score(c, q, n, sc)) continue;
                    if (trow >= 0) {  // a node without a score is dropped (framework/session.go:247-251)
                        const int dd = c.node_domain[(size_t)trow * c.N + n];
                        const int dv = (dd >= 0 && dd < c.D) ? dec[dd] : KAI_TOPO_NO_SCORE;
                        if (dv == KAI_TOPO_NO_SCORE) continue;
                        sc += dv * KAI_TOPO_SCORE_UNIT;
                    }
                    const uint64_t k = bn_orderable(sc);
                    if (best < 0 || k > bk) { best = n; bk = k; }
                }
                // over the wave: the greatest key, then the lowest name rank among the lanes that hold it (0 = no candidate)
                if (best < 0) bk = 0;
                const uint64_t wk = kw::wave_max_u64(bk);
                const uint64_t mine = (best >= 0 && bk == wk) ? (uint64_t)(0x7fffffff - best) + 1 : 0;
                const uint64_t wn = kw::wave_max_u64(mine);
                if (lane == 0) { part_key[wave] = wk; part_node[wave] = wn ? 0x7fffffff - (int32_t)(wn - 1) : -1; }
                kw::sync();
                if (tid == 0) {
                    int node = -1; uint64_t key = 0;
                    for (int w = 0; w < nw; w++) {
                        const int n = part_node[w]; const uint64_t k = part_key[w];
                        if (n < 0) continue;
                        if (node < 0 || k > key || (k == key && n < node)) { node = n; key = k; }  // greater key, or equal key and lower name rank
                    }
                    if (node >= 0) {
                        bool allocatable = q.best_effort || fits(c, q.req, node, false);  // NodeInfo.IsTaskAllocatable (Engine::find_node)
#ifdef KAI_SHARED_GPUS
                        if (c.shared_on && q.shared) allocatable = q.best_effort || fits_shared(c, q, node, false);
#endif
                        const int kind = (pipeline_only || !allocatable) ? KAI_OP_PIPELINE : KAI_OP_ALLOCATE;
                        if (!ap.apply(c, a, kind, p, node, len)) s_stop = 1;
                        a.head->wrote = 1;
                        kai_op o; o.seq = len; o.kind = kind; o.pod = p; o.node = node; o.job = c.p_job[p]; o.stmt = 0; o.pad = 0;
                        a.ops[len - a.len0] = o;
                    }
                    s_node = node;
                }
                kw::sync();  // the state the operation wrote is read by the next task's scan
                if (s_stop) return;
                if (s_node < 0) { fail = ti; break; }
                len++;
            }
            if (tid == 0) a.fail_at[gg.first_set + si] = fail;
            if (fail == gg.n_tasks) { took = si; break; }
            // the set failed: its operations are undone back to the gang's checkpoint
            if constexpr (Ap::kWide) {
                for (int i = cp + tid; i < len; i += lanes) { const StmtOp op = c.ops[i]; (void)st_undo_record(c, a.stamp, nullptr, 0, op); }
            } else {
                if (tid == 0 && len > cp && !ap.rollback(c, a, cp, len)) s_stop = 1;
            }
            kw::sync();  // ... before the next set's scans, and before lane 0 writes the next request
            if (s_stop) return;
            len = cp;
        }
        if (tid == 0) {
            kai_place_answer ans;
            ans.status = took >= 0 ? KAI_PLACE_PLACED : KAI_PLACE_NO_FIT; ans.set = took; ans.sets_tried = tried; ans.pad = 0;
            ans.first_op = cp - a.len0; ans.n_ops = len - cp;
            a.answers[g] = ans;
        }
    }
    if (tid == 0) ap.end(c, a, len);
}

// Where the pieces of one call lie in the handle's scratch (device) and staging (pinned host), 16-byte aligned.  The permutation comes first, at an offset no call moves;
// [gangs | tasks | sets | used rows | row offsets | the NAMED rows | score rows | deciles | head] is what every call sends, in ONE copy (with the permutation in front of it on the
// first call of a session); [head | answers | fail_at | operations] is what comes back, in ONE copy; the lists lie behind.
struct SpLayout {
    size_t perm, gangs, tasks, sets, used, row_off, rows_in, score_rows, deciles, head, answers, fail_at, ops, down_end, list, end;
    SpLayout(int N, int G, int T, int S, int R, int W, int n_used, int n_score_rows, int D, size_t list_len) {
        auto al = [](size_t x) { return (x + 15) & ~(size_t)15; };
        size_t o = 0;
        perm = o; o = al(o + (size_t)(N > 0 ? N : 1) * 4);
        gangs = o; o = al(o + (size_t)G * sizeof(kai_place_gang));
        tasks = o; o = al(o + (size_t)T * 4);
        sets = o; o = al(o + (size_t)S * 4);
        used = o; o = al(o + (size_t)n_used * 4 + 4);
        row_off = o; o = al(o + ((size_t)R + 1) * 4);
        rows_in = o; o = al(o + (size_t)n_used * W * 4 + 4);
        score_rows = o; o = al(o + (size_t)n_score_rows * sizeof(kai_topo_score_row) + 8);
        deciles = o; o = al(o + (size_t)n_score_rows * (size_t)(D > 0 ? D : 0) + 1);
        head = o; o += sizeof(SpHead);
        answers = o; o = al(o + (size_t)G * sizeof(kai_place_answer));
        fail_at = o; o = al(o + (size_t)S * 4);
        ops = o; o = al(o + (size_t)T * sizeof(kai_op));
        down_end = o;
        list = o; o = al(o + list_len * 4 + 4);
        end = o;
    }
};

}  // namespace kai

#if defined(__HIPCC__)
namespace kai {
__global__ void __launch_bounds__(KAI_BN_WG) k_sp_prep(KaiCtx c, SpArgs a) { sp_prep_body(c, a); }
__global__ void __launch_bounds__(KAI_BN_WG) k_sp_place(KaiCtx c, SpArgs a) { SpWide ap; sp_place_body(c, a, ap); }
__global__ void __launch_bounds__(64) k_sp_place_engine(KaiCtx cv, SpArgs a) {
    if (threadIdx.x == 0) { g_ctx = cv; g_ctx.use_index = 0; g_ctx.sg = nullptr; g_ctx.sg_wgs = 0; g_ctx.mw = nullptr; g_ctx.mw_rank = 0; g_ctx.mw_world = 1; }
    __syncthreads();
    DevBackendT<true, false> be;
    Engine<DevBackendT<true, false>> eng(g_ctx, be);  // (every lane writes the same values into the engine's LDS scalars; only the placing lane uses the object)
    __syncthreads();
    SpEngine<DevBackendT<true, false>> ap{eng};
    sp_place_body(g_ctx, a, ap);
}
}  // namespace kai
#endif
