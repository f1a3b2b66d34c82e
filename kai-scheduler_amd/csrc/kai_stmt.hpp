// kai_stmt.hpp — kai_stmt_*: ONE open (uncommitted) Statement on the handle, as framework.Statement is used by the allocate loop (framework/statement.go:44-61, 522-575;
// actions/common/allocate.go): operations are applied without the commit, logged on the device, rolled back to a checkpoint, discarded or committed.
//
// One log, two paths.  The log is the engine's own: StmtOp records in KaiCtx::ops, its length in EngineState::ops_len — so that either path can take over at any point.
//   k_oa_check   (kai_ops_apply.hpp) the batch's verdict; `stamp` is the Statement's own array here: how often the SURVIVING LOG names a pod, so that "named more than
//                once" also sees the operations of earlier calls.  It lives as long as the Statement; records that leave the log take their stamps with them.
//   k_st_apply   the chip-wide apply, a thread per operation, behind the check's verdict: oa_wide_body without the Allocated -> Binding step, and ops[len + i] written
//                exactly as Engine::stmt_allocate / stmt_pipeline / stmt_evict write it.
//   k_st_undo    a thread per record of [cp, len): the inverse of its operation (Engine::unallocate / unpipeline / unevict) with the same f64 atomics.  Order-free for
//                the reason the apply is: the session's quantities add exactly (KaiCtx::exact_sums), and the range names every pod once.
//   k_st_commit  a thread per record: Allocated -> Binding, p_virtual = 0 for evictions, the count of committed evictions / pipelines, the kai_op handed back.
//   k_st_engine  everything else, by ONE lane through the engine's own Statement functions: stmt_* without commit, Engine::rollback / discard / commit(emit).  It never
//                zeroes ops_len / n_undo.
// Which records the chip-wide kernels may undo or commit is the host's knowledge (kai_core.hip keeps one byte per record): a record is `wide` when the batch that wrote it
// named every pod once — in the surviving log and the batch — and every operation started from a state k_oa_check calls wide.  A range of wide records holds no OP_UNDO
// (no call leaves one on the log: Engine::rollback truncates what it pushed) and names every pod once.
//
// The log's room.  Engine::rollback pushes one OP_UNDO record per undone operation on top of the log before it truncates; a discard of a log of L records therefore
// needs 2 L <= ops_cap.  st_log_room(c) = ops_cap / 2 = 2 P + 32 records is what kai_stmt_apply admits.
//
// No kernel waits on another workgroup; every loop is bounded by the number of operations or records, or by the height of the queue tree.
// The bodies are written against kai_simt.hpp, so that tests/host_sim/stmt_sim.cpp runs them with emulated lanes on a machine without a GPU.
#pragma once
#include "kai_ops_apply.hpp"

namespace kai {

enum StMode : int32_t { KAI_ST_APPLY = 0, KAI_ST_ROLLBACK = 1, KAI_ST_DISCARD = 2, KAI_ST_COMMIT = 3 };

struct StArgs {
    OaArgs a;                 // apply: the batch, its verdict, the shadow; every call: head and stamp (the Statement's own)
    int32_t len, cp;          // the log's length before the call; rollback: the records [cp, len) go
    int32_t mode, pad;
    KAI_GP(kai_op) out; int64_t out_cap;  // commit: the surviving operations, nodes as name ranks
};

inline int st_log_room(const KaiCtx& c) { return c.ops_cap / 2; }

// the amounts of one operation on its node, its pod-set, its job and up its queue chain: added (dir = 1) or taken back (dir = -1)
KW_BODY void st_amounts(const KaiCtx& c, double* s_acc, int n_in, int kind, int p, int n, double dir) {
    const BatchCtx& b = c.bt;
    const int j = c.p_job[p], s = c.p_podset[p], d = dir > 0 ? 1 : -1;
    const double q3[3] = {c.p_req[(size_t)KAI_RES_CPU * c.P + p], c.p_req[(size_t)KAI_RES_MEM * c.P + p], c.p_req[(size_t)KAI_RES_GPU * c.P + p]};
    double sign = dir;
    if (kind == KAI_OP_ALLOCATE) {
        for (int r = 0; r < c.R; r++) {
            const double v = c.p_req[(size_t)r * c.P + p]; if (v == 0) continue;
            kw::atomic_add((double*)&c.n_used[(size_t)r * c.N + n], dir * v); kw::atomic_add((double*)&c.n_idle[(size_t)r * c.N + n], -dir * v);
        }
        kw::atomic_add((int32_t*)&c.s_active_alloc[s], d); kw::atomic_add((int32_t*)&c.s_active_used[s], d); kw::atomic_add((int32_t*)&c.j_n_pending[j], -d);
        for (int k = 0; k < 3; k++) if (q3[k] != 0) kw::atomic_add((double*)&c.j_allocated[(size_t)j * 4 + k], dir * q3[k]);
    } else if (kind == KAI_OP_PIPELINE) {  // the node's Releasing pays for a pipelined pod
        for (int r = 0; r < c.R; r++) {
            const double v = c.p_req[(size_t)r * c.P + p]; if (v == 0) continue;
            kw::atomic_add((double*)&c.n_used[(size_t)r * c.N + n], dir * v); kw::atomic_add((double*)&c.n_rel[(size_t)r * c.N + n], -dir * v);
        }
        kw::atomic_add((int32_t*)&c.s_active_alloc[s], d); kw::atomic_add((int32_t*)&c.s_active_used[s], d); kw::atomic_add((int32_t*)&c.s_pipelined[s], d);
        kw::atomic_add((int32_t*)&c.j_n_pending[j], -d);
    } else {  // placed <-> Releasing on its node: Idle and Used stay
        for (int r = 0; r < c.R; r++) {
            const double v = c.p_req[(size_t)r * c.P + p]; if (v == 0) continue;
            kw::atomic_add((double*)&c.n_rel[(size_t)r * c.N + n], dir * v);
        }
        kw::atomic_add((int32_t*)&c.s_active_alloc[s], -d); kw::atomic_add((int32_t*)&c.s_alive[s], -d);
        for (int k = 0; k < 3; k++) if (q3[k] != 0) kw::atomic_add((double*)&c.j_allocated[(size_t)j * 4 + k], -dir * q3[k]);
        sign = -dir;
    }
    if (c.plugins & KAI_PLUGIN_PROPORTION) {  // AllocateFunc / DeallocateFunc (plugins/proportion/proportion.go:443-489)
        const bool np = !c.j_preempt[j];
        for (int q = c.j_queue[j]; q >= 0; q = c.q_parent[q]) {
            const int slot = n_in ? b.q_islot[q] : -1;
            for (int k = 0; k < 3; k++) {
                const double v = sign * q3[k]; if (v == 0) continue;
                if (slot >= 0 && slot < n_in) { kw::atomic_add(&s_acc[slot * 6 + k], v); if (np) kw::atomic_add(&s_acc[slot * 6 + 3 + k], v); }
                else { kw::atomic_add((double*)&c.q_share[(size_t)q * 3 + k].allocated, v); if (np) kw::atomic_add((double*)&c.q_share[(size_t)q * 3 + k].allocated_np, v); }
            }
        }
    }
}
// the workgroup's sums of the inner queue nodes, one atomic each
KW_BODY void st_flush_inner(const KaiCtx& c, const double* s_acc, int n_in) {
    const BatchCtx& b = c.bt;
    for (int k = kw::tid(); k < n_in * 6; k += kw::bdim()) {
        const double v = s_acc[k]; if (v == 0) continue;
        const int q = b.h_nodes[b.h_off[1] + k / 6], r = k % 3;
        if (k % 6 < 3) kw::atomic_add((double*)&c.q_share[(size_t)q * 3 + r].allocated, v); else kw::atomic_add((double*)&c.q_share[(size_t)q * 3 + r].allocated_np, v);
    }
}
KAI_HD int st_n_inner(const KaiCtx& c, const OaArgs& a, bool go) { return (go && a.use_islot) ? (c.bt.n_inner < KB_APPLY_INNER ? c.bt.n_inner : KB_APPLY_INNER) : 0; }

KW_BODY void st_apply_body(const KaiCtx& c, const StArgs& s) {
    KW_SHARED double s_acc[KB_APPLY_INNER * 6];
    const OaArgs& a = s.a;
    const int tid = kw::tid(), T = kw::bdim();
    const int64_t i = (int64_t)kw::bid() * T + tid;
    // the same for every lane of the grid: the check kernel finished before this one started.  What st_apply_drive does with the verdict, decided here the same way
    const bool check_only = (a.flags & KAI_APPLY_CHECK_ONLY) != 0, dup = a.head->dup != 0;
    const bool refused = !dup && a.head->bad != KAI_OA_NONE;
    const bool engine = (a.flags & (KAI_APPLY_ENGINE_PATH | KAI_OA_NOT_WIDE)) != 0 || dup || a.head->not_wide != 0;
    const bool go = !refused && !engine && !check_only;
    const bool engine_runs = !refused && engine && (!check_only || dup);  // the walk keeps the stamps or takes them back itself
    const int n_in = st_n_inner(c, a, go);
    for (int k = tid; k < n_in * 6; k += T) s_acc[k] = 0.0;
    kw::sync();
    if (i < a.n) {
        const kai_op o = a.ops[i];
        const int p = o.pod;
        if (go) {
            const int j = c.p_job[p];
            StmtOp r{}; r.pod = p; r.op_index = -1; r.prev_virtual = c.p_virtual[p];  // as push_op gets it from stmt_allocate / stmt_pipeline / stmt_evict
            int n = o.node;
            c.p_accepted[p] = 1; c.j_tta_valid[j] = 0; c.p_virtual[p] = 1;
            if (o.kind == KAI_OP_ALLOCATE) {
                r.name = OP_ALLOCATE; r.next_node = n;
                c.p_status[p] = KAI_POD_ALLOCATED; c.p_node[p] = n; c.p_on_node[p] = n; c.p_on_node_status[p] = KAI_POD_ALLOCATED;
            } else if (o.kind == KAI_OP_PIPELINE) {
                r.name = OP_PIPELINE; r.prev_status = c.p_status[p]; r.prev_node = c.p_node[p]; r.next_node = n;
#ifdef KAI_SHARED_GPUS
                r.pad = -1;  // (no shared-GPU group: the chip-wide path takes no such session)
#endif
                c.p_status[p] = KAI_POD_PIPELINED; c.p_node[p] = n; c.p_on_node[p] = n; c.p_on_node_status[p] = KAI_POD_PIPELINED;
            } else {
                n = c.p_node[p];  // (= o.node: the check's precondition)
                r.name = OP_EVICT; r.prev_status = c.p_status[p]; r.prev_node = n;
#ifdef KAI_SHARED_GPUS
                r.pad = -1;
#endif
                c.p_status[p] = KAI_POD_RELEASING; c.p_on_node_status[p] = KAI_POD_RELEASING;
            }
            c.ops[s.len + i] = r;
            st_amounts(c, s_acc, n_in, o.kind, p, n, 1.0);
        } else if (!engine_runs) kw::atomic_add((int32_t*)&a.stamp[p], -1);  // the batch does not join the log: what the check counted goes
    }
    kw::sync();
    st_flush_inner(c, s_acc, n_in);
    if (go && i == 0) { a.head->applied = KAI_APPLY_PATH_WIDE; c.st->ops_len = s.len + a.n; }
}

// one record undone (k_st_undo: a thread per record; k_sp_place: a lane per record of a set that failed).  false: an OP_UNDO record, nothing written
KW_BODY bool st_undo_record(const KaiCtx& c, KAI_GP(int32_t) stamp, double* s_acc, int n_in, const StmtOp& op) {
    const int p = op.pod;
    if (op.name != OP_ALLOCATE && op.name != OP_PIPELINE && op.name != OP_EVICT) return false;
    kw::atomic_add((int32_t*)&stamp[p], -1);
    c.j_tta_valid[c.p_job[p]] = 0; c.p_virtual[p] = (uint8_t)op.prev_virtual;
    if (op.name == OP_ALLOCATE) {  // Engine::unallocate
        st_amounts(c, s_acc, n_in, KAI_OP_ALLOCATE, p, c.p_node[p], -1.0);
        c.p_status[p] = KAI_POD_PENDING; c.p_node[p] = -1; c.p_on_node[p] = -1;
    } else if (op.name == OP_PIPELINE) {  // Engine::unpipeline
        st_amounts(c, s_acc, n_in, KAI_OP_PIPELINE, p, c.p_node[p], -1.0);
        c.p_status[p] = op.prev_status; c.p_node[p] = op.prev_node; c.p_on_node[p] = -1;
    } else {  // Engine::unevict: the node's copy is taken off and added again with the status that comes back
        st_amounts(c, s_acc, n_in, KAI_OP_EVICT, p, op.prev_node, -1.0);
        c.p_status[p] = op.prev_status; c.p_on_node_status[p] = op.prev_status;
    }
    return true;
}

KW_BODY void st_undo_body(const KaiCtx& c, const StArgs& s) {
    KW_SHARED double s_acc[KB_APPLY_INNER * 6];
    const OaArgs& a = s.a;
    const int tid = kw::tid(), T = kw::bdim();
    const int64_t i = (int64_t)kw::bid() * T + tid;
    const int n_in = st_n_inner(c, a, true);
    for (int k = tid; k < n_in * 6; k += T) s_acc[k] = 0.0;
    kw::sync();
    if (i < s.len - s.cp) {
        const StmtOp op = c.ops[s.cp + i];
        if (!st_undo_record(c, a.stamp, s_acc, n_in, op)) { a.head->fault = FAULT_INTERNAL; a.head->fault_line = __LINE__; }  // (an OP_UNDO record: the host never sends such a range here)
    }
    kw::sync();
    st_flush_inner(c, s_acc, n_in);
    if (i == 0) { a.head->applied = KAI_APPLY_PATH_WIDE; c.st->ops_len = s.cp; }
}

KW_BODY void st_commit_body(const KaiCtx& c, const StArgs& s) {
    KW_SHARED int32_t s_non_alloc;
    const OaArgs& a = s.a;
    const int tid = kw::tid(), T = kw::bdim();
    const int64_t i = (int64_t)kw::bid() * T + tid;
    if (tid == 0) s_non_alloc = 0;
    kw::sync();
    if (i < s.len) {
        const StmtOp op = c.ops[i];
        const int p = op.pod;
        kw::atomic_add((int32_t*)&a.stamp[p], -1);
        kai_op o; o.seq = i; o.pod = p; o.job = c.p_job[p]; o.node = c.p_node[p]; o.stmt = 0; o.pad = 0;
        if (op.name == OP_EVICT) { o.kind = KAI_OP_EVICT; o.node = op.prev_node; c.p_virtual[p] = 0; kw::atomic_add(&s_non_alloc, 1); }
        else if (op.name == OP_PIPELINE) { o.kind = KAI_OP_PIPELINE; kw::atomic_add(&s_non_alloc, 1); }
        else { o.kind = KAI_OP_ALLOCATE; c.p_status[p] = KAI_POD_BINDING; c.j_tta_valid[o.job] = 0; }  // ssn.BindPod: the counters do not tell Allocated from Binding
        s.out[i] = o;
    }
    kw::sync();
    if (tid == 0 && s_non_alloc) kw::atomic_add((unsigned long long*)&c.st->non_allocate_commits, (unsigned long long)s_non_alloc);
    if (i == 0) { a.head->applied = KAI_APPLY_PATH_WIDE; c.st->ops_len = 0; }
}

// The engine walk of every kai_stmt_* call, by ONE lane (the device: lane 0 of k_st_engine's only workgroup).  c.use_index is 0; commit: c.out_ops / c.out_cap are the
// call's own (s.out).  The log is the Statement's: its length must be what the host counted, and no call leaves an OP_UNDO on it.
template <class Backend>
KAI_HD void st_engine_walk(const KaiCtx& c, Backend& be, const StArgs& s) {
    const OaArgs& a = s.a;
    EngineState& st = *c.st;
    auto unstamp = [&](int lo, int hi) { for (int i = lo; i < hi; i++) a.stamp[c.ops[i].pod]--; };
    if (s.mode == KAI_ST_APPLY) {
        // ---- the validation walk of oa_engine_walk: every operation against the state its predecessors leave, on a shadow
        int bad = KAI_OA_NONE;
        for (int i = 0; i < a.n; i++) {
            const kai_op o = a.ops[i];
            const bool own = a.sh_status[o.pod] != 0;
            int ps = own ? a.sh_status[o.pod] : c.p_status[o.pod], nd = own ? a.sh_node[o.pod] : c.p_node[o.pod];
            if (!oa_pre_ok(o.kind, ps, nd, o.node)) { bad = i; break; }
            if (o.kind == KAI_OP_ALLOCATE) { ps = KAI_POD_ALLOCATED; nd = o.node; } else if (o.kind == KAI_OP_PIPELINE) { ps = KAI_POD_PIPELINED; nd = o.node; } else ps = KAI_POD_RELEASING;
            a.sh_status[o.pod] = ps; a.sh_node[o.pod] = nd;
        }
        for (int i = 0; i < a.n; i++) a.sh_status[a.ops[i].pod] = 0;
        a.head->bad = bad;
        if (bad != KAI_OA_NONE || (a.flags & KAI_APPLY_CHECK_ONLY)) { for (int i = 0; i < a.n; i++) a.stamp[a.ops[i].pod]--; return; }
    }
    if (st.ops_len != s.len || st.n_undo != 0) {  // (the log is not the Statement's: nothing is written)
        if (s.mode == KAI_ST_APPLY) for (int i = 0; i < a.n; i++) a.stamp[a.ops[i].pod]--;
        a.head->fault = FAULT_INTERNAL; a.head->fault_line = __LINE__; return;
    }
    Engine<Backend> eng(c, be);
    st.fault = 0; st.fault_line = 0;
    eng.el().h.out_len = 0; eng.el().h.stmts = 0;
    if (s.mode == KAI_ST_APPLY) {
        for (int i = 0; i < a.n && !st.fault; i++) {
            const kai_op o = a.ops[i];
            const bool ok = o.kind == KAI_OP_ALLOCATE ? eng.stmt_allocate(o.pod, o.node) : o.kind == KAI_OP_PIPELINE ? eng.stmt_pipeline(o.pod, o.node, true) : eng.stmt_evict(o.pod);
            if (!ok) eng.fault(FAULT_INTERNAL);  // (the validation walk passed: the engine's own state disagrees with the pod states)
        }
    } else if (s.mode == KAI_ST_ROLLBACK) { unstamp(s.cp, s.len); eng.rollback(s.cp); }
    else if (s.mode == KAI_ST_DISCARD) { unstamp(0, s.len); eng.discard(); }
    else { unstamp(0, s.len); eng.commit(true); }
    a.head->fault = st.fault; a.head->fault_line = st.fault_line;
    if (!st.fault) a.head->applied = KAI_APPLY_PATH_ENGINE;
}

// The calls' control flow, written once against a Launcher (kai_core.hip StLauncher: HIP launches on the session's stream; tests/host_sim/stmt_sim.cpp: the lock-step
// emulator):  void check(grid, lanes, c, s.a), void apply / undo / commit(grid, lanes, c, s), int engine(c, s), int read_head(OaHead&, s.a)  (synchronises).
// st_apply_drive is oa_drive with the Statement's kernels: KAI_OK: `path` took the batch (KAI_APPLY_CHECK_ONLY: would take it); KAI_ERR_STATE: hv.bad is the first
// operation whose precondition fails, nothing was written.
template <class L>
int st_apply_drive(L& l, const KaiCtx& c, const StArgs& s, int lanes, OaHead& hv, int& path) {
    const OaArgs& a = s.a;
    path = KAI_APPLY_PATH_NONE;
    const int grid = (int)(((int64_t)a.n + lanes - 1) / lanes);
    l.check(grid, lanes, c, a);
    l.apply(grid, lanes, c, s);  // leaves at once unless the check's verdict lets it write
    if (int rc = l.read_head(hv, a)) return rc;
    const bool check_only = (a.flags & KAI_APPLY_CHECK_ONLY) != 0;
    if (!hv.dup && hv.bad != KAI_OA_NONE) return KAI_ERR_STATE;
    const bool engine = (a.flags & (KAI_APPLY_ENGINE_PATH | KAI_OA_NOT_WIDE)) || hv.dup || hv.not_wide;
    if (engine && (!check_only || hv.dup)) {
        if (int rc = l.engine(c, s)) return rc;
        if (int rc = l.read_head(hv, a)) return rc;
        if (hv.bad != KAI_OA_NONE) return KAI_ERR_STATE;
        if (hv.fault) return KAI_ERR_DEVICE_FAULT;
    }
    path = engine ? KAI_APPLY_PATH_ENGINE : KAI_APPLY_PATH_WIDE;
    return KAI_OK;
}
// rollback, discard, commit: one launch — the chip-wide kernel over the records where the host knows them all `wide`, else the engine — and the verdict's download
template <class L>
int st_range_drive(L& l, const KaiCtx& c, const StArgs& s, int lanes, bool wide, OaHead& hv, int& path) {
    const int n = s.mode == KAI_ST_COMMIT ? s.len : s.len - s.cp;
    const int grid = (int)(((int64_t)n + lanes - 1) / lanes);
    if (wide) { if (s.mode == KAI_ST_COMMIT) l.commit(grid, lanes, c, s); else l.undo(grid, lanes, c, s); }
    else if (int rc = l.engine(c, s)) return rc;
    if (int rc = l.read_head(hv, s.a)) return rc;
    if (hv.fault) return KAI_ERR_DEVICE_FAULT;
    path = wide ? KAI_APPLY_PATH_WIDE : KAI_APPLY_PATH_ENGINE;
    return KAI_OK;
}

// Where the Statement's own device memory lies (16-byte aligned): the stamps, at an offset that depends on nothing, and the verdict of rollback / discard / commit.  Sized
// at kai_stmt_begin for the session's pods: it does not grow while the Statement is open.  (The committed operations have a buffer of their own, grown by the commit.)
struct StLayout {
    size_t stamp, head, end;
    explicit StLayout(size_t pod_cap) {
        auto al = [](size_t x) { return (x + 15) & ~(size_t)15; };
        size_t o = 0;
        stamp = o; o = al(o + pod_cap * 4);
        head = o; o += sizeof(OaHead);
        end = o;
    }
};

}  // namespace kai

#if defined(__HIPCC__)
namespace kai {
__global__ void __launch_bounds__(KAI_OA_WG) k_st_apply(KaiCtx c, StArgs s) { st_apply_body(c, s); }
__global__ void __launch_bounds__(KAI_OA_WG) k_st_undo(KaiCtx c, StArgs s) { st_undo_body(c, s); }
__global__ void __launch_bounds__(KAI_OA_WG) k_st_commit(KaiCtx c, StArgs s) { st_commit_body(c, s); }
__global__ void __launch_bounds__(64) k_st_engine(KaiCtx cv, StArgs s) {
    if (threadIdx.x == 0) {
        g_ctx = cv; g_ctx.use_index = 0; g_ctx.sg = nullptr; g_ctx.sg_wgs = 0; g_ctx.mw = nullptr; g_ctx.mw_rank = 0; g_ctx.mw_world = 1;
        if (s.mode == KAI_ST_COMMIT) { g_ctx.out_ops = s.out; g_ctx.out_cap = s.out_cap; }
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    DevBackendT<true, false> be;
    st_engine_walk(g_ctx, be, s);
}
}  // namespace kai
#endif
