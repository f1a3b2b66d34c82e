// kai_ops_apply.hpp — kai_ops_apply: committed operations (kai_op: allocate / pipeline / evict, grouped into Statements by `stmt`) taken back into the open session,
// as framework.Statement applies and commits them (framework/statement.go:63-126, 197-358, 536-575).
//
//   k_oa_check   a thread per operation, chip-wide, writes no session state: the operation's precondition against the session's CURRENT state (the verdict for a
//                batch that names every pod once), whether the chip-wide path takes its start state, and whether its pod is named more than once — a per-pod
//                stamp in the handle's scratch, counted up with an atomic; the lowest offending index through an atomic minimum.
//   k_oa_wide    the chip-wide path, a thread per operation; it reads the check's verdict and does nothing but clear the stamps it touched unless the batch is
//                valid, names every pod once and starts from states this path takes.  Then: pod state, node accounting with f64 atomics, pod-set and job counters,
//                the proportion event handlers up the queue chain — modelled on kb_apply_jobs (kai_batch_kernels.hpp), and exact for the same reason: the
//                session's quantities add exactly in any order (HostPrep::batch_units, KaiCtx::exact_sums).  The inner queue nodes are summed per workgroup in
//                LDS first, as there: the few top-level queues would take an atomic per operation on one cache line.
//   k_oa_engine  everything else (a pod evicted and pipelined again in one call, a Releasing pod pipelined, a forced A/B run): ONE lane walks the batch.  First
//                over a shadow of (status, node) in scratch, so that a batch with an operation whose precondition fails writes nothing; then through the engine's
//                own stmt_allocate / stmt_pipeline / stmt_evict and commit, one Statement per run of equal `stmt`, in the victim-search instantiation (a pod that
//                lives on two nodes needs its second-residency table).  The context it runs on has use_index = 0: the class index is rebuilt by the next action
//                (kai_core.hip sets index_stale after either path), so the walk needs no service waves.
//
// No kernel waits on another workgroup; every loop is bounded by n_ops or by the height of the queue tree.
//
// What the paths leave beside the three read-backs, as the engine's Statement code leaves it: p_on_node / p_on_node_status / p_accepted / p_virtual, the pod-set
// counters (s_active_alloc, s_active_used, s_alive, s_pipelined), j_n_pending, j_allocated, j_tta_valid = 0.  Not kept: the job-order tree's QF_VALID flags (k_leaf_init
// rewrites every node at the start of every action) and the engine's kept pre-order range and best nodes (EngineLocal: they live for one kernel).
//
// The bodies are written against kai_simt.hpp, so that tests/host_sim/ops_apply_sim.cpp runs them with emulated lanes on a machine without a GPU.
#pragma once
#include "kai_engine.hpp"
#include "kai_simt.hpp"
#include "kai_batch_kernels.hpp"

namespace kai {

constexpr int KAI_OA_WG = 256;               // lanes of a workgroup of k_oa_check / k_oa_wide
constexpr int32_t KAI_OA_NONE = 0x7fffffff;  // OaHead::bad: no offending operation
constexpr uint32_t KAI_OA_NOT_WIDE = 0x100u; // OaArgs::flags, set by the host: the session does not qualify for the chip-wide path

// the call's verdict: sent with the operations (bad = KAI_OA_NONE, the rest 0), read back after the launches
struct OaHead {
    int32_t bad;        // lowest index of an operation whose precondition fails (the check: against the current state; the engine walk: in sequence)
    int32_t dup;        // a pod is named more than once: the check's verdict does not hold, the engine walk decides
    int32_t not_wide;   // an operation starts from a state the chip-wide path does not take
    int32_t applied;    // KAI_APPLY_PATH_WIDE / KAI_APPLY_PATH_ENGINE: that path wrote the batch (diagnostics)
    int32_t fault, fault_line, pad[10];
};
static_assert(sizeof(OaHead) == 64, "OaHead is one 64-byte record in front of the staged operations");

struct OaArgs {
    int32_t n; uint32_t flags; int32_t use_islot, pad;  // use_islot: the batch path's tables are bound (BatchCtx::q_islot, h_nodes): inner queue nodes through LDS
    KAI_GP(const kai_op) ops;    // [n] node = name rank
    KAI_GP(OaHead) head;
    KAI_GP(int32_t) stamp;       // [P] times the pod is named by the running call; zero between calls
    KAI_GP(int32_t) sh_status;   // [P] the validation walk's shadow status, 0 = the session's own; zero between calls
    KAI_GP(int32_t) sh_node;     // [P] ... and node
};

constexpr int32_t KAI_OA_PLACED = KAI_POD_ALLOCATED | KAI_POD_BINDING | KAI_POD_BOUND | KAI_POD_RUNNING;  // what the chip-wide path evicts

KAI_HD bool oa_pre_ok(int kind, int status, int node, int op_node) {
    if (kind == KAI_OP_ALLOCATE) return status == KAI_POD_PENDING;
    if (kind == KAI_OP_PIPELINE) return status == KAI_POD_PENDING || status == KAI_POD_RELEASING;
    return node >= 0 && node == op_node;  // the reference evicts Pipelined and already Releasing pods too: "has a node", not "is running"
}

KW_BODY void oa_check_body(const KaiCtx& c, const OaArgs& a) {
    const int64_t i = (int64_t)kw::bid() * kw::bdim() + kw::tid();
    if (i >= a.n) return;
    const kai_op o = a.ops[i];
    const int st = c.p_status[o.pod], nd = c.p_node[o.pod];
    if (kw::atomic_add((int32_t*)&a.stamp[o.pod], 1) != 0) a.head->dup = 1;  // (every writer stores the same value)
    if (!oa_pre_ok(o.kind, st, nd, o.node)) kw::atomic_min((int32_t*)&a.head->bad, (int)i);
    const bool wide = o.kind == KAI_OP_EVICT ? ((st & KAI_OA_PLACED) != 0 && c.p_on_node[o.pod] == nd && (c.p_on_node_status[o.pod] & KAI_OA_PLACED) != 0)
                                             : (st == KAI_POD_PENDING && c.p_on_node[o.pod] < 0);
    if (!wide) a.head->not_wide = 1;
}

KW_BODY void oa_wide_body(const KaiCtx& c, const OaArgs& a) {
    KW_SHARED double s_acc[KB_APPLY_INNER * 6];  // per inner queue node: allocated [3], allocated_np [3]
    const int tid = kw::tid(), T = kw::bdim();
    const int64_t i = (int64_t)kw::bid() * T + tid;
    // the same for every lane of the grid: the check kernel finished before this one started
    const bool go = a.head->bad == KAI_OA_NONE && !a.head->dup && !a.head->not_wide && !(a.flags & (KAI_APPLY_CHECK_ONLY | KAI_APPLY_ENGINE_PATH | KAI_OA_NOT_WIDE));
    const BatchCtx& b = c.bt;
    const int n_in = (go && a.use_islot) ? (b.n_inner < KB_APPLY_INNER ? b.n_inner : KB_APPLY_INNER) : 0;
    for (int k = tid; k < n_in * 6; k += T) s_acc[k] = 0.0;
    kw::sync();
    if (i < a.n) {
        const kai_op o = a.ops[i];
        const int p = o.pod;
        a.stamp[p] = 0;  // only the touched entries are cleaned
        if (go) {
            const int n = o.node, j = c.p_job[p], s = c.p_podset[p];
            const double q3[3] = {c.p_req[(size_t)KAI_RES_CPU * c.P + p], c.p_req[(size_t)KAI_RES_MEM * c.P + p], c.p_req[(size_t)KAI_RES_GPU * c.P + p]};
            double sign = 1.0;
            c.p_accepted[p] = 1; c.j_tta_valid[j] = 0;
            if (o.kind == KAI_OP_ALLOCATE) {  // Statement.Allocate, then BindPod at the commit: Pending -> Allocated -> Binding
                c.p_status[p] = KAI_POD_BINDING; c.p_node[p] = n; c.p_on_node[p] = n; c.p_on_node_status[p] = KAI_POD_ALLOCATED; c.p_virtual[p] = 1;
                for (int r = 0; r < c.R; r++) {
                    const double v = c.p_req[(size_t)r * c.P + p]; if (v == 0) continue;
                    kw::atomic_add((double*)&c.n_used[(size_t)r * c.N + n], v); kw::atomic_add((double*)&c.n_idle[(size_t)r * c.N + n], -v);
                }
                kw::atomic_add((int32_t*)&c.s_active_alloc[s], 1); kw::atomic_add((int32_t*)&c.s_active_used[s], 1); kw::atomic_add((int32_t*)&c.j_n_pending[j], -1);
                for (int k = 0; k < 3; k++) if (q3[k] != 0) kw::atomic_add((double*)&c.j_allocated[(size_t)j * 4 + k], q3[k]);
            } else if (o.kind == KAI_OP_PIPELINE) {  // Pending -> Pipelined: the node's Releasing pays for it
                c.p_status[p] = KAI_POD_PIPELINED; c.p_node[p] = n; c.p_on_node[p] = n; c.p_on_node_status[p] = KAI_POD_PIPELINED; c.p_virtual[p] = 1;
                for (int r = 0; r < c.R; r++) {
                    const double v = c.p_req[(size_t)r * c.P + p]; if (v == 0) continue;
                    kw::atomic_add((double*)&c.n_used[(size_t)r * c.N + n], v); kw::atomic_add((double*)&c.n_rel[(size_t)r * c.N + n], -v);
                }
                kw::atomic_add((int32_t*)&c.s_active_alloc[s], 1); kw::atomic_add((int32_t*)&c.s_active_used[s], 1); kw::atomic_add((int32_t*)&c.s_pipelined[s], 1);
                kw::atomic_add((int32_t*)&c.j_n_pending[j], -1);
            } else {  // placed -> Releasing on its node: the node's copy is removed and added again, which leaves Idle and Used as they were
                c.p_status[p] = KAI_POD_RELEASING; c.p_on_node_status[p] = KAI_POD_RELEASING; c.p_virtual[p] = 0;
                for (int r = 0; r < c.R; r++) {
                    const double v = c.p_req[(size_t)r * c.P + p]; if (v == 0) continue;
                    kw::atomic_add((double*)&c.n_rel[(size_t)r * c.N + n], v);
                }
                kw::atomic_add((int32_t*)&c.s_active_alloc[s], -1); kw::atomic_add((int32_t*)&c.s_alive[s], -1);
                for (int k = 0; k < 3; k++) if (q3[k] != 0) kw::atomic_add((double*)&c.j_allocated[(size_t)j * 4 + k], -q3[k]);
                sign = -1.0;
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
    }
    kw::sync();
    for (int k = tid; k < n_in * 6; k += T) {
        const double v = s_acc[k]; if (v == 0) continue;
        const int q = b.h_nodes[b.h_off[1] + k / 6], r = k % 3;
        if (k % 6 < 3) kw::atomic_add((double*)&c.q_share[(size_t)q * 3 + r].allocated, v); else kw::atomic_add((double*)&c.q_share[(size_t)q * 3 + r].allocated_np, v);
    }
    if (go && i == 0) a.head->applied = KAI_APPLY_PATH_WIDE;
}

// The engine walk, by ONE lane (the device: lane 0 of k_oa_engine's only workgroup).  c.use_index is 0: node_apply's mark_dirty stops before the class index.
template <class Backend>
KAI_HD void oa_engine_walk(const KaiCtx& c, Backend& be, const OaArgs& a) {
    // ---- the validation walk: every operation against the state its predecessors leave, on a shadow; the touched entries are cleaned before anything else happens
    int bad = KAI_OA_NONE;
    for (int i = 0; i < a.n; i++) {
        const kai_op o = a.ops[i];
        const bool own = a.sh_status[o.pod] != 0;
        int st = own ? a.sh_status[o.pod] : c.p_status[o.pod], nd = own ? a.sh_node[o.pod] : c.p_node[o.pod];
        if (!oa_pre_ok(o.kind, st, nd, o.node)) { bad = i; break; }
        if (o.kind == KAI_OP_ALLOCATE) { st = KAI_POD_ALLOCATED; nd = o.node; } else if (o.kind == KAI_OP_PIPELINE) { st = KAI_POD_PIPELINED; nd = o.node; } else st = KAI_POD_RELEASING;
        a.sh_status[o.pod] = st; a.sh_node[o.pod] = nd;
    }
    for (int i = 0; i < a.n; i++) a.sh_status[a.ops[i].pod] = 0;
    a.head->bad = bad;  // (with a pod named twice the check kernel's verdict was only a guess)
    if (bad != KAI_OA_NONE || (a.flags & KAI_APPLY_CHECK_ONLY)) return;
    // ---- the Statements
    Engine<Backend> eng(c, be);
    EngineState& st = *c.st;
    st.ops_len = 0; st.n_undo = 0; st.fault = 0; st.fault_line = 0;
    const int lim = c.ops_cap - 2;  // a longer Statement is committed in pieces: the commit only moves Allocated to Binding, which no later operation tells apart
    eng.el().h.out_len = 0; eng.el().h.stmts = 0;
    auto commit = [&] { eng.commit(false); };  // (nothing is handed back: the operations came from the caller)
    int cur = a.ops[0].stmt;
    for (int i = 0; i < a.n && !st.fault; i++) {
        const kai_op o = a.ops[i];
        if (o.stmt != cur || st.ops_len >= lim) { commit(); cur = o.stmt; }
        const bool ok = o.kind == KAI_OP_ALLOCATE ? eng.stmt_allocate(o.pod, o.node) : o.kind == KAI_OP_PIPELINE ? eng.stmt_pipeline(o.pod, o.node, true) : eng.stmt_evict(o.pod);
        if (!ok) eng.fault(FAULT_INTERNAL);  // (the validation walk passed: the engine's own state disagrees with the pod states)
    }
    if (!st.fault) commit();
    a.head->fault = st.fault; a.head->fault_line = st.fault_line;
    if (!st.fault) a.head->applied = KAI_APPLY_PATH_ENGINE;
}

// The call's control flow, written once against a Launcher (kai_core.hip OaLauncher: HIP launches on the session's stream; tests/host_sim/ops_apply_sim.cpp: the lock-step emulator):
//   void check(grid, lanes, c, a), void wide(grid, lanes, c, a), int engine(c, a), int read_head(OaHead&, a)  (synchronises).
// KAI_OK: `path` took the batch (KAI_APPLY_CHECK_ONLY: would take it).  KAI_ERR_STATE: hv.bad is the first operation whose precondition fails; nothing was written.
template <class L>
int oa_drive(L& l, const KaiCtx& c, const OaArgs& a, int lanes, OaHead& hv, int& path) {
    path = KAI_APPLY_PATH_NONE;
    const int grid = (int)(((int64_t)a.n + lanes - 1) / lanes);
    l.check(grid, lanes, c, a);
    l.wide(grid, lanes, c, a);  // leaves at once unless the check's verdict lets it write
    if (int rc = l.read_head(hv, a)) return rc;
    const bool check_only = (a.flags & KAI_APPLY_CHECK_ONLY) != 0;
    if (!hv.dup && hv.bad != KAI_OA_NONE) return KAI_ERR_STATE;
    const bool engine = (a.flags & (KAI_APPLY_ENGINE_PATH | KAI_OA_NOT_WIDE)) || hv.dup || hv.not_wide;
    if (engine && (!check_only || hv.dup)) {  // (a check-only call needs the walk only where a pod is named twice: its shadow decides)
        if (int rc = l.engine(c, a)) return rc;
        if (int rc = l.read_head(hv, a)) return rc;
        if (hv.bad != KAI_OA_NONE) return KAI_ERR_STATE;
        if (hv.fault) return KAI_ERR_DEVICE_FAULT;
    }
    path = engine ? KAI_APPLY_PATH_ENGINE : KAI_APPLY_PATH_WIDE;
    return KAI_OK;
}
// the session qualifies for the chip-wide path as it does for the batch path's apply: quantities that add exactly in any order, no MIG rows, no shared GPUs
inline bool oa_wide_session(const KaiCtx& c) { return c.exact_sums && c.R <= 4 && !c.mig_on && !c.quota_on && !c.shared_on; }
inline int oa_use_islot(const KaiCtx& c) { return (c.bt.enabled && c.bt.q_islot && c.bt.h_nodes && c.bt.h_off && c.bt.n_inner > 0) ? 1 : 0; }

// Where the pieces of one call lie in the handle's scratch (device) and staging (pinned host), 16-byte aligned.  The per-pod arrays come first, at offsets that depend
// on the scratch's pod capacity only: they are zero between calls and stay where they are while the scratch is large enough.  [head | ops] is what every call sends.
struct OaLayout {
    size_t stamp, sh_status, sh_node, head, ops, end;
    OaLayout(size_t pod_cap, int64_t n) {
        auto al = [](size_t x) { return (x + 15) & ~(size_t)15; };
        size_t o = 0;
        stamp = o; o = al(o + pod_cap * 4);
        sh_status = o; o = al(o + pod_cap * 4);
        sh_node = o; o = al(o + pod_cap * 4);
        head = o; o += sizeof(OaHead);
        ops = o; o = al(o + (size_t)n * sizeof(kai_op));
        end = o;
    }
};

}  // namespace kai

#if defined(__HIPCC__)
#include "kai_kernels.hpp"  // the action kernel's LDS objects (g_ctx, g_el, g_eb) and DevBackendT
namespace kai {
__global__ void __launch_bounds__(KAI_OA_WG) k_oa_check(KaiCtx c, OaArgs a) { oa_check_body(c, a); }
__global__ void __launch_bounds__(KAI_OA_WG) k_oa_wide(KaiCtx c, OaArgs a) { oa_wide_body(c, a); }
__global__ void __launch_bounds__(64) k_oa_engine(KaiCtx cv, OaArgs a) {
    if (threadIdx.x == 0) { g_ctx = cv; g_ctx.use_index = 0; g_ctx.sg = nullptr; g_ctx.sg_wgs = 0; g_ctx.mw = nullptr; g_ctx.mw_rank = 0; g_ctx.mw_world = 1; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    DevBackendT<true, false> be;
    oa_engine_walk(g_ctx, be, a);
}
}  // namespace kai
#endif
