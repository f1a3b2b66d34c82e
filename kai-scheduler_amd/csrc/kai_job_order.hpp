// kai_job_order.hpp — kai_job_order: the pop order of a JobsOrderByQueues over the session's CURRENT state (plugins/reflectjoborder/reflect_job_order.go:41-66: FilterNonPending,
// FilterUnready, the allocate action's queue depth, popped until empty without allocating anything), and every job's place in it and in its own leaf queue.
//
// The common front is the allocate action's init at the current state (k_job_init, k_leaf_init of kai_open_kernels.hpp, unchanged) on a copy of the context whose action is
// "allocate" and whose queue depth is the call's, then
//   k_jo_qualify    a thread per job: both position arrays to -1; the queued jobs counted, and among them the ones the chip-wide path cannot order (a job in another elastic
//                   state than "below minAvailable": the leaf's side heap; a job without a valid tasks-to-allocate chunk), one atomic per wavefront.
// CHIP-WIDE PATH.  Nothing is allocated between two pops, so no queue's shares change: the plan of kai_batch.hpp in the special case of constant shares — one pass over the
// whole queue, no capacity gate, no fit prediction, no rounds.  The static sibling order (k_batch_static_rank / _check), the regions of every queue node in the pools
// (k_plan_setup, a leaf offering min(depth, what it holds)) and the merge (k_plan_rank) are the plan's own kernels, unchanged, on a context whose BatchCtx points into the handle's
// scratch.  New here, order only:
//   k_jo_leaf       a wavefront per leaf: the key the leaf competes with before each of its pops (plan_key_c over the leaf's shares as they stand and the job's
//                   tasks-to-allocate resources), as a running maximum.
//   k_jo_keys       per tree height, a thread per position of the height's merged streams, chip-wide: the stale-path job the node's key is read through before that pop (the
//                   reference's lazy reorder, getBestJobFromNode job_order_by_queue.go:309-318 with Fix(0) deferred :194-217, as kb_plan_gather finds it) and the key — the six
//                   f64 divisions per key are the cost, and with constant shares no position depends on another.
//   k_jo_scan       a workgroup per queue node of the height: what is left of kb_plan_scan, a running maximum of 32-byte keys along the node's stream, in place, in tiles of
//                   bdim x KB_PLAN_SCAN_ELEMS positions with a carry (config 5's 38 k-position streams: ten tiles of 4 096).
//   k_jo_emit       a thread per position of the virtual root's stream: the job, its position, and its position in its leaf's stream (the leaf element's index: no second pass).
// ENGINE PATH.  k_jo_engine: one lane walks the engine's own job-order tree (Engine::init_jobs_order, pop_next_job: container/heap's sift rules, the lazy reorder, truncate_leaf,
// the side heaps) until it is empty.  No allocation attempt, no Statement, no statistics.  The fallback and the A/B partner.
//
// What the call writes of the session are arrays every action's own init writes again before anything reads them: j_state, the tasks-to-allocate caches (tta, j_tta_n,
// j_tta_res, j_tta_valid: rebuilt only where invalid, from the state as it stands), lq_sorted / lq_cur / lq_end / lq_side / lq_side_len, qn, qheap, root_heap.
// No kernel waits on another workgroup; every loop is bounded by a leaf's jobs, a node's stream, a node's children or the jobs of the session.
// The bodies are written against kai_simt.hpp: tests/host_sim/job_order_sim.cpp runs them and jo_drive with emulated lanes.
#pragma once
#include <algorithm>

#include "kai_batch_kernels.hpp"
#include "kai_host_prep.hpp"
#include "kai_open_kernels.hpp"

namespace kai {

constexpr int KAI_JO_WG = 256;  // lanes of a workgroup of the per-item kernels (the emulator also runs them with 100 and 1)

// the call's verdicts and counts: sent zeroed in front of the tree tables, read back behind the qualification and again with the order.  The first four words are what
// BatchCtx::qual points at (k_batch_static_rank / _check count sibling sets without a strict static order in word 1)
struct JoHead { int32_t irregular, order_bad, queued, pad0, n_ordered, n_leaves, fault, fault_line, pad[8]; };
static_assert(sizeof(JoHead) == 64, "JoHead is one 64-byte record in front of the tree tables");
enum : int32_t { JO_FAULT_STREAM = 1, JO_FAULT_ENGINE = 2 };  // a merged stream that is no permutation of its children's keys; the engine's own fault (fault_line: its source line)

struct JoArgs {
    int32_t J, pool_e, pool_k, pad;
    KAI_GP(JoHead) head;
    KAI_GP(int32_t) order;    // [J] job indices in pop order
    KAI_GP(int32_t) pos;      // [J] position in `order`, -1 = not in it
    KAI_GP(int32_t) qpos;     // [J] position among the jobs of the job's own leaf queue, -1 = not in the order
    KAI_GP(int32_t) q_taken;  // [Q+1] engine path: jobs popped from the leaf so far
};

// Where the pieces lie in the handle's scratch, 16-byte aligned, for the session's J jobs, Q queues and tree heights and pools of `pool` slots.  [head | q_height | h_off |
// h_nodes] is what every call sends (up_end bytes), [the same | order | pos | qpos] what it reads back in one piece (down_end bytes, or less where the caller wants no positions).
struct JoLayout {
    size_t head, q_height, h_off, h_nodes, up_end, order, pos, qpos, down_end, q_srank, cur_sp, q_cnt, q_ebase, q_kbase, q_valid, q_nk, q_sent, q_taken, q_complete, plan_tot,
           pk, sp, k_owner, el_leaf, el_ck, el_next, e_job, end;
    JoLayout(size_t J, size_t Q, size_t n_heights, size_t pool) {
        auto al = [](size_t x) { return (x + 15) & ~(size_t)15; };
        size_t o = 0;
        head = o; o += sizeof(JoHead);
        q_height = o; o += (Q + 1) * 4; h_off = o; o += (n_heights + 1) * 4; h_nodes = o; o += (Q + 1) * 4; o = al(o); up_end = o;
        order = o; o = al(o + J * 4); pos = o; o = al(o + J * 4); qpos = o; o = al(o + J * 4); down_end = o;
        q_srank = o; o = al(o + (Q + 1) * 4); cur_sp = o; o = al(o + (Q + 1) * 4);
        q_cnt = o; o = al(o + (Q + 1) * 4); q_ebase = o; o = al(o + (Q + 1) * 4); q_kbase = o; o = al(o + (Q + 1) * 4); q_valid = o; o = al(o + (Q + 1) * 4);
        q_nk = o; o = al(o + (Q + 1) * 4); q_sent = o; o = al(o + (Q + 1) * 4); q_taken = o; o = al(o + (Q + 1) * 4); q_complete = o; o = al(o + Q + 1);
        plan_tot = o; o = al(o + 8);
        pk = o; o = al(o + pool * sizeof(PlanKey)); sp = o; o = al(o + pool * 4); k_owner = o; o = al(o + pool * 4);
        el_leaf = o; o = al(o + pool * 4); el_ck = o; o = al(o + pool * 4); el_next = o; o = al(o + pool); e_job = o; o = al(o + pool * 4);
        end = o;
    }
};
// the pools of a session of J jobs and Q queues in a tree of n_heights heights (the virtual root's included): what batch_bind gives the plan
inline size_t jo_pool(int J, int Q, int n_heights) { return (size_t)J * (size_t)n_heights + 2 * (size_t)Q + 64; }

// the context the call's kernels get: the session's, with the allocate action's filters, the call's queue depth and a BatchCtx in the handle's scratch at `d`
inline KaiCtx jo_bind_ctx(const KaiCtx& c, unsigned char* d, const JoLayout& L, int n_heights, size_t pool, int queue_depth) {
    KaiCtx cj = c;
    cj.action = KAI_ACTION_ALLOCATE; cj.queue_depth = queue_depth;
    BatchCtx b{};
    b.enabled = 1; b.n_h = n_heights; b.pool_e = (int32_t)pool; b.pool_k = (int32_t)pool; b.world = 1; b.n_hi = c.N;
#define JO_B(field) b.field = (decltype(b.field))(d + L.field)
    JO_B(q_height); JO_B(h_off); JO_B(h_nodes); JO_B(q_srank); JO_B(cur_sp);
    JO_B(q_cnt); JO_B(q_ebase); JO_B(q_kbase); JO_B(q_valid); JO_B(q_nk); JO_B(q_sent); JO_B(q_taken); JO_B(q_complete); JO_B(plan_tot);
    JO_B(pk); JO_B(sp); JO_B(k_owner); JO_B(el_leaf); JO_B(el_ck); JO_B(el_next); JO_B(e_job);
#undef JO_B
    b.qual = (decltype(b.qual))(d + L.head);
    cj.bt = b;
    return cj;
}
inline JoArgs jo_bind_args(const KaiCtx& c, unsigned char* d, const JoLayout& L, size_t pool) {
    JoArgs a{};
    a.J = c.J; a.pool_e = (int32_t)pool; a.pool_k = (int32_t)pool;
    a.head = (KAI_GP(JoHead))(d + L.head); a.order = (KAI_GP(int32_t))(d + L.order); a.pos = (KAI_GP(int32_t))(d + L.pos); a.qpos = (KAI_GP(int32_t))(d + L.qpos);
    a.q_taken = (KAI_GP(int32_t))(d + L.q_taken);
    return a;
}

KW_BODY void jo_qualify_body(const KaiCtx& c, const JoArgs& a) {
    const int64_t j = (int64_t)kw::bid() * kw::bdim() + kw::tid();
    bool queued = false, irregular = false;
    if (j < c.J) {
        a.pos[j] = -1; a.qpos[j] = -1;
        const int st = c.j_state[j];
        queued = st != 3;
        irregular = queued && (st != 0 || !c.j_tta_valid[j]);
    }
    const uint64_t mq = kw::ballot(queued), mi = kw::ballot(irregular);
    if (kw::lane() == 0) {  // (no lane left before the ballots: lane 0 is there)
        if (mq) kw::atomic_add((int32_t*)&a.head->queued, __builtin_popcountll(mq));
        if (mi) kw::atomic_add((int32_t*)&a.head->irregular, __builtin_popcountll(mi));
    }
}

// One wavefront per leaf queue: the leaf's jobs in JobOrderFn order (k_leaf_init's sorted region, the first q_cnt of them: the queue depth), the key before each pop.  The
// queue, and so the trip count of the loop with the scans, is the wavefront's.
KW_BODY void jo_leaf_body(const KaiCtx& c, const JoArgs& a) {
    const BatchCtx& b = c.bt;
    const int q = kw::bid() * (kw::bdim() >> 6) + (kw::tid() >> 6), lane = kw::lane();
    if (q >= c.Q || !kb_is_leaf(c, q)) return;
    const int V = b.q_cnt[q], off = c.q_job_off[q] + c.lq_cur[q], eb = b.q_ebase[q], kb = b.q_kbase[q], srank = b.q_srank[q];
    double alloc[3];
    for (int k = 0; k < 3; k++) alloc[k] = c.q_share[(size_t)q * 3 + k].allocated;
    const PlanNodeConst nc = plan_node_const(c, q, c.st->total[0], c.st->total[1], c.st->total[2]);
    PlanKey run; run.w0 = run.w1 = run.w2 = run.w3 = 0; bool have_run = false;
    for (int base = 0; base < V; base += 64) {
        const int i = base + lane; const bool is_key = i < V;
        const int job = is_key ? c.lq_sorted[off + i] : -1;
        double res[3] = {0, 0, 0};
        if (job >= 0) for (int k = 0; k < 3; k++) res[k] = c.j_tta_res[(size_t)job * 4 + k];
        PlanKey key; key.w0 = key.w1 = key.w2 = key.w3 = 0;
        if (is_key) key = plan_key_c(nc, alloc, res, srank);
        key = kb_wave_scan_max(key, is_key, run, have_run);
        if (is_key) { b.e_job[eb + i] = job; b.pk[kb + i] = key; b.sp[kb + i] = job; b.k_owner[kb + i] = q; }
        run.w0 = kw::shfl(key.w0, 63); run.w1 = kw::shfl(key.w1, 63); run.w2 = kw::shfl(key.w2, 63); run.w3 = kw::shfl(key.w3, 63); have_run = true;
    }
    if (lane == 0) { b.q_valid[q] = V; b.q_nk[q] = V; b.q_complete[q] = 1; if (V > 0) kw::atomic_add((int32_t*)&a.head->n_leaves, 1); }
}

// One thread per position of the merged streams of the inner nodes of height rp.height (k_plan_rank wrote them): the stale-path job and the node's key before that pop.
// The node's heap top before its pop t: before the first pop its best child; after a pop from a child that still has a key, that child (its next stale-path job); else the
// child popped from is gone and the top is the best remaining child, the one position t is taken from.  Every index read out of the pools is checked before it is used.
KW_BODY void jo_keys_body(const KaiCtx& c, const JoArgs& a, RoundParams rp) {
    const BatchCtx& b = c.bt;
    const int p = kw::bid() * kw::bdim() + kw::tid();
    if (p >= b.plan_tot[0] || p >= a.pool_e) return;
    int lo = b.h_off[rp.height], hi = b.h_off[rp.height + 1];  // nodes of this height, their regions ascending in the pools
    if (lo >= hi || p < b.q_ebase[b.h_nodes[lo]]) return;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (b.q_ebase[b.h_nodes[mid]] <= p) lo = mid; else hi = mid; }
    const int x = b.h_nodes[lo], eb = b.q_ebase[x], kb = b.q_kbase[x], t = p - eb;
    if (x == c.Q || t >= b.q_cnt[x]) return;
    int slot;
    if (t > 0 && b.el_next[p - 1]) slot = b.el_ck[p - 1]; else slot = b.el_ck[p] - 1;
    const int spj = (slot >= 0 && slot < a.pool_k) ? b.sp[slot] : -1;
    if (spj < 0 || spj >= c.J || kb + t >= a.pool_k) { a.head->fault = JO_FAULT_STREAM; return; }
    double alloc[3], rq[3];
    for (int k = 0; k < 3; k++) { alloc[k] = c.q_share[(size_t)x * 3 + k].allocated; rq[k] = c.j_tta_res[(size_t)spj * 4 + k]; }
    const PlanNodeConst nc = plan_node_const(c, x, c.st->total[0], c.st->total[1], c.st->total[2]);
    b.pk[kb + t] = plan_key_c(nc, alloc, rq, b.q_srank[x]); b.sp[kb + t] = spj; b.k_owner[kb + t] = x;
}

// One workgroup per queue node of height rp.height: the running maximum of the node's keys along its stream, in place.  KB_PLAN_SCAN_ELEMS consecutive positions per
// thread and tile: a thread folds its own positions serially, the workgroup scans the threads' maxima (kb_block_excl_max), the tile's last maximum is the next tile's carry.
KW_BODY void jo_scan_body(const KaiCtx& c, RoundParams rp) {
    const BatchCtx& b = c.bt;
    KW_SHARED PlanScanLds L;
    constexpr int E = KB_PLAN_SCAN_ELEMS;
    const int idx = b.h_off[rp.height] + kw::bid(), tid = kw::tid(), T = kw::bdim();
    if (idx >= b.h_off[rp.height + 1]) return;  // the same for the whole workgroup
    const int x = b.h_nodes[idx];
    if (x == c.Q) return;
    const int V = b.q_cnt[x], kb = b.q_kbase[x];
    PlanKey run; run.w0 = run.w1 = run.w2 = run.w3 = 0; bool have_run = false;
    for (int base = 0; base < V; base += T * E) {  // (the same trip count in every lane)
        const int t0 = base + tid * E;
        PlanKey key[E]; PlanKey tm; tm.w0 = tm.w1 = tm.w2 = tm.w3 = 0; bool tmv = false;
        for (int j = 0; j < E; j++) {
            key[j].w0 = key[j].w1 = key[j].w2 = key[j].w3 = 0;
            if (t0 + j < V) {
                key[j] = b.pk[kb + t0 + j];
                if (tmv && pk_less(key[j], tm)) key[j] = tm;  // running maximum inside the thread
                tm = key[j]; tmv = true;
            }
        }
        PlanKey pm, last; bool have_pm, have_last;
        kb_block_excl_max(L, tm, tmv, run, have_run, pm, have_pm, last, have_last);
        for (int j = 0; j < E; j++) if (t0 + j < V) { PlanKey out = key[j]; if (have_pm && pk_less(out, pm)) out = pm; b.pk[kb + t0 + j] = out; }
        run = last; have_run = have_last;
    }
    if (tid == 0) { b.q_valid[x] = V; b.q_nk[x] = V; b.q_complete[x] = 1; }
}

// the order: one thread per position of the virtual root's stream
KW_BODY void jo_emit_body(const KaiCtx& c, const JoArgs& a) {
    const BatchCtx& b = c.bt;
    const int t = kw::bid() * kw::bdim() + kw::tid(), n = b.q_cnt[c.Q];
    if (t == 0) a.head->n_ordered = n;
    if (t >= n || t >= a.J) return;
    const int ep = b.q_ebase[c.Q] + t;
    const int e = ep < a.pool_e ? b.el_leaf[ep] : -1;
    const int job = (e >= 0 && e < a.pool_e) ? b.e_job[e] : -1;
    if (job < 0 || job >= c.J) { a.head->fault = JO_FAULT_STREAM; a.order[t] = -1; return; }
    a.order[t] = job; a.pos[job] = t; a.qpos[job] = e - b.q_ebase[c.j_queue[job]];
}

// The engine walk, by ONE lane (the device: lane 0 of k_jo_engine's only workgroup): the job-order tree of the allocate action, popped until it is empty.  c.use_index is 0:
// pop_next_job stages nothing.  The engine's fault word is the session's: it leaves as it came.
template <class Backend>
KAI_HD void jo_engine_walk(const KaiCtx& c, Backend& be, const JoArgs& a) {
    Engine<Backend> eng(c, be);
    EngineState& st = *c.st;
    const int fault0 = st.fault, line0 = st.fault_line;
    st.fault = 0; st.fault_line = 0;
    for (int q = 0; q <= c.Q; q++) a.q_taken[q] = 0;
    eng.init_jobs_order();
    int leaves = 0;
    for (int q = 0; q < c.Q; q++) if (eng.q_is_leaf(q) && eng.qnp()[q].len > 0) leaves++;
    int n = 0;
    while (n < a.J && !st.fault) {  // (nothing is pushed back: a job is popped once)
        const int j = eng.pop_next_job();
        if (j < 0) break;
        a.order[n] = j; a.pos[j] = n; a.qpos[j] = a.q_taken[c.j_queue[j]]++;
        n++;
    }
    a.head->n_ordered = n; a.head->n_leaves = leaves;
    if (st.fault) { a.head->fault = JO_FAULT_ENGINE; a.head->fault_line = st.fault_line; }
    st.fault = fault0; st.fault_line = line0;
}

// what the host can tell of the session before any launch: the chip-wide path orders queues by the proportion plugin's comparator, in a tree of at most 16 levels, in pools
// whose indices fit an int32
inline bool jo_wide_session(const KaiCtx& c, int n_heights, size_t pool) { return (c.plugins & KAI_PLUGIN_PROPORTION) && n_heights <= 17 && pool < ((size_t)1 << 30); }

// The call's control flow from its first launch on, written once against a Launcher (kai_core.hip JoLauncher: HIP launches on the session's stream; tests/host_sim/job_order_sim.cpp:
// the lock-step emulator):
//   void job_init / leaf_init / static_rank / static_check(grid, lanes, cj),  void qualify / leaf / emit(grid, lanes, cj, a),  void plan_setup / plan_rank / scan(grid, lanes, cj, rp),
//   void keys(grid, lanes, cj, a, rp),  int engine(cj, a),  int read_head(JoHead&, a)  (synchronises).
// cj: jo_bind_ctx's context; depth: jobs a leaf offers, 0 = all; shape: the queue tree's (HostPrep::BatchShape).  KAI_OK: hd holds the counts, `path` the path that ordered.
template <class L>
int jo_drive(L& l, const KaiCtx& cj, const JoArgs& a, const HostPrep::BatchShape& shape, bool wide_session, int depth, uint32_t flags, int lanes, JoHead& hd, int& path) {
    path = KAI_JOB_ORDER_PATH_NONE;
    const int J = cj.J, Q = cj.Q, TB = OPEN_TB;
    // ---- the common front: the allocate action's init at the current state
    if (J) l.job_init((J + TB - 1) / TB, TB, cj);
    if (Q) l.leaf_init((Q + 3) / 4, TB, cj);
    if (J) l.qualify((int)(((int64_t)J + lanes - 1) / lanes), lanes, cj, a);
    const bool try_wide = wide_session && !(flags & KAI_JOB_ORDER_ENGINE_PATH);
    if (try_wide && Q) { l.static_rank((Q + lanes - 1) / lanes, lanes, cj); l.static_check((Q + lanes - 1) / lanes, lanes, cj); }
    if (int rc = l.read_head(hd, a)) return rc;
    if (hd.queued == 0) return KAI_OK;
    if (!try_wide || hd.irregular || hd.order_bad) {
        if (int rc = l.engine(cj, a)) return rc;
        if (int rc = l.read_head(hd, a)) return rc;
        if (hd.fault) return KAI_ERR_DEVICE_FAULT;
        path = KAI_JOB_ORDER_PATH_ENGINE;
        return KAI_OK;
    }
    // ---- the plan with constant shares: one pass, every leaf offers all it holds up to the depth
    RoundParams rp{}; rp.h_leaf = depth > 0 ? depth : KB_INF;
    const int64_t e_bound = depth > 0 ? std::min<int64_t>(hd.queued, (int64_t)shape.n_leaves * depth) : hd.queued;
    const int64_t slots = std::min<int64_t>(a.pool_k, e_bound * shape.n_heights + 2 * (int64_t)Q + 2);  // element and key slots the regions can take
    rp.n_slots = (int32_t)slots;
    const int slot_grid = std::max(1, (int)((slots + lanes - 1) / lanes));
    l.plan_setup(1, KB_PLAN_SETUP_THREADS, cj, rp);
    l.leaf((Q + 3) / 4, 256, cj, a);
    for (int h = 1; h < shape.n_heights; h++) {
        rp.height = h;
        l.plan_rank(slot_grid, lanes, cj, rp);
        if (h + 1 == shape.n_heights) break;  // (the virtual root's stream is the order: it competes with nobody)
        l.keys(slot_grid, lanes, cj, a, rp);
        const int64_t per_node = e_bound / std::max(shape.h_count[h], 1);
        const int scan_tb = std::min(KB_PLAN_SCAN_THREADS, per_node >= 8192 ? 1024 : per_node >= 1024 ? 512 : per_node >= 192 ? 128 : 64);
        l.scan(std::max(shape.h_count[h], 1), scan_tb, cj, rp);
    }
    l.emit(std::max(1, (int)((e_bound + lanes - 1) / lanes)), lanes, cj, a);
    if (int rc = l.read_head(hd, a)) return rc;
    if (hd.fault) return KAI_ERR_DEVICE_FAULT;
    path = KAI_JOB_ORDER_PATH_WIDE;
    return KAI_OK;
}

}  // namespace kai

#if defined(__HIPCC__)
#include "kai_kernels.hpp"  // the action kernel's LDS objects (g_ctx, g_el, g_eb) and DevBackendT
namespace kai {
__global__ void __launch_bounds__(KAI_JO_WG) k_jo_qualify(KaiCtx c, JoArgs a) { jo_qualify_body(c, a); }
__global__ void __launch_bounds__(256) k_jo_leaf(KaiCtx c, JoArgs a) { jo_leaf_body(c, a); }
__global__ void __launch_bounds__(KAI_JO_WG) k_jo_keys(KaiCtx c, JoArgs a, RoundParams rp) { jo_keys_body(c, a, rp); }
__global__ void __launch_bounds__(1024) k_jo_scan(KaiCtx c, RoundParams rp) { jo_scan_body(c, rp); }
__global__ void __launch_bounds__(KAI_JO_WG) k_jo_emit(KaiCtx c, JoArgs a) { jo_emit_body(c, a); }
// one wavefront, of which lane 0 walks: the pop needs the context, the engine's scalars and nothing of k_action's service waves or its index levels in LDS
__global__ void __launch_bounds__(64) k_jo_engine(KaiCtx cv, JoArgs a) {
    if (threadIdx.x == 0) { g_ctx = cv; g_ctx.use_index = 0; g_ctx.sg = nullptr; g_ctx.sg_wgs = 0; g_ctx.mw = nullptr; g_ctx.mw_rank = 0; g_ctx.mw_world = 1; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    DevBackendT<false, false> be;
    jo_engine_walk(g_ctx, be, a);
}
}  // namespace kai
#endif
