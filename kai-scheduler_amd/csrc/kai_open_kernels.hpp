// kai_open_kernels.hpp — the kernels every cycle starts and ends in, as bodies on kai_simt.hpp, and their launch sequences.
//
//  * session open and reset: node accounting from the pods, proportion totals, queue usage roll-up (segmented reductions pods → job → leaf queue → ancestors),
//    fair-share division per tree level, the static fields of the job-order tree, and the class-index build (one wavefront per 64-node block, every scan class);
//  * action init: per-job eligibility / elastic state, per-leaf-queue stable compaction into job order;
//  * the drain: once no class has a fitting node, the jobs still queued are resolved chip-wide.
//
// Under hipcc every body gets a one-line __global__ entry point.  The launch sequences (open_drive, action_init_drive, index_drive, drain_drive) are written once
// against a Launcher: kai_session_open.hpp's OpenLauncher issues HIP launches on the session's stream, tests/host_sim/sim_session.hpp's runs the same bodies with the
// same grids and blocks on the lock-step emulator, so the CPU suite executes the device's algorithm — lane strides, butterflies, LDS staging, barriers — against the oracle.
//
// Every cross-lane call (kw::shfl, kw::ballot, kw::wave_sync, kw::sync) is reached by whole wavefronts; each body says why.  Block sizes are multiples of 64.
// No <hip/hip_runtime.h> here.
#pragma once
#include <algorithm>

#include "kai_ctx_build.hpp"
#include "kai_simt.hpp"

namespace kai {

// ------------------------------------------------------------------------------------------------------
// session open
// ------------------------------------------------------------------------------------------------------

// NodeInfo.AddTask for every active-used pod of the snapshot (api/node_info/node_info.go:384-493).
// Quantities are integers in float64 (milli-cores, bytes, devices, pod counts) so the f64 atomics commute exactly.  No cross-lane call.
KW_BODY void node_accounting_body(const KaiCtx& c) {
    int p = kw::bid() * kw::bdim() + kw::tid();
    if (p >= c.P) return;
    int s = c.p_status[p], n = c.p_node[p];
    c.p_on_node[p] = -1; c.p_on_node_status[p] = 0; c.p_accepted[p] = 0; c.p_virtual[p] = 0;
    if (!st_active_used(s) || n < 0 || n >= c.N) return;
    c.p_on_node[p] = n; c.p_on_node_status[p] = s; c.p_accepted[p] = 1;
    for (int r = 0; r < c.R; r++) {
        double v = c.p_req[(size_t)r * c.P + p]; if (v == 0) continue;
        size_t i = (size_t)r * c.N + n;
        kw::atomic_add(&c.n_used[i], v);
        if (s == KAI_POD_RELEASING) { kw::atomic_add(&c.n_rel[i], v); kw::atomic_add(&c.n_idle[i], -v); }
        else if (s == KAI_POD_PIPELINED) kw::atomic_add(&c.n_rel[i], -v);
        else kw::atomic_add(&c.n_idle[i], -v);
    }
}

#ifdef KAI_SHARED_GPUS
// shared GPUs: NodeInfo.AddTask of a node's active pods in UID order by ONE lane per node — addSharedTaskResources' guards read what the
// pods before them left behind (api/node_info/gpu_sharing_node_info.go:83-136), so the order inside a node is part of the result.  No cross-lane call in either.
KW_BODY void pod_accounting_reset_body(const KaiCtx& c) {
    int p = kw::bid() * kw::bdim() + kw::tid();
    if (p >= c.P) return;
    c.p_on_node[p] = -1; c.p_on_node_status[p] = 0; c.p_accepted[p] = 0; c.p_virtual[p] = 0; c.p_on_group[p] = -1;
}
KW_BODY void node_accounting_shared_body(const KaiCtx& c, const int32_t* np_off, const int32_t* np_pods) {
    int n = kw::bid() * kw::bdim() + kw::tid();
    if (n >= c.N) return;
    for (int i = np_off[n]; i < np_off[n + 1]; i++) {
        const int p = np_pods[i], st = c.p_status[p];
        c.p_on_node[p] = n; c.p_on_node_status[p] = st; c.p_accepted[p] = 1;
        const bool frac = c.p_shared[p] != 0;
        if (frac && c.p_group[p] >= 0) c.p_on_group[p] = c.p_group[p];
        for (int r = 0; r < c.R; r++) {
            if (r == KAI_RES_GPU && frac) continue;  // getAcceptedTaskResourceWithoutSharedGPU :52-66
            const double v = c.p_req[(size_t)r * c.P + p]; if (v == 0) continue;
            const size_t x = (size_t)r * c.N + n;
            c.n_used[x] += v;
            if (st == KAI_POD_RELEASING) { c.n_rel[x] += v; c.n_idle[x] -= v; } else if (st == KAI_POD_PIPELINED) c.n_rel[x] -= v; else c.n_idle[x] -= v;
        }
        if (frac && c.p_on_group[p] >= 0) { SgNode g{c, n}; if (!g.add(st, c.p_mem[p], c.p_on_group[p])) { c.st->fault = FAULT_INTERNAL; c.st->fault_line = __LINE__; } }
    }
    { SgNode g{c, n}; g.refit(); }  // the class keys' summary bits of the node's groups (also clears what an earlier session of this snapshot left: kai_session_reset)
}
#endif

// sum over the wavefront, in every lane: a butterfly of ds_bpermute shuffles on the device, the same addition tree on the emulator
template <class T> KW_BODY T wave_sum(T v) {
    for (int o = 32; o > 0; o >>= 1) v += kw::shfl(v, kw::lane() ^ o);
    return v;
}

// proportion.setTotalResources (plugins/proportion/proportion.go:252-288): Σ allocatable of ready nodes …
// (no lane leaves before the folds: the grid-stride loop ends per lane, the folds are reached by all)
KW_BODY void total_nodes_body(const KaiCtx& c) {
    double acc[3] = {0, 0, 0};
    for (int n = kw::bid() * kw::bdim() + kw::tid(); n < c.N; n += kw::gdim() * kw::bdim()) {
        uint32_t f = c.n_flags[n];
        if (f & KAI_NODE_NOT_READY) continue;
        bool ignore_gpus = c.restrict_nodes && !(f & KAI_NODE_GPU_WORKER);
        acc[KAI_Q_CPU] += c.n_alloc[(size_t)KAI_RES_CPU * c.N + n];
        acc[KAI_Q_MEM] += c.n_alloc[(size_t)KAI_RES_MEM * c.N + n];
        if (!ignore_gpus) {  // QuantifyResource(Allocatable): GPUs + MIG instances by weight (resource_info.go:177-194)
            acc[KAI_Q_GPU] += c.n_alloc[(size_t)KAI_RES_GPU * c.N + n];
#ifdef KAI_SHARED_GPUS
            if (c.mig_on) for (int r = KAI_RES_PODS + 1; r < c.R; r++) if (c.res_mig_g[r] > 0) acc[KAI_Q_GPU] += (double)c.res_mig_g[r] * c.n_alloc[(size_t)r * c.N + n];
#endif
        }
    }
    for (int k = 0; k < 3; k++) { double v = wave_sum(acc[k]); if (kw::lane() == 0 && v != 0) kw::atomic_add(&c.st->total[k], v); }
}
// … minus the active pods of other schedulers on those nodes (:276-285).  No cross-lane call.
KW_BODY void total_foreign_body(const KaiCtx& c) {
    int p = kw::bid() * kw::bdim() + kw::tid();
    if (p >= c.P) return;
    if (!(c.p_flags[p] & KAI_POD_FOREIGN_SCHEDULER)) return;
    int n = c.p_on_node[p]; if (n < 0) return;
    if (!st_active_used(c.p_on_node_status[p])) return;
    if (c.n_flags[n] & KAI_NODE_NOT_READY) return;
    kw::atomic_add(&c.st->total[KAI_Q_CPU], -c.p_req[(size_t)KAI_RES_CPU * c.P + p]);
    kw::atomic_add(&c.st->total[KAI_Q_MEM], -c.p_req[(size_t)KAI_RES_MEM * c.P + p]);
#ifdef KAI_SHARED_GPUS
    kw::atomic_add(&c.st->total[KAI_Q_GPU], -(c.quota_on ? c.p_quota_gpu[p] : c.p_req[(size_t)KAI_RES_GPU * c.P + p]));  // QuantifyResourceRequirements(ResReq)
#else
    kw::atomic_add(&c.st->total[KAI_Q_GPU], -c.p_req[(size_t)KAI_RES_GPU * c.P + p]);
#endif
}

// per-job sums + pod-set / job counters (api/podgroup_info/job_info.go:208-226, subgroup_info/podset.go:56-77).
// jsum[9][J]: (allocated, allocated_np, request) × (CPU, Memory, GPU) — proportion.updateQueuesCurrentResourceUsage :347-401.  No cross-lane call.
KW_BODY void job_usage_body(const KaiCtx& c, double* jsum) {
    int j = kw::bid() * kw::bdim() + kw::tid();
    if (j >= c.J) return;
    double al[3] = {0, 0, 0}, rq[3] = {0, 0, 0}, ja[3] = {0, 0, 0};
    int pending = 0;
    for (int k = 0; k < c.j_n_ps[j]; k++) { int s = c.j_first_ps[j] + k; c.s_active_alloc[s] = 0; c.s_active_used[s] = 0; c.s_alive[s] = 0; c.s_gated[s] = 0; c.s_pipelined[s] = 0; }
    for (int i = 0; i < c.j_n_pods[j]; i++) {
        int p = c.j_first_pod[j] + i, s = c.p_status[p], ps = c.p_podset[p];
        if (st_active_allocated(s)) c.s_active_alloc[ps]++;
        if (st_active_used(s)) c.s_active_used[ps]++;
        if (st_alive(s)) c.s_alive[ps]++;
        if (s == KAI_POD_GATED) c.s_gated[ps]++;
        if (s == KAI_POD_PIPELINED) c.s_pipelined[ps]++;
        if (s == KAI_POD_PENDING) pending++;
        double q[3] = {c.p_req[(size_t)KAI_RES_CPU * c.P + p], c.p_req[(size_t)KAI_RES_MEM * c.P + p], c.p_req[(size_t)KAI_RES_GPU * c.P + p]};
        double qa = q[2], qp = q[2], qq = q[2];  // GPU quota of AcceptedResource / GPU weight of a pending request / quota of ResReq: they differ from ResReq.GPUs() for gpu-memory and MIG requests
#ifdef KAI_SHARED_GPUS
        if (c.quota_on) { qa = c.p_acc_gpu[p]; qp = c.p_pend_gpu[p]; qq = c.p_quota_gpu[p]; }
#endif
        if (st_allocated(s)) {
            for (int k = 0; k < 3; k++) ja[k] += k == 2 ? qq : q[k];  // PodGroupInfo.Allocated carries the MIG instances (job_info.go:231-251): QuantifyResource of it
            if (c.p_accepted[p]) for (int k = 0; k < 3; k++) { const double v = k == 2 ? qa : q[k]; al[k] += v; rq[k] += v; }  // AcceptedResource is empty for a pod no node holds
        } else if (s == KAI_POD_PENDING) {
            for (int k = 0; k < 3; k++) rq[k] += k == 2 ? qp : q[k];
        }
    }
    c.j_n_pending[j] = pending; c.j_tta_valid[j] = 0; c.j_tta_n[j] = 0;
    bool np = !c.j_preempt[j];
    for (int k = 0; k < 3; k++) {
        c.j_allocated[(size_t)j * 4 + k] = ja[k];
        jsum[(size_t)(0 + k) * c.J + j] = al[k]; jsum[(size_t)(3 + k) * c.J + j] = np ? al[k] : 0.0; jsum[(size_t)(6 + k) * c.J + j] = rq[k];
    }
}
// one wavefront per leaf queue: segmented reduction over the queue's jobs (jobs_static is CSR by q_job_off; the sum order is
// fixed by the lane stride, and the addends are integer-valued, so the result does not depend on it).  The queue is the wavefront's: it leaves whole or folds whole.
KW_BODY void leaf_usage_body(const KaiCtx& c, const double* jsum) {
    int q = kw::bid() * (kw::bdim() / 64) + (kw::tid() >> 6);
    if (q >= c.Q) return;
    int lane = kw::lane(), b = c.q_job_off[q], e = c.q_job_off[q + 1];
    double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = b + lane; i < e; i += 64) { int j = c.jobs_static[i]; for (int x = 0; x < 9; x++) acc[x] += jsum[(size_t)x * c.J + j]; }
    for (int x = 0; x < 9; x++) acc[x] = wave_sum(acc[x]);
    if (lane == 0) for (int k = 0; k < 3; k++) {
        QShare& s = c.q_share[(size_t)q * 3 + k];
        s.allocated = acc[k]; s.allocated_np = acc[3 + k]; s.request = acc[6 + k]; s.fair = 0;
    }
}
// ancestors: level by level up the tree (leaf = height 0), one lane per (inner queue, field): a segmented reduction over the queue's children,
// added in child-index order like the sequential roll-up.  One workgroup; h_nodes / h_off list the queues by height (HostPrep::build_batch).
// The loop over the heights is the same in every lane, so every lane reaches every barrier.
KW_BODY void tree_usage_body(const KaiCtx& c, const int32_t* h_off, const int32_t* h_nodes, int n_h) {
    for (int h = 1; h < n_h - 1; h++) {  // the virtual root (last height) holds no shares
        const int b = h_off[h], e = h_off[h + 1];
        for (int t = kw::tid(); t < (e - b) * 9; t += kw::bdim()) {
            const int x = h_nodes[b + t / 9], f = (t % 9) / 3, k = t % 3;
            if (x >= c.Q) continue;
            double acc = 0.0;
            for (int i = c.q_child_off[x]; i < c.q_child_off[x + 1]; i++) {
                const QShare& s = c.q_share[(size_t)c.q_children[i] * 3 + k];
                acc += f == 0 ? s.allocated : f == 1 ? s.allocated_np : s.request;
            }
            QShare& d = c.q_share[(size_t)x * 3 + k];
            if (f == 0) d.allocated += acc; else if (f == 1) d.allocated_np += acc; else d.request += acc;
        }
        kw::fence(); kw::sync();
    }
}
// proportion.setFairShareForQueues (plugins/proportion/proportion.go:410-423), one tree level per launch (a level's totals are the parents' fair
// shares of the level above).  One wavefront per (sibling set, resource): the lanes stage the set — shares, priorities, creation times — into LDS,
// lane 0 runs the division (resource_division.go:26-357: rounds whose outcome feeds the next, sequential by construction) on the staged copy, the
// lanes write the fair shares back.  Sets of more than 64 queues run on the session arrays directly.  (set, resource) and the set's size are the
// wavefront's: it leaves whole, or reaches both wave_syncs whole.
struct SiblingsLds {
    QShare* sh; int64_t* pr; int64_t* cr; uint32_t* ui; double* w; double* ra; uint8_t* rh;
    KAI_HD QShare& share(int i) const { return sh[i]; }
    KAI_HD int64_t prio(int i) const { return pr[i]; }
    KAI_HD int64_t created(int i) const { return cr[i]; }
    KAI_HD uint32_t uid(int i) const { return ui[i]; }
    KAI_HD double& weight(int i) const { return w[i]; }
    KAI_HD double& rem_amt(int i) const { return ra[i]; }
    KAI_HD uint8_t& rem_has(int i) const { return rh[i]; }
};
constexpr int FS_WAVES = 4, FS_MAX = 64;
KW_BODY void fair_share_level_body(const KaiCtx& c, const int32_t* lvl_parents, int first, int count, double* weight, double* rem_amt, uint8_t* rem_has) {
    KW_SHARED QShare s_sh[FS_WAVES][FS_MAX]; KW_SHARED int64_t s_pr[FS_WAVES][FS_MAX], s_cr[FS_WAVES][FS_MAX];
    KW_SHARED uint32_t s_ui[FS_WAVES][FS_MAX]; KW_SHARED double s_w[FS_WAVES][FS_MAX], s_ra[FS_WAVES][FS_MAX]; KW_SHARED uint8_t s_rh[FS_WAVES][FS_MAX];
    const int wave = kw::tid() >> 6, lane = kw::lane(), t = kw::bid() * FS_WAVES + wave;
    if (t >= count * 3) return;
    const int par = lvl_parents[first + t / 3], k = t % 3;
    const double total = par == c.Q ? c.st->total[k] : c.q_share[(size_t)par * 3 + k].fair;
    const int32_t* kids = c.q_children + c.q_child_off[par];
    const int nk = c.q_child_off[par + 1] - c.q_child_off[par];
    if (nk > FS_MAX) { if (lane == 0) divide_sibling_set(c, kids, nk, k, total, c.k_value, weight + (size_t)k * c.Q, rem_amt + (size_t)k * c.Q, rem_has + (size_t)k * c.Q); return; }
    if (lane < nk) { const int q = kids[lane]; s_sh[wave][lane] = c.q_share[(size_t)q * 3 + k]; s_pr[wave][lane] = c.q_prio[q]; s_cr[wave][lane] = c.q_created[q]; s_ui[wave][lane] = c.q_uid_rank[q]; }
    kw::wave_sync();
    if (lane == 0) { SiblingsLds v{s_sh[wave], s_pr[wave], s_cr[wave], s_ui[wave], s_w[wave], s_ra[wave], s_rh[wave]}; divide_sibling_view(v, nk, total, c.k_value); }
    kw::wave_sync();
    if (lane < nk) c.q_share[(size_t)kids[lane] * 3 + k].fair = s_sh[wave][lane].fair;
}

// L1 of the class index: one wavefront per 64-node block, every class (node state is read once per class from L1/L2).  The block is the wavefront's,
// and a lane past the last node takes part with key 0.
KW_BODY void index_build_body(const KaiCtx& c) {
    int b = kw::bid() * (kw::bdim() / 64) + (kw::tid() >> 6);
    if (b >= c.NB) return;
    int lane = kw::lane(), n = b * KAI_BLOCK + lane;
    NodeRegs ns; load_node(c, n < c.N ? n : 0, ns);
    for (int k = 0; k < c.C; k++) {
        uint64_t key = n < c.N ? class_key_regs(c, c.cls[k], ns) : 0; int bn = n;
        kw::wave_argmax_first(key, bn);
        if (lane == 0) { c.sum1_key[(size_t)k * c.NB + b] = key; c.sum1_node[(size_t)k * c.NB + b] = bn; }
    }
}

// ------------------------------------------------------------------------------------------------------
// action init
// ------------------------------------------------------------------------------------------------------
struct NullBackend {  // kernels that only need the engine's pure helpers
    static constexpr bool kVictim = false;
    template <class T> KW_DEV static void assume_tree(T*) {}
    const KaiCtx* cref = nullptr; EngineLocal loc;
    static constexpr bool kBig = false;  // (no scan lane ever reads the control lane's larger data; big() only has to exist)
    KW_DEV static EngineBig& big();
    KW_DEV void bind(const KaiCtx& c) { cref = &c; }
    KW_DEV const KaiCtx& ctx() const { return *cref; }
    KW_DEV EngineLocal& local() { return loc; }
    KW_DEV void minmax(const KaiCtx&, int, double&, double&) {}
    KW_DEV bool topo_scan(const KaiCtx&, TopoScan&) { return false; }
    KW_DEV bool pfor(const KaiCtx&, const PforReq&) { return false; }
#if defined(__HIPCC__)
    KW_DEV void or32(uint32_t* w, uint32_t bits) { atomicOr(w, bits); }
    KW_DEV static void add_f64(double* p, double v) { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }  // the roll-ups of subSetNodesFn: one workgroup, one L2
    KW_DEV static void add_i32(int32_t* p, int32_t v) { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    KW_DEV static double coh_f64(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }  // coherent with the atomics of workgroups on other XCDs
    KW_DEV static int32_t coh_i32(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
#else  // the emulator: one lane runs at a time
    void or32(uint32_t* w, uint32_t bits) { *w |= bits; }
    static void add_f64(double* p, double v) { *p += v; }
    static void add_i32(int32_t* p, int32_t v) { *p += v; }
    static double coh_f64(const double* p) { return *p; }
    static int32_t coh_i32(const int32_t* p) { return *p; }
#endif
    KW_DEV int best_node(const KaiCtx&, const ScanReq&, double* = nullptr) { return -1; }
    KW_DEV bool eval_nodes(const KaiCtx&, const ScanReq&, const int32_t*, int, double*, uint8_t*) { return false; }
    KW_DEV void begin(const KaiCtx&) {}
    KW_DEV bool dirty_add(int) { return true; }
    KW_DEV int dirty_count() { return 0; }
    KW_DEV void refresh(const KaiCtx&) {}
    KW_DEV void class_top(const KaiCtx&, int, uint64_t& k, int& n) { k = 0; n = -1; }
    KW_DEV bool all_dead(const KaiCtx&) { return false; }
    KW_DEV void stage_async(const KaiCtx&, int) {}
    KW_DEV bool staged(int) { return false; }
    KW_DEV void hot(const KaiCtx&, QNode*&, int32_t*&, int32_t*&) {}
    KW_DEV bool sim_tree(QNode*&, int32_t*&, int32_t*&) { return false; }
    KW_DEV int64_t clock() { return 0; }
};
#if !defined(__HIPCC__)
inline EngineBig& NullBackend::big() { static EngineBig b; return b; }  // (never dereferenced: kBig is false; the device's is an LDS object of kai_kernels.hpp)
#endif

// static fields of the job-order tree records (parent chain, priority, heap offsets): valid from session open on.  No cross-lane call, nor in job_init_body.
KW_BODY void qnode_static_body(const KaiCtx& c) {
    int q = kw::bid() * kw::bdim() + kw::tid();
    if (q < c.Q) qnode_init(c, q, 0);
}
KW_BODY void job_init_body(const KaiCtx& c) {
    int j = kw::bid() * kw::bdim() + kw::tid();
    if (j >= c.J) return;
    uint8_t st = job_init_state(c, j);
    c.j_state[j] = st;
    // the tasks-to-allocate chunk of every queued job (allocation_info.go:27-113), which the queue comparator reads for the best
    // job of each queue: computed here chip-wide instead of lazily by the control lane.  Nothing is virtual before the first
    // statement of an action, so the chunk does not depend on isRealAllocation.
    if (st != 3 && c.j_n_ps[j] <= 64) { NullBackend nb; Engine<NullBackend> eng(c, nb); eng.ensure_tta(j, true); }
}
// One wavefront per leaf queue: stable compaction of the eligible "below minAvailable" jobs (host order: priority desc,
// creation, uid) into the leaf's sorted region; the few jobs in another elastic state go to the leaf's side heap, which lane 0
// heapifies once the other lanes' entries are in place.  The queue, and so the trip count of the loop with the ballots, is the wavefront's.
KW_BODY void leaf_init_body(const KaiCtx& c) {
    int q = kw::bid() * (kw::bdim() / 64) + (kw::tid() >> 6);
    if (q >= c.Q) return;
    int lane = kw::lane(), b = c.q_job_off[q], e = c.q_job_off[q + 1];
    int cnt = 0, side = 0;
    for (int base = b; base < e; base += 64) {
        int i = base + lane, j = i < e ? c.jobs_static[i] : -1;
        int st = j >= 0 ? c.j_state[j] : 3;
        uint64_t m0 = kw::ballot(st == 0), m12 = kw::ballot(st == 1 || st == 2);
        if (st == 0) c.lq_sorted[b + cnt + kw::rank_below(m0)] = j;
        if (st == 1 || st == 2) c.lq_side[b + side + kw::rank_below(m12)] = j;
        cnt += __builtin_popcountll(m0); side += __builtin_popcountll(m12);
    }
    kw::wave_sync();
    if (lane == 0) {
        c.lq_cur[q] = 0; c.lq_end[q] = cnt; c.lq_side_len[q] = 0;
        qnode_init(c, q, cnt + side);
        if (side) {
            NullBackend nb; Engine<NullBackend> eng(c, nb);
            int32_t* h = c.lq_side + b;
            for (int i = 0; i < side; i++) { c.lq_side_len[q] = i + 1; eng.heap_up(h, i, typename Engine<NullBackend>::JobLess{&eng}); }
        }
    }
}

// ------------------------------------------------------------------------------------------------------
// end of allocate
// ------------------------------------------------------------------------------------------------------
// Once no class has a fitting node at a committed state, every job still queued is attempted, gated and fails at its first
// task without changing any state (Engine::drain_job): resolve them chip-wide.  Slot i of a leaf's region holds a job of the
// sorted part if cur <= pos < end and a job of the side heap if pos < side_len.  drain_pending is the same for every lane, and the
// grid-stride loop ends per lane: the folds are reached by all.
KW_BODY void drain_body(const KaiCtx& c, const int32_t* slot_queue) {
    if (!c.st->drain_pending) return;
    NullBackend nb; Engine<NullBackend> eng(c, nb);
    int64_t att = 0, dec = 0, rb = 0;
    for (int i = kw::bid() * kw::bdim() + kw::tid(); i < c.J; i += kw::gdim() * kw::bdim()) {
        int q = slot_queue[i]; if (q < 0) continue;
        int pos = i - c.q_job_off[q];
        if (pos >= c.lq_cur[q] && pos < c.lq_end[q]) eng.drain_job(c.lq_sorted[i], att, dec, rb);
        if (pos < c.lq_side_len[q]) eng.drain_job(c.lq_side[i], att, dec, rb);
    }
    att = wave_sum(att); dec = wave_sum(dec); rb = wave_sum(rb);
    if (kw::lane() == 0 && att) {
        kw::atomic_add((unsigned long long*)&c.st->jobs_attempted, (unsigned long long)att); kw::atomic_add((unsigned long long*)&c.st->decisions, (unsigned long long)dec);
        kw::atomic_add((unsigned long long*)&c.st->rollbacks, (unsigned long long)rb);
        kw::atomic_add((unsigned long long*)&c.st->drained_jobs, (unsigned long long)att); kw::atomic_add((unsigned long long*)&c.st->drained_decisions, (unsigned long long)dec);
    }
}

#if defined(__HIPCC__)
__global__ void k_node_accounting(KaiCtx c) { node_accounting_body(c); }
#ifdef KAI_SHARED_GPUS
__global__ void k_pod_accounting_reset(KaiCtx c) { pod_accounting_reset_body(c); }
__global__ void k_node_accounting_shared(KaiCtx c, const int32_t* np_off, const int32_t* np_pods) { node_accounting_shared_body(c, np_off, np_pods); }
#endif
__global__ void k_total_nodes(KaiCtx c) { total_nodes_body(c); }
__global__ void k_total_foreign(KaiCtx c) { total_foreign_body(c); }
__global__ void k_job_usage(KaiCtx c, double* jsum) { job_usage_body(c, jsum); }
__global__ void k_leaf_usage(KaiCtx c, const double* jsum) { leaf_usage_body(c, jsum); }
__global__ void k_tree_usage(KaiCtx c, const int32_t* h_off, const int32_t* h_nodes, int n_h) { tree_usage_body(c, h_off, h_nodes, n_h); }
__global__ void __launch_bounds__(FS_WAVES * 64) k_fair_share_level(KaiCtx c, const int32_t* lvl_parents, int first, int count, double* weight, double* rem_amt, uint8_t* rem_has) { fair_share_level_body(c, lvl_parents, first, count, weight, rem_amt, rem_has); }
__global__ void k_qnode_static(KaiCtx c) { qnode_static_body(c); }
__global__ void k_index_build(KaiCtx c) { index_build_body(c); }
__global__ void k_job_init(KaiCtx c) { job_init_body(c); }
__global__ void k_leaf_init(KaiCtx c) { leaf_init_body(c); }
__global__ void k_drain(KaiCtx c, const int32_t* slot_queue) { drain_body(c, slot_queue); }
#endif

// ------------------------------------------------------------------------------------------------------
// the launch sequences, written once against a Launcher: a method per kernel (grid, block, the kernel's arguments) and fill32(array, byte, elements)
// ------------------------------------------------------------------------------------------------------
constexpr int OPEN_TB = 256;  // four wavefronts per workgroup: a thread, or a wavefront, per item
// what the open's launches need of the host preparation besides OpenAux
struct OpenShape { int n_levels; const int32_t* lvl_off; int n_heights; uint32_t plugins; bool shared; };

template <class L> void index_drive(L& l, const KaiCtx& c) { if (c.use_index && c.NB) l.index_build((c.NB + 3) / 4, OPEN_TB, c); }
// session open and reset over the resident snapshot, first half: node accounting, proportion totals, queue usage up the tree
template <class L> void open_usage_drive(L& l, const KaiCtx& c, const OpenAux& x, const OpenShape& s) {
    const int N = c.N, P = c.P, J = c.J, Q = c.Q, TB = OPEN_TB;
    const bool prop = s.plugins & KAI_PLUGIN_PROPORTION;
    if (s.shared) {  // shared GPUs: group tables reset, then every node adds its pods in UID order (one lane per node)
        if (N) l.fill32(c.ng_id, 0xFF, (size_t)N * KAI_GMAX);
        if (P) l.pod_accounting_reset((P + TB - 1) / TB, TB, c);
        if (N) l.node_accounting_shared((N + TB - 1) / TB, TB, c, x.np_off, x.np_pods);
    } else if (P) l.node_accounting((P + TB - 1) / TB, TB, c);
    if (prop) {
        if (N) l.total_nodes(std::min(1024, (N + TB - 1) / TB), TB, c);
        if (P) l.total_foreign((P + TB - 1) / TB, TB, c);
    }
    if (J) l.job_usage((J + TB - 1) / TB, TB, c, x.jsum);
    if (prop && Q) {
        l.leaf_usage((Q + 3) / 4, TB, c, x.jsum);
        l.tree_usage(1, 1024, c, x.h_off, x.h_nodes, s.n_heights);
    }
}
// ... second half: fair shares level by level, the job-order tree's static fields, the class index
template <class L> void open_shares_drive(L& l, const KaiCtx& c, const OpenAux& x, const OpenShape& s) {
    const int Q = c.Q;
    if (s.plugins & KAI_PLUGIN_PROPORTION) for (int lv = 0; Q && lv < s.n_levels; lv++) {  // a level's totals are the fair shares of the level above: one launch per level
        const int first = s.lvl_off[lv], count = s.lvl_off[lv + 1] - first;
        if (count > 0) l.fair_share_level((count * 3 + FS_WAVES - 1) / FS_WAVES, FS_WAVES * 64, c, x.lvl_parents, first, count, x.weight, x.rem_amt, x.rem_has);
    }
    if (Q) l.qnode_static((Q + OPEN_TB - 1) / OPEN_TB, OPEN_TB, c);
    index_drive(l, c);
}
template <class L> void open_drive(L& l, const KaiCtx& c, const OpenAux& x, const OpenShape& s) { open_usage_drive(l, c, x, s); open_shares_drive(l, c, x, s); }
// the start of every action: the class index rebuilt if the last action left it stale, the jobs' and the leaves' state
template <class L> void action_init_drive(L& l, const KaiCtx& c, bool& index_stale) {
    if (index_stale) { index_drive(l, c); index_stale = false; }
    if (c.J) l.job_init((c.J + OPEN_TB - 1) / OPEN_TB, OPEN_TB, c);
    if (c.Q) l.leaf_init((c.Q + 3) / 4, OPEN_TB, c);
}
template <class L> void drain_drive(L& l, const KaiCtx& c, const OpenAux& x) { if (c.J) l.drain(std::min(2048, (c.J + 255) / 256), 256, c, x.slot_queue); }

}  // namespace kai
