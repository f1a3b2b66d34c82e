// kai_ctx_build.hpp — the session context (KaiCtx) built from a snapshot and its host preparation: which arrays exist, their element counts, what an absent optional array
// stands for, which constants are written where they are read instead of being sent.  Written ONCE, over an arena type A, and called by kai_session_open (kai_session_open.hpp:
// the slab allocator in HBM) and by the host simulation (tests/host_sim/sim_session.hpp: one std::vector per array) — so what the CPU suite exercises under the oracle is the
// open the device runs.  No HIP here.  The ORDER of the arena calls is the session's layout in HBM.
//
// An arena offers, each call on a field of the context or of OpenAux (n elements of the field's type; an array of no elements is one element nobody reads):
//   alloc(field, n)                    allocated, not written
//   zero(field, n), fill(field, n, b)  allocated, every byte set
//   upload(field, host, n)             allocated and copied from the host; n == 0 leaves one zeroed element
//   stage(field, host, n), flush()     the snapshot's own arrays, which go up before the host preparation runs (the library sends them from pinned staging meanwhile)
//   copy_of(field, src, n)             allocated and filled from an array the arena already holds
//   status()                           KAI_OK, or the first failure — after which every call does nothing
#pragma once
#include "kai_engine.hpp"
#include "kai_host_prep.hpp"

namespace kai {

// arrays of the open that belong to the handle, not to the context (no part of a victim action's replicas): arguments of the session-open kernels, k_drain and k_best_node
struct OpenAux {
    int32_t *slot_queue = nullptr, *lvl_off = nullptr, *lvl_parents = nullptr, *h_off = nullptr, *h_nodes = nullptr;  // job slot -> its queue; fair-share levels; queues by height (leaf = 0), for the usage roll-up
    int32_t *group0 = nullptr, *np_off = nullptr, *np_pods = nullptr;  // shared GPUs: the pods' initial groups (kai_session_reset), each node's active pods in UID order
    double *jsum = nullptr, *weight = nullptr, *rem_amt = nullptr; uint8_t* rem_has = nullptr; int32_t* best_out = nullptr;  // [9 J], [3 Q] each, [2]
};
struct CtxBuildIn {
    const kai_config& cfg; const kai_snapshot_soa* s; const HostPrep& prep; const SharedPods& sp;
    bool full_uploads;  // KAI_OPEN_FULL_UPLOADS (diagnostic): every array sent from the host, no constant written in place
    int out_lists;      // out_ops holds that many actions' operations (the library: 1, every action hands its own to the caller)
};
// what the open's caller keeps beside the context (kai_session_update's bookkeeping)
struct CtxBuildOut {
    bool idx_forced_off = false, fast_forced_off = false;  // the shared-GPU / MIG rules switched the class index / the staged job path off
    int32_t next_group = KAI_NEW_GROUP;  // first shared-GPU group id the cycle may open
    std::vector<int32_t> groups;         // the pods' shared-GPU groups as sent (empty: none anywhere, -1 written in place)
    std::vector<int64_t> gpu_mem;        // node_gpu_memory in engine order (what n_gpu_mem holds)
    std::vector<int32_t> np_off, np_pods;  // what OpenAux::np_off / np_pods hold
};

// NodeInfo.LegacyMIGTasks (node_info.go:407-409): a node that holds a legacy MIG task takes no MIG request.  Before the builder: the flag goes up with n_flags.
// (needs s->pod_flags; cnt: per engine node, its active legacy MIG tasks)
inline void flag_legacy_mig_nodes(const kai_snapshot_soa* s, HostPrep& prep, std::vector<int32_t>& cnt) {
    cnt.assign((size_t)s->n_nodes, 0);
    for (int p = 0; p < s->n_pods; p++)
        if ((s->pod_flags[p] & KAI_POD_LEGACY_MIG) && prep.pod_node[p] >= 0 && (s->pod_status[p] & KAI_POD_ACTIVE)) { prep.node_flags[prep.pod_node[p]] |= KAI_NODE_LEGACY_MIG_I; cnt[(size_t)prep.pod_node[p]]++; }
}

// the scalars that need no host preparation (the first thing an open does to its context)
inline void ctx_scalars(KaiCtx& c, const kai_config& cfg, const kai_snapshot_soa* s) {
    c = KaiCtx{};
    c.N = s->n_nodes; c.P = s->n_pods; c.S = s->n_podsets; c.J = s->n_jobs; c.Q = s->n_queues; c.R = s->n_res;
    c.n_pod_classes = std::max(1, s->n_pod_classes); c.n_node_classes = std::max(1, s->n_node_classes);
    c.plugins = cfg.plugins; c.gpu_strategy = cfg.gpu_strategy; c.cpu_strategy = cfg.cpu_strategy;
    c.restrict_nodes = cfg.restrict_node_scheduling; c.k_value = cfg.k_value <= 0.0 ? 0.0 : cfg.k_value;  // proportion.go:77-84
    { int d = cfg.queue_depth[KAI_ACTION_ALLOCATE]; c.queue_depth = d > 0 ? d : 0; }
    c.action = KAI_ACTION_ALLOCATE; c.max_consolidation_preemptees = cfg.max_consolidation_preemptees; c.allow_consolidating_reclaim = cfg.allow_consolidating_reclaim;
    c.saturation_multiplier = cfg.reclaimer_saturation_multiplier; c.use_signatures = cfg.use_scheduling_signatures ? 1 : 0;
    c.now_ns = cfg.now_ns; c.def_preempt_mr = cfg.default_preempt_min_runtime_ns; c.def_reclaim_mr = cfg.default_reclaim_min_runtime_ns; c.reclaim_method = cfg.reclaim_resolve_method;
}
// the snapshot's own arrays: allocated first, on their way while the host preparation runs
template <class A> int ctx_stage_snapshot(A& a, KaiCtx& c, const kai_snapshot_soa* s) {
    const size_t P = (size_t)c.P, S = (size_t)c.S, J = (size_t)c.J;
    a.stage(c.p_req, s->pod_req, (size_t)c.R * P); a.stage(c.p_job, s->pod_job, P); a.stage(c.p_podset, s->pod_podset, P);
    if (s->pod_flags) a.stage(c.p_flags, s->pod_flags, P); else a.zero(c.p_flags, P);  // (an optional array that is absent: zeros written in place, not 4 MB of host zeros sent over)
    if (s->pod_class) a.stage(c.p_class, s->pod_class, P); else a.zero(c.p_class, P);
    a.stage(c.p_status, s->pod_status, P);
    a.stage(c.s_job, s->podset_job, S); a.stage(c.s_min, s->podset_min_available, S); a.stage(c.s_name_rank, s->podset_name_rank, S);
    a.stage(c.j_queue, s->job_queue, J); a.stage(c.j_prio, s->job_priority, J); a.stage(c.j_preempt, s->job_preemptible, J); a.stage(c.j_created, s->job_created_ns, J); a.stage(c.j_uid_rank, s->job_uid_rank, J);
    a.stage(c.j_first_pod, s->job_first_pod, J); a.stage(c.j_n_pods, s->job_n_pods, J); a.stage(c.j_first_ps, s->job_first_podset, J); a.stage(c.j_n_ps, s->job_n_podsets, J);
    return a.flush();
}
// static arrays (optional ones get neutral defaults); nodes go up in name-rank order
template <class A> int ctx_static_arrays(A& a, KaiCtx& c, OpenAux& x, const CtxBuildIn& in) {
    const kai_snapshot_soa* s = in.s; const HostPrep& prep = in.prep; const size_t N = (size_t)c.N, P = (size_t)c.P, J = (size_t)c.J, Q = (size_t)c.Q;
    const uint8_t one = 1;
    a.upload(c.n_alloc, prep.node_alloc.data(), (size_t)c.R * N); a.upload(c.n_flags, prep.node_flags.data(), N); a.upload(c.n_gpu_count, prep.node_gpu_count.data(), N); a.upload(c.n_class, prep.node_class.data(), N);
    if (prep.any_nominated || in.full_uploads) a.upload(c.p_nominated, prep.pod_nominated.data(), P);
    else a.fill(c.p_nominated, P, 0xFF);  // no nominated node anywhere: -1 in every element
    a.upload(c.p_scls, prep.pod_scls.data(), P);
    a.upload(c.q_parent, s->queue_parent, Q); a.upload(c.q_prio, s->queue_priority, Q); a.upload(c.q_created, s->queue_created_ns, Q); a.upload(c.q_uid_rank, s->queue_uid_rank, Q);
    if (s->class_fit && s->n_pod_classes > 0 && s->n_node_classes > 0) a.upload(c.class_fit, s->class_fit, (size_t)s->n_pod_classes * s->n_node_classes);
    else a.upload(c.class_fit, &one, (size_t)1);
    a.upload(c.j_pods_sorted, prep.sorted.data(), P);
    a.upload(c.q_child_off, prep.child_off.data(), Q + 2); a.upload(c.q_children, prep.children.data(), std::max<size_t>(Q, 1)); a.upload(c.q_job_off, prep.job_off.data(), Q + 1);
    a.upload(c.jobs_static, prep.jobs_static.data(), std::max<size_t>(J, 1)); a.upload(c.q_depth_order, prep.depth_order.data(), Q); a.upload(x.slot_queue, prep.slot_queue.data(), std::max<size_t>(J, 1));
    a.upload(x.lvl_off, prep.lvl_off.data(), prep.lvl_off.size()); a.upload(x.lvl_parents, prep.lvl_parents.data(), prep.lvl_parents.size());
    a.upload(x.h_off, prep.h_off.data(), prep.h_off.size()); a.upload(x.h_nodes, prep.h_nodes.data(), prep.h_nodes.size());
    // ---- scan classes + class index
    c.C = (int)prep.classes.size(); c.NB = (c.N + KAI_BLOCK - 1) / KAI_BLOCK; c.NSB = (c.NB + 63) / 64;
    c.use_index = c.C > 0 ? 1 : 0; c.all_tracked = prep.all_tracked; c.fast_ok = prep.fast_ok; c.exact_sums = prep.exact_sums;
    if (s->job_signature) a.upload(c.j_signature, s->job_signature, J);
    if (s->job_last_start_ns) a.upload(c.j_last_start, s->job_last_start_ns, J);
    if (s->queue_preempt_min_runtime_ns) a.upload(c.q_preempt_mr, s->queue_preempt_min_runtime_ns, Q); if (s->queue_reclaim_min_runtime_ns) a.upload(c.q_reclaim_mr, s->queue_reclaim_min_runtime_ns, Q);
    a.upload(c.cls, prep.classes.data(), prep.classes.size());
    const size_t CB = (size_t)std::max(c.C, 1) * std::max(c.NB, 1);
    a.zero(c.sum1_key, CB); a.zero(c.sum1_node, CB);
    return a.status();
}
// shared GPUs: per-pod portion / group, per-node GPU memory and group tables (api/node_info/gpu_sharing_node_info.go)
template <class A> int ctx_shared_gpus(A& a, KaiCtx& c, OpenAux& x, const CtxBuildIn& in, CtxBuildOut& out) {
    const kai_snapshot_soa* s = in.s; const HostPrep& prep = in.prep; const SharedPods& sp = in.sp; const int N = c.N, P = c.P;
    const bool shared = sp.any; out.gpu_mem.assign((size_t)std::max(N, 1), 100);
    for (int n = 0; n < N; n++) out.gpu_mem[n] = s->node_gpu_memory ? s->node_gpu_memory[prep.perm[n]] : 100;
    c.quota_on = sp.on ? 1 : 0; c.mig_on = sp.mig ? 1 : 0;
    for (int r = 0; r < KAI_MAX_RES; r++) { c.res_mig_g[r] = sp.mig_g[r]; c.res_mig_m[r] = sp.mig_m[r]; }
    // (both ways allocate the arrays in ONE order — the session's layout in HBM does not depend on what is sent; tests/test_open_uploads.py compares the images)
    a.upload(c.p_shared, sp.shared.data(), (size_t)P);
    const size_t P1 = (size_t)std::max(P, 1);
    bool por_zero = true;  // pod_gpu_portion absent, or +0.0 in every element (what a packer that always fills the array sends for a cluster without fractions)
    if (!sp.on && s->pod_gpu_portion) {
        std::vector<char> nz((size_t)chunk_count((size_t)P), 0);
        parallel_chunks((size_t)P, [&](int ci, size_t p0, size_t p1) { for (size_t p = p0; p < p1; p++) { uint64_t b; std::memcpy(&b, &s->pod_gpu_portion[p], 8); if (b) { nz[(size_t)ci] = 1; return; } } });
        for (char v : nz) if (v) por_zero = false;
    }
    // A snapshot without shared-GPU requests and without MIG rows (SharedPods: neither `any` nor `mig`): the per-pod quantities of the shared-GPU model are constants —
    // no memory of a device asked for, no MIG quota, every GPU quantity the pod's GPU request (the row of p_req that the arena holds already), no group anywhere.  They are
    // written where they are read instead of being sent: at config 5 these arrays are 73 of the open's 190 MB over PCIe.  (The host simulation checks on every
    // snapshot the CPU suite runs that both ways leave the same bytes: tests/host_sim/sim_session.hpp lean_equals_full.)
    const bool lean_pods = !sp.on && por_zero && !in.full_uploads;
    std::vector<double> por; std::vector<int32_t> minus1; std::vector<int32_t>& grp = out.groups;
    out.next_group = KAI_NEW_GROUP; grp.clear();
    if (!lean_pods) {
        por.assign(P1, 0.0); grp.assign(P1, -1); minus1.assign(P1, -1);
        for (int p = 0; p < P; p++) { por[p] = s->pod_gpu_portion ? s->pod_gpu_portion[p] : 0.0; grp[p] = (s->pod_gpu_group && sp.shared[p]) ? s->pod_gpu_group[p] : -1; if (grp[p] >= out.next_group) out.next_group = grp[p] + 1; }
    }
    const auto gpu_row = c.p_req + (size_t)KAI_RES_GPU * P;  // the pods' GPU requests
    if (lean_pods) {
        a.zero(c.p_mem, (size_t)P); a.zero(c.p_gmem, (size_t)P);
        a.copy_of(c.p_acc_gpu, gpu_row, (size_t)P); a.copy_of(c.p_pend_gpu, gpu_row, (size_t)P); a.copy_of(c.p_quota_gpu, gpu_row, (size_t)P);
        a.zero(c.p_mig_q, (size_t)P);
    } else {
        a.upload(c.p_mem, sp.mem.data(), (size_t)P); a.upload(c.p_gmem, sp.gmem.data(), (size_t)P);
        a.upload(c.p_acc_gpu, sp.acc_gpu.data(), (size_t)P); a.upload(c.p_pend_gpu, sp.pend_gpu.data(), (size_t)P);
        a.upload(c.p_quota_gpu, sp.quota_gpu.data(), (size_t)P); a.upload(c.p_mig_q, sp.mig_q.data(), (size_t)P);
    }
    a.upload(c.p_kind, sp.kind.data(), (size_t)P);
    if (lean_pods) { a.zero(c.p_portion, (size_t)P); a.fill(c.p_group, (size_t)P, 0xFF); a.fill(c.p_on_group, (size_t)P, 0xFF); }
    else { a.upload(c.p_portion, por.data(), (size_t)P); a.upload(c.p_group, grp.data(), (size_t)P); a.upload(c.p_on_group, minus1.data(), (size_t)P); }
    a.upload(c.n_gpu_mem, out.gpu_mem.data(), (size_t)N);
    if (lean_pods) a.fill(x.group0, (size_t)P, 0xFF); else a.upload(x.group0, grp.data(), P1);
    const size_t NG = (size_t)N * KAI_GMAX;
    a.alloc(c.ng_id, NG);  // (written by the open's first kernel of a shared-GPU session; nothing reads it in any other)
    a.zero(c.ng_used, NG); a.zero(c.ng_rel, NG); a.zero(c.ng_alloc, NG); a.zero(c.ng_mark, (size_t)N); a.zero(c.ng_has_alloc, (size_t)N);
    a.upload(c.next_new_group, &out.next_group, (size_t)1);
    c.shared_on = shared ? 1 : 0;
    // shared GPUs: the pods that ask for a fraction are in no class (brute-force scans over the nodes' GPU groups), the other classes stay indexed with the gpusharingorder bit in their
    // keys (kai_engine.hpp key_shared_layout; KAI_SHARED_INDEX=0: every scan by brute force, as before round 6); MIG rows: every scan by brute force (the class keys do not know the MIG predicates)
    out.idx_forced_off = false; out.fast_forced_off = false;
    if (shared || sp.mig) { c.all_tracked = 0; const char* e = std::getenv("KAI_SHARED_INDEX"); const int lvl = e ? std::atoi(e) : 2; if (sp.mig || lvl == 0) { c.use_index = 0; out.idx_forced_off = true; } if (sp.mig || lvl < 2) { c.fast_ok = 0; out.fast_forced_off = true; } }  // (2: gangs without a fraction pod also keep the staged job path)
    // each node's active pods in UID order: the shared-GPU guards of addTaskResources are order sensitive (nodes_fake/nodes.go:289-302 adds tasks by UID)
    std::vector<int32_t>& np_off = out.np_off; std::vector<int32_t>& np_pods = out.np_pods; np_off.assign((size_t)N + 1, 0); np_pods.clear();
    if (shared) {
        std::vector<int> order; for (int p = 0; p < P; p++) { const int st = s->pod_status[p], n = prep.pod_node[p]; if (n >= 0 && (st & KAI_POD_ACTIVE)) { order.push_back(p); np_off[n + 1]++; } }
        std::sort(order.begin(), order.end(), [&](int l, int r) { return s->pod_uid_rank[l] < s->pod_uid_rank[r]; });
        for (int n = 0; n < N; n++) np_off[n + 1] += np_off[n];
        np_pods.resize(order.size()); std::vector<int32_t> fillp(np_off.begin(), np_off.end() - 1);
        for (int p : order) np_pods[fillp[prep.pod_node[p]]++] = p;
    }
    a.upload(x.np_off, np_off.data(), np_off.size()); a.upload(x.np_pods, np_pods.data(), np_pods.size());
    return a.status();
}
// topologies + sub-group tree
template <class A> int ctx_topology(A& a, KaiCtx& c, const CtxBuildIn& in) {
    const HostPrep& prep = in.prep; const size_t S = (size_t)c.S, J = (size_t)c.J;
    c.T = prep.T; c.TL = prep.TL; c.D = prep.D; c.G = prep.G; c.W = (c.N + 31) / 32;
    a.upload(c.topo_level_off, prep.topo_level_off.data(), prep.topo_level_off.size()); a.upload(c.node_domain, prep.node_domain.data(), prep.node_domain.size());
    a.upload(c.dom_level, prep.dom_level.data(), prep.dom_level.size()); a.upload(c.dom_topo, prep.dom_topo.data(), prep.dom_topo.size());
    a.upload(c.dom_parent, prep.dom_parent.data(), prep.dom_parent.size()); a.upload(c.dom_id_rank, prep.dom_id_rank.data(), prep.dom_id_rank.size());
    a.upload(c.dom_child_off, prep.dom_child_off.data(), prep.dom_child_off.size()); a.upload(c.dom_children, prep.dom_children.data(), prep.dom_children.size());
    const size_t DT = (size_t)prep.D + prep.T;
    a.zero(c.dom_alloc_pods, DT); a.zero(c.dom_free, DT * KAI_MAX_RES); a.zero(c.dom_tmp, 3 * DT + 4); a.zero(c.dom_ratio, DT); a.zero(c.dom_key, 2 * DT);
    a.zero(c.ns_bits, (size_t)KAI_TDEPTH * std::max(c.W, 1)); a.zero(c.ns_sets, (size_t)KAI_TDEPTH * (DT + 1));
    a.zero(c.sg_score, (size_t)KAI_TKEYS * std::max<size_t>(DT, 1)); a.zero(c.sg_key, (size_t)KAI_TKEYS); a.zero(c.sg_row, (size_t)KAI_TKEYS);
    // no sub-group tree in the snapshot (HostPrep::build_topology's identity tables: one root group per job, G = J): no parent, no topology, no required / preferred level
    // anywhere (-1), name rank 0, no children, and a pod-set's group is its job — constants written in place, the pod-sets' groups copied from s_job (which the arena holds
    // already).  (One allocation order either way: the session's layout in HBM does not depend on what is sent.)
    const bool lean_groups = prep.groups_default && !in.full_uploads;
    a.upload(c.g_job, prep.g_job.data(), prep.g_job.size());
    if (lean_groups) { a.fill(c.g_parent, J, 0xFF); a.zero(c.g_name_rank, J); a.fill(c.g_topo, J, 0xFF); a.fill(c.g_req, J, 0xFF); a.fill(c.g_pref, J, 0xFF); }
    else { a.upload(c.g_parent, prep.g_parent.data(), prep.g_parent.size()); a.upload(c.g_name_rank, prep.g_name_rank.data(), prep.g_name_rank.size()); a.upload(c.g_topo, prep.g_topo.data(), prep.g_topo.size());
           a.upload(c.g_req, prep.g_req.data(), prep.g_req.size()); a.upload(c.g_pref, prep.g_pref.data(), prep.g_pref.size()); }
    a.upload(c.j_root_group, prep.j_root_group.data(), prep.j_root_group.size());
    if (lean_groups) a.zero(c.g_child_off, J + 1); else a.upload(c.g_child_off, prep.g_child_off.data(), prep.g_child_off.size());
    a.upload(c.g_children, prep.g_children.data(), prep.g_children.size());
    if (lean_groups) {
        a.copy_of(c.s_group, c.s_job, S); a.fill(c.s_topo, S, 0xFF); a.fill(c.s_req, S, 0xFF); a.fill(c.s_pref, S, 0xFF);
        a.zero(c.j_has_topology, std::max<size_t>(J, 1));
    } else {
        a.upload(c.s_group, prep.s_group.data(), prep.s_group.size()); a.upload(c.s_topo, prep.s_topo.data(), prep.s_topo.size());
        a.upload(c.s_req, prep.s_req.data(), prep.s_req.size()); a.upload(c.s_pref, prep.s_pref.data(), prep.s_pref.size());
        a.upload(c.j_has_topology, prep.j_has_topology.data(), prep.j_has_topology.size());
    }
    return a.status();
}
// dynamic state as the session-open kernels expect it, the operation logs, the kernels' scratch
template <class A> int ctx_dynamic_state(A& a, KaiCtx& c, OpenAux& x, const CtxBuildIn& in) {
    const size_t N = (size_t)c.N, P = (size_t)c.P, S = (size_t)c.S, J = (size_t)c.J, Q = (size_t)c.Q, RN = (size_t)c.R * N;
    a.copy_of(c.n_idle, c.n_alloc, RN);  // NewNodeInfo: Idle = Allocatable
    a.zero(c.n_rel, RN); a.zero(c.n_used, RN);
    a.upload(c.p_node, in.prep.pod_node.data(), P);
    a.zero(c.p_on_node, P); a.zero(c.p_on_node_status, P); a.zero(c.p_virtual, P); a.zero(c.p_accepted, P);
    a.zero(c.s_active_alloc, S); a.zero(c.s_active_used, S); a.zero(c.s_alive, S); a.zero(c.s_gated, S); a.zero(c.s_pipelined, S);
    a.zero(c.j_n_pending, J); a.zero(c.j_tta_valid, J); a.zero(c.j_tta_n, J); a.zero(c.tta, P); a.zero(c.j_tta_res, 4 * J); a.zero(c.j_allocated, 4 * J);
    a.zero(c.lq_sorted, J); a.zero(c.lq_side, J); a.zero(c.lq_cur, Q); a.zero(c.lq_end, Q); a.zero(c.lq_side_len, Q); a.zero(c.j_state, J);
    a.zero(c.qheap, Q + 1); a.zero(c.root_heap, Q + 1); a.zero(c.qn, Q + 1);
    c.ops_cap = 4 * c.P + 64; a.alloc(c.ops, (size_t)c.ops_cap);
    c.out_cap = ((int64_t)2 * c.P + 64) * in.out_lists; a.alloc(c.out_ops, (size_t)c.out_cap);
    a.zero(c.scratch, P + 64); a.zero(c.st, (size_t)1);
    a.zero(x.jsum, 9 * J); a.zero(x.weight, 3 * Q); a.zero(x.rem_amt, 3 * Q); a.zero(x.rem_has, 3 * Q); a.zero(x.best_out, (size_t)2);
    a.upload(c.q_share, in.prep.shares.data(), in.prep.shares.size());
    return a.status();
}
// everything behind the host preparation, in the order of the session's layout
template <class A> int ctx_build(A& a, KaiCtx& c, OpenAux& x, const CtxBuildIn& in, CtxBuildOut& out) {
    if (int rc = ctx_static_arrays(a, c, x, in)) return rc;
    if (int rc = ctx_shared_gpus(a, c, x, in, out)) return rc;
    return ctx_topology(a, c, in) ? a.status() : ctx_dynamic_state(a, c, x, in);
}

}  // namespace kai
