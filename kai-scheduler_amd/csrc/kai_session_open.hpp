// kai_session_open.hpp — kai_session_open's host side in its sections, the kernels behind the open and the reset (launch_open_kernels), kai_session_reset's body (reset_state).
#pragma once
#include "kai_handle.hpp"
namespace {
// session-open kernels over the HBM-resident snapshot (used by kai_session_open and kai_session_reset)
int launch_open_kernels(kai_core* core) {
    KaiCtx& c = core->ctx;
    const int N = c.N, P = c.P, J = c.J, Q = c.Q;
    const int TB = 256;
    if (core->shared) {  // shared GPUs: group tables reset, then every node adds its pods in UID order (one lane per node)
        HIP_TRY(core, hipMemsetAsync(KAI_VP(c.ng_id), 0xFF, sizeof(int32_t) * (size_t)std::max(N, 1) * KAI_GMAX, core->stream));
        if (P) hipLaunchKernelGGL(k_pod_accounting_reset, dim3((P + TB - 1) / TB), dim3(TB), 0, core->stream, c);
        if (N) hipLaunchKernelGGL(k_node_accounting_shared, dim3((N + TB - 1) / TB), dim3(TB), 0, core->stream, c, (const int32_t*)core->d_np_off, (const int32_t*)core->d_np_pods);
    } else if (P) hipLaunchKernelGGL(k_node_accounting, dim3((P + TB - 1) / TB), dim3(TB), 0, core->stream, c);
    if (core->cfg.plugins & KAI_PLUGIN_PROPORTION) {
        if (N) hipLaunchKernelGGL(k_total_nodes, dim3(std::min(1024, (N + TB - 1) / TB)), dim3(TB), 0, core->stream, c);
        if (P) hipLaunchKernelGGL(k_total_foreign, dim3((P + TB - 1) / TB), dim3(TB), 0, core->stream, c);
    }
    if (J) hipLaunchKernelGGL(k_job_usage, dim3((J + TB - 1) / TB), dim3(TB), 0, core->stream, c, core->d_jsum);
    if (core->cfg.plugins & KAI_PLUGIN_PROPORTION) {
        if (Q) hipLaunchKernelGGL(k_leaf_usage, dim3((Q + 3) / 4), dim3(TB), 0, core->stream, c, core->d_jsum);
        if (Q) hipLaunchKernelGGL(k_tree_usage, dim3(1), dim3(1024), 0, core->stream, c, (const int32_t*)core->d_h_off, (const int32_t*)core->d_h_nodes, core->n_heights);
        for (int l = 0; Q && l < core->n_levels; l++) {  // a level's totals are the fair shares of the level above: one launch per level
            const int first = core->h_lvl_off[l], count = core->h_lvl_off[l + 1] - first;
            if (count > 0) hipLaunchKernelGGL(k_fair_share_level, dim3((count * 3 + FS_WAVES - 1) / FS_WAVES), dim3(FS_WAVES * 64), 0, core->stream, c, (const int32_t*)core->d_lvl_parents, first, count,
                                              core->d_weight, core->d_rem_amt, core->d_rem_has);
        }
    }
    if (Q) hipLaunchKernelGGL(k_qnode_static, dim3((Q + TB - 1) / TB), dim3(TB), 0, core->stream, c);
    if (c.use_index && c.NB) hipLaunchKernelGGL(k_index_build, dim3((c.NB + 3) / 4), dim3(TB), 0, core->stream, c);
    HIP_TRY(core, hipGetLastError());
    return KAI_OK;
}
// ---- kai_session_open in its sections (session_open_impl below calls them in this order; the order of the allocations is the session's layout in HBM).
// checks: the dimensions, the required arrays, the fallback rules on the pods' flags, the shared-GPU model's own refusals (SharedPods)
int open_checks(kai_core* core, const kai_snapshot_soa* s, bool& any_legacy_mig) {
    const int N = s->n_nodes, P = s->n_pods, S = s->n_podsets, J = s->n_jobs, Q = s->n_queues;
    if (N < 0 || P < 0 || S < 0 || J < 0 || Q < 0) return fail(core, KAI_ERR_INVALID_ARG, "negative dimension");
    if (const char* m = HostPrep::missing_array(s)) return fail(core, KAI_ERR_INVALID_ARG, m);  // (before anything reads the snapshot's arrays; HostPrep::build reports the same)
    if (s->pod_flags) {  // one pass over the pods' flags on the host's cores: the two fallback rules (the first one wins, as when checked one after the other) and whether any pod is a legacy MIG task
        const int K = chunk_count((size_t)P);
        std::vector<unsigned char> seen((size_t)K, 0);
        parallel_chunks((size_t)P, [&](int ci, size_t p0, size_t p1) {
            unsigned char f = 0;
            for (size_t p = p0; p < p1; p++) {
                const uint32_t fl = s->pod_flags[p];
                if (!(fl & (KAI_POD_CPU_FALLBACK | KAI_POD_GPU_UNMODELLED | KAI_POD_LEGACY_MIG))) continue;
                if ((fl & KAI_POD_CPU_FALLBACK) && s->pod_status[p] == KAI_POD_PENDING) f |= 1;
                if ((fl & KAI_POD_GPU_UNMODELLED) && (s->pod_status[p] & KAI_POD_ACTIVE)) f |= 2;
                if (fl & KAI_POD_LEGACY_MIG) f |= 4;
            }
            seen[(size_t)ci] = f;
        });
        unsigned char all = 0; for (unsigned char f : seen) all |= f;
        if (all & 1) return fail(core, KAI_ERR_UNSUPPORTED, "a pending pod is flagged KAI_POD_CPU_FALLBACK: leave its job to the host path");
        if (all & 2) return fail(core, KAI_ERR_UNSUPPORTED, "an active pod holds GPU state the device does not model (gpu-memory / several fractional devices / MIG / DRA): its node's idle GPUs would be overstated");
        any_legacy_mig = all & 4;
    }
    // shared GPUs (ABI v4): fractions of one device.  One GPU memory size for the whole cluster keeps the queue-capacity step node independent.
    SharedPods& sp = core->sp;
    try { if (!sp.build(core->cfg, s)) return fail(core, KAI_ERR_UNSUPPORTED, sp.err.c_str()); }
    catch (const std::bad_alloc&) { throw; }  // (kai_session_open reports it as what it is)
    catch (const std::exception& e) { core->err = std::string("host preparation: ") + e.what(); return KAI_ERR_INVALID_ARG; }
    core->shared = sp.any;
    return KAI_OK;
}
// the snapshot's own arrays: allocated first, sent from pinned staging while the host preparation runs (UploadStage)
int open_stage_snapshot(kai_core* core, const kai_snapshot_soa* s) {
    KaiCtx& c = core->ctx; const int P = c.P, S = c.S, J = c.J, R = c.R;
    UploadStage up{core}; int rcu = 0;
    auto UP = [&](auto& field, const auto* host, size_t n) { if (!rcu) rcu = up.add(field, host, n); };
    UP(c.p_req, s->pod_req, (size_t)R * P); UP(c.p_job, s->pod_job, P); UP(c.p_podset, s->pod_podset, P);
    if (s->pod_flags) UP(c.p_flags, s->pod_flags, P); else if (!rcu) rcu = dzero_f(core, c.p_flags, (size_t)P);  // (an optional array that is absent: zeros written on the device, not 4 MB of host zeros sent over)
    if (s->pod_class) UP(c.p_class, s->pod_class, P); else if (!rcu) rcu = dzero_f(core, c.p_class, (size_t)P);
    UP(c.p_status, s->pod_status, P);
    UP(c.s_job, s->podset_job, S); UP(c.s_min, s->podset_min_available, S); UP(c.s_name_rank, s->podset_name_rank, S);
    UP(c.j_queue, s->job_queue, J); UP(c.j_prio, s->job_priority, J); UP(c.j_preempt, s->job_preemptible, J); UP(c.j_created, s->job_created_ns, J); UP(c.j_uid_rank, s->job_uid_rank, J);
    UP(c.j_first_pod, s->job_first_pod, J); UP(c.j_n_pods, s->job_n_pods, J); UP(c.j_first_ps, s->job_first_podset, J); UP(c.j_n_ps, s->job_n_podsets, J);
    return rcu ? rcu : up.flush();
}
// static arrays (optional ones get neutral defaults); nodes go up in name-rank order.  full_uploads (KAI_OPEN_FULL_UPLOADS, diagnostic): every array sent from the host, no constant written on the device
int open_static_arrays(kai_core* core, const kai_snapshot_soa* s, bool full_uploads) {
    KaiCtx& c = core->ctx; HostPrep& prep = core->prep; const int N = c.N, P = c.P, J = c.J, Q = c.Q, R = c.R;
    uint8_t one = 1;
    KAI_TRY(dupload_f(core, c.n_alloc, prep.node_alloc.data(), (size_t)R * N));
    KAI_TRY(dupload_f(core, c.n_flags, prep.node_flags.data(), (size_t)N));
    KAI_TRY(dupload_f(core, c.n_gpu_count, prep.node_gpu_count.data(), (size_t)N));
    KAI_TRY(dupload_f(core, c.n_class, prep.node_class.data(), (size_t)N));
    if (prep.any_nominated || full_uploads) KAI_TRY(dupload_f(core, c.p_nominated, prep.pod_nominated.data(), (size_t)P));
    else KAI_TRY(dfill_f(core, c.p_nominated, (size_t)P, 0xFF));  // no nominated node anywhere: -1 in every element
    KAI_TRY(dupload_f(core, c.p_scls, prep.pod_scls.data(), (size_t)P));
    KAI_TRY(dupload_f(core, c.q_parent, s->queue_parent, (size_t)Q));
    KAI_TRY(dupload_f(core, c.q_prio, s->queue_priority, (size_t)Q));
    KAI_TRY(dupload_f(core, c.q_created, s->queue_created_ns, (size_t)Q));
    KAI_TRY(dupload_f(core, c.q_uid_rank, s->queue_uid_rank, (size_t)Q));
    if (s->class_fit && s->n_pod_classes > 0 && s->n_node_classes > 0) KAI_TRY(dupload_f(core, c.class_fit, s->class_fit, (size_t)s->n_pod_classes * s->n_node_classes));
    else KAI_TRY(dupload_f(core, c.class_fit, &one, (size_t)1));
    KAI_TRY(dupload_f(core, c.j_pods_sorted, prep.sorted.data(), (size_t)P));
    KAI_TRY(dupload_f(core, c.q_child_off, prep.child_off.data(), (size_t)Q + 2));
    KAI_TRY(dupload_f(core, c.q_children, prep.children.data(), (size_t)std::max(Q, 1)));
    KAI_TRY(dupload_f(core, c.q_job_off, prep.job_off.data(), (size_t)Q + 1));
    KAI_TRY(dupload_f(core, c.jobs_static, prep.jobs_static.data(), (size_t)std::max(J, 1)));
    KAI_TRY(dupload_f(core, c.q_depth_order, prep.depth_order.data(), (size_t)Q));
    KAI_TRY(dupload_f(core, core->d_slot_queue, prep.slot_queue.data(), (size_t)std::max(J, 1)));  // (a field of the handle, not of the context: no part of a replica)
    KAI_TRY(dupload_f(core, core->d_lvl_off, prep.lvl_off.data(), prep.lvl_off.size())); KAI_TRY(dupload_f(core, core->d_lvl_parents, prep.lvl_parents.data(), prep.lvl_parents.size()));
    core->n_levels = prep.n_levels; core->h_lvl_off = prep.lvl_off; core->n_heights = prep.n_heights;
    KAI_TRY(dupload_f(core, core->d_h_off, prep.h_off.data(), prep.h_off.size())); KAI_TRY(dupload_f(core, core->d_h_nodes, prep.h_nodes.data(), prep.h_nodes.size()));
    // ---- scan classes + class index
    c.C = (int)prep.classes.size(); c.NB = (N + KAI_BLOCK - 1) / KAI_BLOCK; c.NSB = (c.NB + 63) / 64;
    c.use_index = c.C > 0 ? 1 : 0; c.all_tracked = prep.all_tracked; c.fast_ok = prep.fast_ok; core->fast_ok0 = prep.fast_ok; c.exact_sums = prep.exact_sums;
    { int d = core->cfg.queue_depth[KAI_ACTION_ALLOCATE]; c.queue_depth = d > 0 ? d : 0; }
    c.action = KAI_ACTION_ALLOCATE; c.max_consolidation_preemptees = core->cfg.max_consolidation_preemptees; c.allow_consolidating_reclaim = core->cfg.allow_consolidating_reclaim;
    c.saturation_multiplier = core->cfg.reclaimer_saturation_multiplier; c.sv = SolverCtx{}; core->solver_ready = false;
    c.use_signatures = core->cfg.use_scheduling_signatures ? 1 : 0; c.j_signature = nullptr;
    if (s->job_signature) KAI_TRY(dupload_f(core, c.j_signature, s->job_signature, (size_t)J));
    c.j_last_start = nullptr; c.q_preempt_mr = nullptr; c.q_reclaim_mr = nullptr;
    if (s->job_last_start_ns) KAI_TRY(dupload_f(core, c.j_last_start, s->job_last_start_ns, (size_t)J));
    if (s->queue_preempt_min_runtime_ns) KAI_TRY(dupload_f(core, c.q_preempt_mr, s->queue_preempt_min_runtime_ns, (size_t)Q));
    if (s->queue_reclaim_min_runtime_ns) KAI_TRY(dupload_f(core, c.q_reclaim_mr, s->queue_reclaim_min_runtime_ns, (size_t)Q));
    c.now_ns = core->cfg.now_ns; c.def_preempt_mr = core->cfg.default_preempt_min_runtime_ns; c.def_reclaim_mr = core->cfg.default_reclaim_min_runtime_ns; c.reclaim_method = core->cfg.reclaim_resolve_method;
    KAI_TRY(dupload_f(core, c.cls, prep.classes.data(), prep.classes.size())); core->cls_cap = std::max(c.C, 1);
    KAI_TRY(dzero_f(core, c.sum1_key, (size_t)std::max(c.C, 1) * std::max(c.NB, 1))); KAI_TRY(dzero_f(core, c.sum1_node, (size_t)std::max(c.C, 1) * std::max(c.NB, 1)));

    return KAI_OK;
}
// shared GPUs: per-pod portion / group, per-node GPU memory and group tables (api/node_info/gpu_sharing_node_info.go)
int open_shared_gpus(kai_core* core, const kai_snapshot_soa* s, bool full_uploads) {
    KaiCtx& c = core->ctx; HostPrep& prep = core->prep; SharedPods& sp = core->sp; const int N = c.N, P = c.P;
    const bool shared = core->shared;
    {
        std::vector<int64_t> gm((size_t)std::max(N, 1), 100);
        int32_t next_new = KAI_NEW_GROUP;
        for (int n = 0; n < N; n++) gm[n] = s->node_gpu_memory ? s->node_gpu_memory[prep.perm[n]] : 100;
        c.quota_on = sp.on ? 1 : 0; c.mig_on = sp.mig ? 1 : 0;
        for (int r = 0; r < KAI_MAX_RES; r++) { c.res_mig_g[r] = sp.mig_g[r]; c.res_mig_m[r] = sp.mig_m[r]; }
        // (both ways allocate the arrays in ONE order — the session's layout in HBM does not depend on what is sent; tests/test_open_uploads.py compares the images)
        KAI_TRY(dupload_f(core, c.p_shared, sp.shared.data(), (size_t)P));
        const size_t P1 = (size_t)std::max(P, 1);
        bool por_zero = true;  // pod_gpu_portion absent, or +0.0 in every element (what a packer that always fills the array sends for a cluster without fractions)
        if (!sp.on && s->pod_gpu_portion) {
            std::vector<char> nz((size_t)chunk_count((size_t)P), 0);
            parallel_chunks((size_t)P, [&](int ci, size_t p0, size_t p1) { for (size_t p = p0; p < p1; p++) { uint64_t b; std::memcpy(&b, &s->pod_gpu_portion[p], 8); if (b) { nz[(size_t)ci] = 1; return; } } });
            for (char x : nz) if (x) por_zero = false;
        }
        // A snapshot without shared-GPU requests and without MIG rows (SharedPods: neither `any` nor `mig`): the per-pod quantities of the shared-GPU model are constants —
        // no memory of a device asked for, no MIG quota, every GPU quantity the pod's GPU request (the row of p_req that is in HBM already), no group anywhere.  They are
        // written where they are read instead of being sent: at config 5 these arrays are 73 of the open's 190 MB over PCIe.  (kai_hostsim_run checks the same statement
        // about SharedPods on every snapshot the CPU suite runs: tests/host_sim/host_sim.cpp lean_shared_pods_hold.)
        const bool lean_pods = !sp.on && por_zero && !full_uploads;
        std::vector<double> por; std::vector<int32_t> grp, minus1;
        if (!lean_pods) {
            por.assign(P1, 0.0); grp.assign(P1, -1); minus1.assign(P1, -1);
            core->new_groups.clear();
            for (int p = 0; p < P; p++) { por[p] = s->pod_gpu_portion ? s->pod_gpu_portion[p] : 0.0; grp[p] = (s->pod_gpu_group && sp.shared[p]) ? s->pod_gpu_group[p] : -1; if (grp[p] >= next_new) next_new = grp[p] + 1; if (grp[p] >= KAI_NEW_GROUP) core->new_groups[grp[p]]++; }
        }
        auto gpu_row = [&](auto& field) -> int {  // the pods' GPU requests: a device-to-device copy of that row of p_req
            int rc2 = dalloc_f(core, field, (size_t)P); if (rc2) return rc2;
            if (P) HIP_TRY(core, hipMemcpyAsync(KAI_VP(field), (const double*)KAI_VP(c.p_req) + (size_t)KAI_RES_GPU * P, (size_t)P * sizeof(double), hipMemcpyDeviceToDevice, core->stream));
            return KAI_OK; };
        if (lean_pods) {
            KAI_TRY(dzero_f(core, c.p_mem, (size_t)P)); KAI_TRY(dzero_f(core, c.p_gmem, (size_t)P));
            KAI_TRY(gpu_row(c.p_acc_gpu)); KAI_TRY(gpu_row(c.p_pend_gpu)); KAI_TRY(gpu_row(c.p_quota_gpu));
            KAI_TRY(dzero_f(core, c.p_mig_q, (size_t)P));
        } else {
            KAI_TRY(dupload_f(core, c.p_mem, sp.mem.data(), (size_t)P)); KAI_TRY(dupload_f(core, c.p_gmem, sp.gmem.data(), (size_t)P));
            KAI_TRY(dupload_f(core, c.p_acc_gpu, sp.acc_gpu.data(), (size_t)P)); KAI_TRY(dupload_f(core, c.p_pend_gpu, sp.pend_gpu.data(), (size_t)P));
            KAI_TRY(dupload_f(core, c.p_quota_gpu, sp.quota_gpu.data(), (size_t)P)); KAI_TRY(dupload_f(core, c.p_mig_q, sp.mig_q.data(), (size_t)P));
        }
        KAI_TRY(dupload_f(core, c.p_kind, sp.kind.data(), (size_t)P));
        if (lean_pods) { KAI_TRY(dzero_f(core, c.p_portion, (size_t)P)); KAI_TRY(dfill_f(core, c.p_group, (size_t)P, 0xFF)); KAI_TRY(dfill_f(core, c.p_on_group, (size_t)P, 0xFF)); }
        else { KAI_TRY(dupload_f(core, c.p_portion, por.data(), (size_t)P)); KAI_TRY(dupload_f(core, c.p_group, grp.data(), (size_t)P)); KAI_TRY(dupload_f(core, c.p_on_group, minus1.data(), (size_t)P)); }
        KAI_TRY(dupload_f(core, c.n_gpu_mem, gm.data(), (size_t)N));
        if (lean_pods) KAI_TRY(dfill_f(core, core->d_group0, (size_t)P, 0xFF));
        else KAI_TRY(dupload_f(core, core->d_group0, grp.data(), P1));
        KAI_TRY(dalloc_f(core, c.ng_id, (size_t)N * KAI_GMAX)); KAI_TRY(dzero_f(core, c.ng_used, (size_t)N * KAI_GMAX)); KAI_TRY(dzero_f(core, c.ng_rel, (size_t)N * KAI_GMAX)); KAI_TRY(dzero_f(core, c.ng_alloc, (size_t)N * KAI_GMAX));
        KAI_TRY(dzero_f(core, c.ng_mark, (size_t)N)); KAI_TRY(dzero_f(core, c.ng_has_alloc, (size_t)N));
        KAI_TRY(dupload_f(core, c.next_new_group, &next_new, (size_t)1)); core->next_group0 = next_new;
        c.shared_on = shared ? 1 : 0;
        // shared GPUs: the pods that ask for a fraction are in no class (brute-force scans over the nodes' GPU groups), the other classes stay indexed with the gpusharingorder bit in their
        // keys (kai_engine.hpp key_shared_layout; KAI_SHARED_INDEX=0: every scan by brute force, as before round 6); MIG rows: every scan by brute force (the class keys do not know the MIG predicates)
        core->idx_forced_off = false; core->fast_forced_off = false;
        if (shared || sp.mig) { c.all_tracked = 0; const char* e = std::getenv("KAI_SHARED_INDEX"); const int lvl = e ? std::atoi(e) : 2; if (sp.mig || lvl == 0) { c.use_index = 0; core->idx_forced_off = true; } if (sp.mig || lvl < 2) { c.fast_ok = 0; core->fast_ok0 = 0; core->fast_forced_off = true; } }  // (2: gangs without a fraction pod also keep the staged job path)
        core->gm_guard = shared && s->node_gpu_memory != nullptr;
        core->h_gpu_mem.swap(gm);
        // each node's active pods in UID order: the shared-GPU guards of addTaskResources are order sensitive (nodes_fake/nodes.go:289-302 adds tasks by UID)
        std::vector<int32_t> np_off((size_t)N + 1, 0), np_pods;
        if (shared) {
            std::vector<int> order; for (int p = 0; p < P; p++) { const int st = s->pod_status[p], n = prep.pod_node[p]; if (n >= 0 && (st & KAI_POD_ACTIVE)) { order.push_back(p); np_off[n + 1]++; } }
            std::sort(order.begin(), order.end(), [&](int a, int b) { return s->pod_uid_rank[a] < s->pod_uid_rank[b]; });
            for (int n = 0; n < N; n++) np_off[n + 1] += np_off[n];
            np_pods.resize(order.size()); std::vector<int32_t> fillp(np_off.begin(), np_off.end() - 1);
            for (int p : order) np_pods[fillp[prep.pod_node[p]]++] = p;
            // (kai_session_update edits these lists by the delta: every pod's UID rank, each node's list with the ranks)
            core->np_uid.assign(s->pod_uid_rank, s->pod_uid_rank + P); core->np_lists.assign((size_t)N, {});
            for (int n = 0; n < N; n++) for (int k = np_off[n]; k < np_off[n + 1]; k++) core->np_lists[(size_t)n].push_back({s->pod_uid_rank[np_pods[k]], np_pods[k]});
        } else { core->np_uid.clear(); core->np_lists.clear(); }
        core->np_cap = np_pods.size();
        KAI_TRY(dupload_f(core, core->d_np_off, np_off.data(), np_off.size())); KAI_TRY(dupload_f(core, core->d_np_pods, np_pods.data(), np_pods.size()));
    }
    return KAI_OK;
}
// topologies + sub-group tree
int open_topology(kai_core* core, const kai_snapshot_soa* s, bool full_uploads) {
    KaiCtx& c = core->ctx; HostPrep& prep = core->prep; const int N = c.N, S = c.S, J = c.J;
    c.T = prep.T; c.TL = prep.TL; c.D = prep.D; c.G = prep.G; c.W = (N + 31) / 32;
    KAI_TRY(dupload_f(core, c.topo_level_off, prep.topo_level_off.data(), prep.topo_level_off.size())); KAI_TRY(dupload_f(core, c.node_domain, prep.node_domain.data(), prep.node_domain.size()));
    KAI_TRY(dupload_f(core, c.dom_level, prep.dom_level.data(), prep.dom_level.size())); KAI_TRY(dupload_f(core, c.dom_topo, prep.dom_topo.data(), prep.dom_topo.size()));
    KAI_TRY(dupload_f(core, c.dom_parent, prep.dom_parent.data(), prep.dom_parent.size())); KAI_TRY(dupload_f(core, c.dom_id_rank, prep.dom_id_rank.data(), prep.dom_id_rank.size()));
    KAI_TRY(dupload_f(core, c.dom_child_off, prep.dom_child_off.data(), prep.dom_child_off.size())); KAI_TRY(dupload_f(core, c.dom_children, prep.dom_children.data(), prep.dom_children.size()));
    { const size_t DT = (size_t)prep.D + prep.T;
      KAI_TRY(dzero_f(core, c.dom_alloc_pods, DT)); KAI_TRY(dzero_f(core, c.dom_free, DT * KAI_MAX_RES)); KAI_TRY(dzero_f(core, c.dom_tmp, 3 * DT + 4)); KAI_TRY(dzero_f(core, c.dom_ratio, DT)); KAI_TRY(dzero_f(core, c.dom_key, 2 * DT));
      KAI_TRY(dzero_f(core, c.ns_bits, (size_t)KAI_TDEPTH * std::max(c.W, 1))); KAI_TRY(dzero_f(core, c.ns_sets, (size_t)KAI_TDEPTH * (DT + 1)));
      KAI_TRY(dzero_f(core, c.sg_score, (size_t)KAI_TKEYS * std::max<size_t>(DT, 1))); KAI_TRY(dzero_f(core, c.sg_key, (size_t)KAI_TKEYS)); KAI_TRY(dzero_f(core, c.sg_row, (size_t)KAI_TKEYS)); }
    {   // no sub-group tree in the snapshot (HostPrep::build_topology's identity tables: one root group per job, G = J): no parent, no topology, no required / preferred level
        // anywhere (-1), name rank 0, no children, and a pod-set's group is its job — constants written on the device, the pod-sets' groups copied from s_job (in HBM already).
        // (One allocation order either way: the session's layout in HBM does not depend on what is sent.)
        const bool lean_groups = prep.groups_default && !full_uploads;
        auto minus_one = [&](auto& field, size_t n) { return dfill_f(core, field, n, 0xFF); };
        KAI_TRY(dupload_f(core, c.g_job, prep.g_job.data(), prep.g_job.size()));
        if (lean_groups) { KAI_TRY(minus_one(c.g_parent, (size_t)J)); KAI_TRY(dzero_f(core, c.g_name_rank, (size_t)J)); KAI_TRY(minus_one(c.g_topo, (size_t)J)); KAI_TRY(minus_one(c.g_req, (size_t)J)); KAI_TRY(minus_one(c.g_pref, (size_t)J)); }
        else { KAI_TRY(dupload_f(core, c.g_parent, prep.g_parent.data(), prep.g_parent.size())); KAI_TRY(dupload_f(core, c.g_name_rank, prep.g_name_rank.data(), prep.g_name_rank.size())); KAI_TRY(dupload_f(core, c.g_topo, prep.g_topo.data(), prep.g_topo.size()));
               KAI_TRY(dupload_f(core, c.g_req, prep.g_req.data(), prep.g_req.size())); KAI_TRY(dupload_f(core, c.g_pref, prep.g_pref.data(), prep.g_pref.size())); }
        KAI_TRY(dupload_f(core, c.j_root_group, prep.j_root_group.data(), prep.j_root_group.size()));
        if (lean_groups) KAI_TRY(dzero_f(core, c.g_child_off, (size_t)J + 1)); else KAI_TRY(dupload_f(core, c.g_child_off, prep.g_child_off.data(), prep.g_child_off.size()));
        KAI_TRY(dupload_f(core, c.g_children, prep.g_children.data(), prep.g_children.size()));
        if (lean_groups) {
            KAI_TRY(dalloc_f(core, c.s_group, (size_t)S));
            if (S) HIP_TRY(core, hipMemcpyAsync(KAI_VP(c.s_group), KAI_VP(c.s_job), (size_t)S * sizeof(int32_t), hipMemcpyDeviceToDevice, core->stream));
            KAI_TRY(minus_one(c.s_topo, (size_t)S)); KAI_TRY(minus_one(c.s_req, (size_t)S)); KAI_TRY(minus_one(c.s_pref, (size_t)S));
            KAI_TRY(dzero_f(core, c.j_has_topology, (size_t)std::max(J, 1)));
        } else {
            KAI_TRY(dupload_f(core, c.s_group, prep.s_group.data(), prep.s_group.size())); KAI_TRY(dupload_f(core, c.s_topo, prep.s_topo.data(), prep.s_topo.size()));
            KAI_TRY(dupload_f(core, c.s_req, prep.s_req.data(), prep.s_req.size())); KAI_TRY(dupload_f(core, c.s_pref, prep.s_pref.data(), prep.s_pref.size()));
            KAI_TRY(dupload_f(core, c.j_has_topology, prep.j_has_topology.data(), prep.j_has_topology.size()));
        }
    }

    return KAI_OK;
}
// dynamic state, the batch path's pools, the initial state kept in HBM for kai_session_reset, the context
int open_dynamic_state(kai_core* core, const kai_snapshot_soa* s) {
    KaiCtx& c = core->ctx; HostPrep& prep = core->prep; const int N = c.N, P = c.P, S = c.S, J = c.J, Q = c.Q, R = c.R;
    KAI_TRY(dalloc_f(core, c.n_idle, (size_t)R * N));
    if ((size_t)R * N) HIP_TRY(core, hipMemcpyAsync(KAI_VP(c.n_idle), KAI_VP(c.n_alloc), (size_t)R * N * sizeof(double), hipMemcpyDeviceToDevice, core->stream));  // NewNodeInfo: Idle = Allocatable
    KAI_TRY(dzero_f(core, c.n_rel, (size_t)R * N)); KAI_TRY(dzero_f(core, c.n_used, (size_t)R * N));
    KAI_TRY(dupload_f(core, c.p_node, prep.pod_node.data(), (size_t)P));
    KAI_TRY(dzero_f(core, c.p_on_node, (size_t)P)); KAI_TRY(dzero_f(core, c.p_on_node_status, (size_t)P)); KAI_TRY(dzero_f(core, c.p_virtual, (size_t)P)); KAI_TRY(dzero_f(core, c.p_accepted, (size_t)P));
    KAI_TRY(dzero_f(core, c.s_active_alloc, (size_t)S)); KAI_TRY(dzero_f(core, c.s_active_used, (size_t)S)); KAI_TRY(dzero_f(core, c.s_alive, (size_t)S)); KAI_TRY(dzero_f(core, c.s_gated, (size_t)S)); KAI_TRY(dzero_f(core, c.s_pipelined, (size_t)S));
    KAI_TRY(dzero_f(core, c.j_n_pending, (size_t)J)); KAI_TRY(dzero_f(core, c.j_tta_valid, (size_t)J)); KAI_TRY(dzero_f(core, c.j_tta_n, (size_t)J)); KAI_TRY(dzero_f(core, c.tta, (size_t)P));
    KAI_TRY(dzero_f(core, c.j_tta_res, (size_t)4 * J)); KAI_TRY(dzero_f(core, c.j_allocated, (size_t)4 * J));
    KAI_TRY(dzero_f(core, c.lq_sorted, (size_t)J)); KAI_TRY(dzero_f(core, c.lq_side, (size_t)J)); KAI_TRY(dzero_f(core, c.lq_cur, (size_t)Q)); KAI_TRY(dzero_f(core, c.lq_end, (size_t)Q)); KAI_TRY(dzero_f(core, c.lq_side_len, (size_t)Q));
    KAI_TRY(dzero_f(core, c.j_state, (size_t)J));
    KAI_TRY(dzero_f(core, c.qheap, (size_t)Q + 1)); KAI_TRY(dzero_f(core, c.root_heap, (size_t)Q + 1)); KAI_TRY(dzero_f(core, c.qn, (size_t)Q + 1));
    c.ops_cap = 4 * P + 64; KAI_TRY(dalloc_f(core, c.ops, (size_t)c.ops_cap));
    c.out_cap = (int64_t)2 * P + 64; KAI_TRY(dalloc_f(core, c.out_ops, (size_t)c.out_cap));
    KAI_TRY(dzero_f(core, c.scratch, (size_t)P + 64));
    KAI_TRY(dzero_f(core, c.st, (size_t)1));
    KAI_TRY(dzero_f(core, core->d_jsum, (size_t)9 * J));
    KAI_TRY(dzero_f(core, core->d_weight, (size_t)3 * Q)); KAI_TRY(dzero_f(core, core->d_rem_amt, (size_t)3 * Q)); KAI_TRY(dzero_f(core, core->d_rem_has, (size_t)3 * Q));
    KAI_TRY(dzero_f(core, core->d_best_out, (size_t)2));
    KAI_TRY(dupload_f(core, c.q_share, prep.shares.data(), prep.shares.size()));
    // batch path of the allocate action (kai_batch.hpp): its pools and tables, when the snapshot admits it
    core->shape = prep.shape;
    KAI_TRY(bind_batch_pools(core));
    if (core->shared) c.bt.enabled = 0;
    // keep the initial dynamic state in HBM so that kai_session_reset needs no host traffic
    KAI_TRY(dalloc(core, &core->d_status0, (size_t)P)); KAI_TRY(dalloc(core, &core->d_node0, (size_t)P)); KAI_TRY(dalloc(core, &core->d_shares0, (size_t)std::max(Q, 1) * 3));
    if (P) { HIP_TRY(core, hipMemcpyAsync(core->d_status0, KAI_VP(c.p_status), (size_t)P * 4, hipMemcpyDeviceToDevice, core->stream));
             HIP_TRY(core, hipMemcpyAsync(core->d_node0, KAI_VP(c.p_node), (size_t)P * 4, hipMemcpyDeviceToDevice, core->stream)); }
    HIP_TRY(core, hipMemcpyAsync(core->d_shares0, KAI_VP(c.q_share), (size_t)std::max(Q, 1) * 3 * sizeof(QShare), hipMemcpyDeviceToDevice, core->stream));
    { KaiCtx* t = nullptr; KAI_TRY(dalloc(core, &t, (size_t)1)); core->d_ctx = t; }
    HIP_TRY(core, hipMemcpyAsync(core->d_ctx, &core->ctx, sizeof(KaiCtx), hipMemcpyHostToDevice, core->stream));
    return KAI_OK;
}
// slabs of earlier (larger) sessions this open did not take: keep two for what the session's actions still allocate (solver scratch, batch pools), release the rest
// ... and the smallest one that holds the LARGEST request the last session made after its open (post_open_max: a victim action's replicas, the batch pools) — or that request
// would pay a hipMalloc every cycle and a hipFree at the next trim, which is what keeping slabs is there to avoid
void trim_spare(kai_core* core) {
    if (core->spare.size() > 2) {
        std::sort(core->spare.begin(), core->spare.end(), [](const std::pair<void*, size_t>& a, const std::pair<void*, size_t>& b) { return a.second < b.second; });
        size_t keep_big = core->spare.size();
        for (size_t i = 2; i < core->spare.size(); i++) if (core->post_open_max > 0 && core->spare[i].second >= core->post_open_max) { keep_big = i; break; }
        if (core->post_open_max > 0 && (core->spare[0].second >= core->post_open_max || core->spare[1].second >= core->post_open_max)) keep_big = core->spare.size();  // (one of the two small ones already holds it)
        std::vector<std::pair<void*, size_t>> kept;
        for (size_t i = 0; i < core->spare.size(); i++) { if (i < 2 || i == keep_big) kept.push_back(core->spare[i]); else (void)hipFree(core->spare[i].first); }
        core->spare.swap(kept);
    }
}

int session_open_impl(kai_core* core, const kai_snapshot_soa* s) {
    if (s->abi_version != KAI_ABI_VERSION || s->n_res < 4 || s->n_res > KAI_MAX_RES) return fail(core, KAI_ERR_INVALID_ARG, "bad abi_version / n_res");
    HIP_TRY(core, hipSetDevice(core->device));
    const bool prof_open = std::getenv("KAI_PROF") != nullptr;  // host clocks of the open: where a production cycle's per-cycle cost goes (stderr)
    auto tnow = [] { return std::chrono::steady_clock::now(); };
    const auto t_begin = tnow();
    free_session(core);
    const auto t_freed = tnow();
    bool any_legacy_mig = false;
    KAI_TRY(open_checks(core, s, any_legacy_mig));
    HIP_TRY(core, hipEventRecord(core->ev0, core->stream));
    const int N = s->n_nodes, P = s->n_pods, S = s->n_podsets, J = s->n_jobs, Q = s->n_queues, R = s->n_res;
    KaiCtx& c = core->ctx;
    c = KaiCtx{};
    c.N = N; c.P = P; c.S = S; c.J = J; c.Q = Q; c.R = R; c.n_pod_classes = std::max(1, s->n_pod_classes); c.n_node_classes = std::max(1, s->n_node_classes);
    c.plugins = core->cfg.plugins; c.gpu_strategy = core->cfg.gpu_strategy; c.cpu_strategy = core->cfg.cpu_strategy;
    c.restrict_nodes = core->cfg.restrict_node_scheduling; c.k_value = core->cfg.k_value <= 0.0 ? 0.0 : core->cfg.k_value;  // proportion.go:77-84

    const auto t_shared = tnow();
    KAI_TRY(open_stage_snapshot(core, s));
    // ---- index structures (pure re-orderings / groupings of the input; kai_host_prep.hpp)
    const auto t_staged = tnow();
    HostPrep& prep = core->prep; SharedPods& sp = core->sp;
    prep.shared_pods = sp.any ? &sp : nullptr;
    try { if (prep.build(core->cfg, s, core->err)) return KAI_ERR_INVALID_ARG; }  // (the staged copies read the handle's pinned buffer: kai_session_open drains the stream on every failure)
    catch (const std::bad_alloc&) { throw; }  // (a worker thread's included: kai_parallel.hpp carries it here)
    catch (const std::exception& e) { core->err = std::string("host preparation: ") + e.what(); return KAI_ERR_INVALID_ARG; }
    const auto t_prep = tnow();
    core->legacy_on = any_legacy_mig; core->legacy_cnt.clear();
    if (any_legacy_mig) { core->legacy_cnt.assign((size_t)N, 0); for (int p = 0; p < P; p++)  // NodeInfo.LegacyMIGTasks (node_info.go:407-409): a node that holds a legacy MIG task takes no MIG request
        if ((s->pod_flags[p] & KAI_POD_LEGACY_MIG) && prep.pod_node[p] >= 0 && (s->pod_status[p] & KAI_POD_ACTIVE)) { prep.node_flags[prep.pod_node[p]] |= KAI_NODE_LEGACY_MIG_I; core->legacy_cnt[(size_t)prep.pod_node[p]]++; } }
    core->perm = prep.perm; core->bn_perm_ok = false; core->oa_rank_ok = false;

    const bool full_uploads = std::getenv("KAI_OPEN_FULL_UPLOADS") != nullptr;
    KAI_TRY(open_static_arrays(core, s, full_uploads));
    KAI_TRY(open_shared_gpus(core, s, full_uploads));
    KAI_TRY(open_topology(core, s, full_uploads));
    KAI_TRY(open_dynamic_state(core, s));
    if (std::getenv("KAI_OPEN_DIGEST")) {  // diagnostic: what the open put into every array of the session context, before its first kernel (FNV-1a per KaiCtx field; tests/test_open_uploads.py)
        HIP_TRY(core, hipStreamSynchronize(core->stream));
        for (const kai_core::AllocRec& a : core->allocs) {
            std::vector<unsigned char> h(a.bytes);
            HIP_TRY(core, hipMemcpyAsync(h.data(), a.base, a.bytes, hipMemcpyDeviceToHost, core->stream)); HIP_TRY(core, hipStreamSynchronize(core->stream));
            uint64_t f = 1469598103934665603ull; for (unsigned char x : h) { f ^= x; f *= 1099511628211ull; }
            std::fprintf(stderr, "kai open digest: field %zu bytes %zu fnv %016llx\n", a.field_off, a.bytes, (unsigned long long)f);
        }
    }
    KAI_TRY(launch_open_kernels(core)); core->index_stale = false;
    HIP_TRY(core, hipEventRecord(core->ev1, core->stream));
    const auto t_enq = tnow();
    HIP_TRY(core, hipStreamSynchronize(core->stream));  // prep's host buffers die with this scope
    if (prof_open) std::fprintf(stderr, "kai open: free %.2f ms, checks + shared pods %.2f, the snapshot's arrays staged %.2f, host prep %.2f, allocate + enqueue uploads %.2f, wait %.2f | total %.2f ms\n",
                                ms_between(t_begin, t_freed), ms_between(t_freed, t_shared), ms_between(t_shared, t_staged), ms_between(t_staged, t_prep), ms_between(t_prep, t_enq), ms_between(t_enq, tnow()), ms_between(t_begin, tnow()));
    if (prof_open) std::fprintf(stderr, "kai open: host prep by phase: range checks %.2f, nodes %.2f, pods %.2f, task order %.2f, queues + job lists %.2f, shares + topology %.2f, classes %.2f, batch shape %.2f ms on %d host threads\n",
                                prep.phase_ms[0], prep.phase_ms[1], prep.phase_ms[2], prep.phase_ms[3], prep.phase_ms[4], prep.phase_ms[5], prep.phase_ms[6], prep.phase_ms[7], host_threads());
    float ms = 0; HIP_TRY(core, hipEventElapsedTime(&ms, core->ev0, core->ev1));
    std::memset(&core->stats, 0, sizeof(core->stats));
    core->stats.upload_ms = ms;
    trim_spare(core);
    core->post_open_max = 0;  // (counted from here on: dalloc)
    core->open = true; core->err = "ok";
    return KAI_OK;
}
// the session's dynamic state from the HBM-resident snapshot: kai_session_reset, and kai_session_update after its scatter
int reset_state(kai_core* core) {
    KaiCtx& c = core->ctx;
    const size_t RN = (size_t)c.R * c.N;
    HIP_TRY(core, hipEventRecord(core->ev0, core->stream));
    if (RN) { HIP_TRY(core, hipMemcpyAsync(KAI_VP(c.n_idle), KAI_VP(c.n_alloc), RN * 8, hipMemcpyDeviceToDevice, core->stream));
              HIP_TRY(core, hipMemsetAsync(KAI_VP(c.n_rel), 0, RN * 8, core->stream)); HIP_TRY(core, hipMemsetAsync(KAI_VP(c.n_used), 0, RN * 8, core->stream)); }
    if (c.P) { HIP_TRY(core, hipMemcpyAsync(KAI_VP(c.p_status), core->d_status0, (size_t)c.P * 4, hipMemcpyDeviceToDevice, core->stream));
               HIP_TRY(core, hipMemcpyAsync(KAI_VP(c.p_node), core->d_node0, (size_t)c.P * 4, hipMemcpyDeviceToDevice, core->stream)); }
    HIP_TRY(core, hipMemcpyAsync(KAI_VP(c.q_share), core->d_shares0, (size_t)std::max(c.Q, 1) * 3 * sizeof(QShare), hipMemcpyDeviceToDevice, core->stream));
    c.fast_ok = core->fast_ok0;
    if (c.P) HIP_TRY(core, hipMemcpyAsync(KAI_VP(c.p_group), core->d_group0, (size_t)c.P * 4, hipMemcpyDeviceToDevice, core->stream));
    HIP_TRY(core, hipMemcpyAsync(KAI_VP(c.next_new_group), &core->next_group0, 4, hipMemcpyHostToDevice, core->stream));
    { const size_t NG = (size_t)std::max(c.N, 1) * KAI_GMAX;
      HIP_TRY(core, hipMemsetAsync(KAI_VP(c.ng_used), 0, NG * 8, core->stream)); HIP_TRY(core, hipMemsetAsync(KAI_VP(c.ng_rel), 0, NG * 8, core->stream)); HIP_TRY(core, hipMemsetAsync(KAI_VP(c.ng_alloc), 0, NG * 8, core->stream));
      HIP_TRY(core, hipMemsetAsync(KAI_VP(c.ng_mark), 0, (size_t)std::max(c.N, 1) * 4, core->stream)); HIP_TRY(core, hipMemsetAsync(KAI_VP(c.ng_has_alloc), 0, (size_t)std::max(c.N, 1) * 4, core->stream)); }
    if (core->solver_ready) HIP_TRY(core, hipMemsetAsync(c.sv.xr_key, 0xFF, sizeof(int64_t) * ((size_t)c.sv.xr_mask + 1), core->stream));
    HIP_TRY(core, hipMemsetAsync(KAI_VP(c.st), 0, sizeof(EngineState), core->stream));
    KAI_TRY(launch_open_kernels(core));
    core->index_stale = false;
    HIP_TRY(core, hipEventRecord(core->ev1, core->stream));
    HIP_TRY(core, hipStreamSynchronize(core->stream));
    float ms = 0; HIP_TRY(core, hipEventElapsedTime(&ms, core->ev0, core->ev1));
    core->stats.upload_ms = ms;
    return KAI_OK;
}
}  // namespace
